"""The neighbour-graph index with upper levels (mevi_amd/hnsw.py, entry="levels") on 6000 x 32, M = 4, 64 entry rows -- levels
6000 / 1500 / 375 / 93 walked and 23 scanned -- against the oracle: sizes, maps, every level's kNN lists and graph, the search as
the reference chain (top scan, descent, level-0 walk), graph replay, the fallback to the strided index, and `faiss_search.py
--param HNSW4` with MEVI_HNSW_ENTRY=levels through its command line.  Bar: bit equality (tests/graph_level_cases.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import graph_cases as gc
import graph_level_cases as glc
from mevi_amd import hnsw
from oracle import dense as odense

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND, DIM, M, NQ, ENTRY_ROWS, EF_UPPER = 6000, 32, 4, 32, 64, 32
SIZES = [6000, 1500, 375, 93, 23]


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(0)
    docs = gc.clustered(rng, ND, DIM, 300)
    q = (docs[rng.integers(0, ND, NQ)] + 0.1 * rng.standard_normal((NQ, DIM))).astype(np.float32)
    down, rows = glc.level_maps(SIZES)
    knn = [odense.ip_topk_exact(docs, docs, M + 1)[1]]
    for l in range(1, len(SIZES) - 1):
        level_docs = np.ascontiguousarray(docs[rows[l - 1]])
        knn.append(odense.ip_topk_exact(level_docs, level_docs, M + 1)[1])
    return docs, q, knn, [gc.link_expected(x, M) for x in knn], down, rows, gc.all_scores(q, docs)


@pytest.fixture(scope="module")
def index(case):
    return hnsw.HNSWIndex(torch.from_numpy(case[0]).cuda(), M, entry="levels", entry_rows=ENTRY_ROWS, ef_upper=EF_UPPER, width_upper=1)


def _same(got, want):
    s, i = got
    torch.cuda.synchronize()
    np.testing.assert_array_equal(i.cpu().numpy(), want[1])
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), want[0].view(np.uint32))


def test_sizes_maps_lists_and_graphs_are_the_oracles(cuda, case, index):
    docs, q, knn, graphs, down, rows, sc = case
    assert glc.level_sizes(ND, M, ENTRY_ROWS) == SIZES == index.level_n and index.entry == "levels"
    assert index.entry_name() == "levels(1500/375/93/23)" and index.degree == 2 * M
    np.testing.assert_array_equal(index.knn.cpu().numpy(), knn[0])
    np.testing.assert_array_equal(index.graph.cpu().numpy(), graphs[0])
    assert len(index.level_knn) == 3
    for l in range(1, 4):
        np.testing.assert_array_equal(index.level_knn[l - 1].cpu().numpy(), knn[l])
    assert index.level_graphs.dtype == index.level_rows.dtype == index.level_down.dtype == torch.int32
    np.testing.assert_array_equal(index.level_graphs.cpu().numpy(), np.concatenate(graphs[1:]))
    np.testing.assert_array_equal(index.level_rows.cpu().numpy(), np.concatenate(rows[:3]))
    np.testing.assert_array_equal(index.level_down.cpu().numpy(), np.concatenate(down[:3]))
    np.testing.assert_array_equal(index.entry_ids.cpu().numpy(), down[3])      # the scan names nodes of level 3
    np.testing.assert_array_equal(index.entry_docs.cpu().numpy(), docs[rows[3]])
    assert index.nseed == 23 and index.walk_nseed == 32 and index.upper == (32, 1, 128)
    upper = sum(SIZES[1:4])
    assert index.graph_bytes() == ND * 8 * 4 + 23 * DIM * 4 + 23 * 8 + upper * 8 * 4 + upper * 4 + upper * 4


@pytest.mark.parametrize("k,ef_search", [(10, 16), (100, 16)])
def test_search_equals_the_reference_chain(cuda, case, index, k, ef_search):
    docs, q, knn, graphs, down, rows, sc = case
    tq = torch.from_numpy(q).cuda()
    top, top_score = glc.top_seeds_expected(sc, rows[3], down[3], 32)
    s, i = index.seeds(tq)
    _same((s, i), (top_score, top))
    seed, seed_score, down_steps, scored = glc.descend_expected(sc, ND, graphs[1:], rows[:3], down[:3], top, top_score, EF_UPPER, 1,
                                                                4 * EF_UPPER, 32)
    got = index.descend(tq, i, s)
    _same((got[1], got[0]), (seed_score, seed))
    ef, width, max_steps = index.plan(k, ef_search, None)
    assert (ef, width, max_steps) == (max(16, k), 1, 4 * max(16, k))
    want = gc.search_expected(sc, graphs[0], seed, k, ef, 1, max_steps, seed_score=seed_score)
    steps = torch.zeros(NQ, dtype=torch.int32, device="cuda")
    dsteps = torch.zeros(NQ, dtype=torch.int32, device="cuda")
    _same(index.search(tq, k, ef_search, steps=steps, descent_steps=dsteps), want)
    np.testing.assert_array_equal(steps.cpu().numpy(), want[2])
    np.testing.assert_array_equal(dsteps.cpu().numpy(), down_steps)
    assert (down_steps >= 3).all()


def test_replay_equals_eager(cuda, case, index):
    docs, q = case[0], case[1]
    for nq in (1, 32):
        tq = torch.from_numpy(q[:nq]).cuda()
        eager = index.search(tq, 10, 16)
        replay = index.search_graph(nq, 10, 16)
        for _ in range(2):
            got = replay.run(tq)
            assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1])
    with pytest.raises(ValueError):
        index.search_graph(33, 10, 16)


def test_levels_without_a_walked_level_is_the_strided_index(cuda):
    rng = np.random.default_rng(4096)
    docs = torch.from_numpy(gc.clustered(rng, 4096, 32, 64)).cuda()
    q = docs[:16] + 0.25
    strided = hnsw.HNSWIndex(docs, 8, entry="strided")
    asked = hnsw.HNSWIndex(docs, 8, knn=strided.knn, graph=strided.graph, entry="levels")
    assert asked.entry == "strided" == strided.entry and asked.entry_name() == "strided" and asked.level_n == [4096]
    assert not hasattr(asked, "level_graphs") and torch.equal(asked.entry_ids, strided.entry_ids)
    assert asked.graph_bytes() == strided.graph_bytes() and asked.walk_nseed == asked.nseed == 32
    a, b = asked.search(q, 10), strided.search(q, 10)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match="entry"):
        hnsw.HNSWIndex(docs, 8, knn=strided.knn, graph=strided.graph, entry="random")


def test_cli_descends_levels_and_exact_restores_flat(cuda, tmp_path):
    """`faiss_search.py --param HNSW4 --dim 16` over 20 000 rows with MEVI_HNSW_ENTRY=levels: levels 20000 / 5000 walked, 1250
    scanned; the recall line on stderr names them; with MEVI_HNSW=exact the output file is the `--param Flat` file byte for byte."""
    rng = np.random.default_rng(8)
    nq, nd, dim, k = 5, 20000, 16, 10
    d = gc.clustered(rng, nd, dim, 100)
    q = (d[rng.integers(0, nd, nq)] + 0.3 * rng.standard_normal((nq, dim))).astype(np.float32)
    q.tofile(tmp_path / "q.bin")
    d.tofile(tmp_path / "d.bin")
    with open(tmp_path / "raw.tsv", "w") as f:
        for i in range(nq):
            f.write(f"q{i}\t{i}\n")
    clean = {n: v for n, v in os.environ.items() if not n.startswith("MEVI_HNSW")}

    def run(param, out, **env):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "faiss_search.py"), "--query_path", str(tmp_path / "q.bin"), "--doc_path",
                            str(tmp_path / "d.bin"), "--output_path", str(tmp_path / out), "--raw_query_path", str(tmp_path / "raw.tsv"),
                            "--dim", str(dim), "--topk", str(k), "--param", param], capture_output=True, text=True,
                           env=dict(clean, PYTHONPATH=ROOT, **env))
        assert r.returncode == 0, r.stderr[-1500:]
        return r

    r = run("HNSW4", "hnsw.tsv", MEVI_HNSW_ENTRY="levels")
    assert "Param HNSW4 trained: True." in r.stdout and f"int64 ({nq}, {k}) float32 ({nq}, {k})" in r.stdout
    line = [l for l in r.stderr.splitlines() if "recall vs exact search" in l]
    assert len(line) == 1 and "HNSW4 efSearch=16 width=1 entry=levels(5000/1250):" in line[0] and "@1 " in line[0] and "@10 " in line[0]
    assert "steps: mean" in line[0] and "max_steps=64" in line[0] and "descent (ef 32, width 4) steps: mean" in line[0]
    size = nd * 8 * 4 + 1250 * dim * 4 + 1250 * 8 + 5000 * 8 * 4 + 5000 * 4 + 5000 * 4
    assert f"{size} bytes of graph" in line[0]
    rows = [l.rstrip("\n").split("\t") for l in open(tmp_path / "hnsw.tsv")]
    assert len(rows) == nq and all(len(r_[2].split(",")) == k for r_ in rows)
    exact = run("HNSW4", "exact.tsv", MEVI_HNSW="exact", MEVI_HNSW_ENTRY="levels")
    assert "Param HNSW4 trained: True." in exact.stdout and "recall vs exact search" not in exact.stderr
    run("Flat", "flat.tsv")
    assert open(tmp_path / "exact.tsv", "rb").read() == open(tmp_path / "flat.tsv", "rb").read()
