"""The neighbour-graph index (mevi_amd/hnsw.py) on 4096 x 32 against the oracle: kNN lists, graph, search with the oracle's seeds,
top-1, graph replay, `faiss_search.py --param HNSW8` through its command line, MEVI_HNSW=exact.  Bar: bit equality
(tests/graph_cases.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import graph_cases as gc
from mevi_amd import hnsw
from oracle import dense as odense

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND, DIM, M, NQ = 4096, 32, 8, 32


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(4096)
    docs = gc.clustered(rng, ND, DIM, 64)
    q = (docs[rng.integers(0, ND, NQ)] + 0.3 * rng.standard_normal((NQ, DIM))).astype(np.float32)
    knn = odense.ip_topk_exact(docs, docs, M + 1)[1]
    return docs, q, knn, gc.link_expected(knn, M), gc.all_scores(q, docs)


@pytest.fixture(scope="module")
def index(case):
    return hnsw.HNSWIndex(torch.from_numpy(case[0]).cuda(), M)


def _same(got, want):
    s, i = got
    torch.cuda.synchronize()
    np.testing.assert_array_equal(i.cpu().numpy(), want[1])
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), want[0].view(np.uint32))


def test_lists_graph_and_entry_rows_are_the_oracles(cuda, case, index):
    docs, q, knn, graph, sc = case
    np.testing.assert_array_equal(index.knn.cpu().numpy(), knn)
    np.testing.assert_array_equal(index.graph.cpu().numpy(), graph)
    np.testing.assert_array_equal(index.entry_ids.cpu().numpy(), gc.entry_rows(ND))
    assert index.nseed == hnsw.N_SEEDS == 32 and index.degree == 2 * M
    big = hnsw.entry_rows(10 ** 7 + 3, "cpu").numpy()                   # the stride on a corpus past ENTRY_ROWS
    assert np.array_equal(big, gc.entry_rows(10 ** 7 + 3)) and len(big) == hnsw.ENTRY_ROWS and big[1] == (10 ** 7 + 3) // 4096


@pytest.mark.parametrize("k,ef_search,width", [(10, None, None), (10, 64, 1), (100, 16, 2), (1, 1, 1)])
def test_search_equals_the_reference_with_the_oracles_seeds(cuda, case, index, k, ef_search, width):
    docs, q, knn, graph, sc = case
    tq = torch.from_numpy(q).cuda()
    seed, seed_score = gc.seeds_expected(sc, 32)
    s, i = index.seeds(tq)
    _same((s, i), (seed_score, seed.astype(np.int64)))
    ef, w, max_steps = index.plan(k, ef_search, width)
    assert ef == max(16 if ef_search is None else ef_search, k) and w == (1 if width is None else width) and max_steps == 4 * ef
    want = gc.search_expected(sc, graph, seed, k, ef, w, max_steps, seed_score=seed_score)
    steps = torch.zeros(NQ, dtype=torch.int32, device="cuda")
    _same(index.search(tq, k, ef_search, width, steps=steps), want)
    np.testing.assert_array_equal(steps.cpu().numpy(), want[2])
    exact = odense.ip_topk_exact(q, docs, 1)
    assert np.array_equal(want[1][:, 0], exact[1][:, 0])               # nd <= ENTRY_ROWS: the best row is a seed, never evicted


def test_replay_equals_eager(cuda, case, index):
    docs, q, knn, graph, sc = case
    for nq in (1, 32):
        tq = torch.from_numpy(q[:nq]).cuda()
        eager = index.search(tq, 10, 64)
        replay = index.search_graph(nq, 10, 64)
        for _ in range(2):
            got = replay.run(tq)
            assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1])
    with pytest.raises(ValueError):
        index.search_graph(33, 10, 64)


def test_cli_serves_the_factory_string_and_exact_restores_flat(cuda, tmp_path):
    """`faiss_search.py --param HNSW8 --dim 16` over 2000 rows: the reference's stdout lines, the recall line on stderr; with
    MEVI_HNSW=exact the output file is the `--param Flat` file byte for byte."""
    rng = np.random.default_rng(8)
    nq, nd, dim, k = 5, 2000, 16, 10
    d = gc.clustered(rng, nd, dim, 16)
    q = (d[rng.integers(0, nd, nq)] + 0.3 * rng.standard_normal((nq, dim))).astype(np.float32)
    q.tofile(tmp_path / "q.bin")
    d.tofile(tmp_path / "d.bin")
    with open(tmp_path / "raw.tsv", "w") as f:
        for i in range(nq):
            f.write(f"q{i}\t{i}\n")

    def run(param, out, **env):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "faiss_search.py"), "--query_path", str(tmp_path / "q.bin"), "--doc_path",
                            str(tmp_path / "d.bin"), "--output_path", str(tmp_path / out), "--raw_query_path", str(tmp_path / "raw.tsv"),
                            "--dim", str(dim), "--topk", str(k), "--param", param], capture_output=True, text=True,
                           env=dict(os.environ, PYTHONPATH=ROOT, **env))
        assert r.returncode == 0, r.stderr[-1500:]
        return r

    r = run("HNSW8", "hnsw.tsv")
    assert "Param HNSW8 trained: True." in r.stdout and f"int64 ({nq}, {k}) float32 ({nq}, {k})" in r.stdout
    line = [l for l in r.stderr.splitlines() if "recall vs exact search" in l]
    assert len(line) == 1 and "HNSW8 efSearch=16 width=1" in line[0] and "@1 " in line[0] and "@10 " in line[0]
    assert "steps: mean" in line[0] and "max_steps=64" in line[0] and f"{nd * 16 * 4 + nd * dim * 4 + nd * 8} bytes of graph" in line[0]
    rows = [l.rstrip("\n").split("\t") for l in open(tmp_path / "hnsw.tsv")]
    assert len(rows) == nq and all(len(r_[2].split(",")) == k for r_ in rows)
    exact = run("HNSW8", "exact.tsv", MEVI_HNSW="exact")
    assert "Param HNSW8 trained: True." in exact.stdout and "recall vs exact search" not in exact.stderr
    run("Flat", "flat.tsv")
    assert open(tmp_path / "exact.tsv", "rb").read() == open(tmp_path / "flat.tsv", "rb").read()
