"""RefineIndex (mevi_amd/refine.py) behind every compressed family, given centroids, codebooks and R: its search is the reference
of tests/refine_cases.py applied to the inner index's own candidates, bit for bit; with every row a candidate it is the exact
search; what refine buys per query; the routing of dense.search / dense.profile / `faiss_search.py --param PQ8,RFlat`."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import refine_cases as rc
from mevi_amd import dense, ivfpq, opq, pqfs, refine, sq
from oracle import dense as odense

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND, NQ, DIM, M, NLIST, K = 3000, 12, 32, 8, 7, 10
ENV = ("MEVI_REFINE", "MEVI_REFINE_K_FACTOR", "MEVI_IVFPQ", "MEVI_PQFS", "MEVI_SQ", "MEVI_OPQ", "MEVI_OPQ_NITER", "MEVI_IVF_NPROBE")


def _bits(a):
    return a.view(np.uint32)


@functools.lru_cache(maxsize=None)
def _corpus():
    """(docs, queries, centroids, R, {nbits: codebook}, exact top-(K + 1) of the oracle): shared, so nobody writes to them.  The
    codebooks are random: the index only has to return SOME candidates."""
    rng = np.random.default_rng(43)
    centres = rng.standard_normal((NLIST, DIM)).astype(np.float32) * 2
    d = (centres[rng.integers(0, NLIST, size=ND)] + rng.standard_normal((ND, DIM))).astype(np.float32)
    q = (centres[rng.integers(0, NLIST, size=NQ)] + rng.standard_normal((NQ, DIM))).astype(np.float32)
    R = opq.random_rotation(DIM, 19).astype(np.float32)
    books = {b: (rng.standard_normal((M, 1 << b, DIM // M)) * 0.8).astype(np.float32) for b in (8, 4)}
    return d, q, centres, R, books, odense.ip_topk_exact(q, d, K + 1)


FAMILIES = ["PQ8", "IVF7,PQ8", "PQ8x4", "IVF7,PQ8x4fs", "OPQ8,IVF7,PQ8", "SQ8", "IVF7,SQ4"]


@functools.lru_cache(maxsize=None)
def _inner(name):
    d, _, centres, R, books, _ = _corpus()
    dt = torch.from_numpy(np.array(d)).cuda()
    cent = torch.from_numpy(np.array(centres))
    book = {b: torch.from_numpy(np.array(v)) for b, v in books.items()}
    if name == "PQ8":
        return ivfpq.IVFPQIndex(dt, None, M, 8, codebook=book[8])
    if name == "IVF7,PQ8":
        return ivfpq.IVFPQIndex(dt, NLIST, M, 8, centroids=cent, codebook=book[8])
    if name == "PQ8x4":
        return ivfpq.IVFPQIndex(dt, None, M, 4, codebook=book[4])
    if name == "IVF7,PQ8x4fs":
        return pqfs.PQFSIndex(dt, NLIST, M, centroids=cent, codebook=book[4])
    if name == "OPQ8,IVF7,PQ8":
        return opq.OPQIndex(dt, M, NLIST, M, 8, False, R=torch.from_numpy(np.array(R)), centroids=cent, codebook=book[8])
    if name == "SQ8":
        return sq.SQIndex(dt, None, 8)
    assert name == "IVF7,SQ4"
    return sq.SQIndex(dt, NLIST, 4, centroids=cent)


@functools.lru_cache(maxsize=None)
def _docs_on():
    return torch.from_numpy(np.array(_corpus()[0])).cuda()


def _queries_on():
    return torch.from_numpy(np.array(_corpus()[1])).cuda()


@pytest.mark.parametrize("k_factor", [1, 4])
@pytest.mark.parametrize("name", FAMILIES)
def test_search_is_the_reference_over_the_inner_candidates(cuda, name, k_factor):
    d, q, _, _, _, _ = _corpus()
    inner = _inner(name)
    index = refine.RefineIndex(inner, _docs_on())
    assert index.docs.data_ptr() == _docs_on().data_ptr()                    # a reference to the resident rows, not a copy
    nprobe = 2
    _, cand = inner.search(_queries_on(), K * k_factor, nprobe)
    s, i = index.search(_queries_on(), K, nprobe, k_factor=k_factor)
    torch.cuda.synchronize()
    cand = cand.cpu().numpy()
    assert cand.shape == (NQ, K * k_factor) and torch.equal(index.last_candidates[0].cpu(), torch.from_numpy(cand))
    want = rc.refine_expected(q, d, cand, K)
    np.testing.assert_array_equal(i.cpu().numpy(), want[1])
    np.testing.assert_array_equal(_bits(s.cpu().numpy()), _bits(want[0]))
    np.testing.assert_array_equal(index.last_candidates[1].cpu().numpy(), want[2])
    assert (want[2] == K * k_factor).all()                                   # two lists of ~430 rows hold that many


def test_every_row_a_candidate_gives_the_exact_search(cuda):
    index = refine.RefineIndex(_inner("PQ8"), _docs_on())
    s, i = index.search(_queries_on(), 300, 1, k_factor=10)                 # k_base = ND
    es, ei = dense.DenseIndex(_docs_on()).search(_queries_on(), 300)
    torch.cuda.synchronize()
    assert index.last_candidates[0].shape == (NQ, ND) and (index.last_candidates[1] == ND).all()
    assert torch.equal(i, ei) and torch.equal(s.view(torch.int32), es.view(torch.int32))


def test_what_refine_buys(cuda):
    d, q, _, _, _, (es, ei) = _corpus()
    assert (es[:, K - 1] > es[:, K]).all()                                   # no tie at rank K: the exact top-K is a set
    exact = [set(row[:K].tolist()) for row in ei]
    rose = []
    for name in FAMILIES:
        inner = _inner(name)
        index = refine.RefineIndex(inner, _docs_on())
        for k_factor in (1, 4):
            _, i = index.search(_queries_on(), K, 2, k_factor=k_factor)
            _, own = inner.search(_queries_on(), K, 2)
            torch.cuda.synchronize()
            cand = index.last_candidates[0].cpu().numpy()
            i, own = i.cpu().numpy(), own.cpu().numpy()
            hits = np.zeros((3, NQ), np.int64)
            for b in range(NQ):
                hits[:, b] = [len(set(i[b].tolist()) & exact[b]), len(set(cand[b].tolist()) & exact[b]), len(set(own[b].tolist()) & exact[b])]
                assert hits[0, b] == hits[1, b] >= hits[2, b], (name, k_factor, b, hits[:, b])
            print(f"{name} k_factor {k_factor}: recall@{K} refined {hits[0].mean() / K:.3f}, inner {hits[2].mean() / K:.3f}")
            if "PQ" in name and hits[0].sum() > hits[2].sum():
                rose.append((name, k_factor))
    assert rose, "refine raised the recall of no PQ configuration"


# ---- routing ----------------------------------------------------------------------------------------------------------------
def test_dense_search_routes_the_suffixed_strings(cuda, monkeypatch, capfd):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    rng = np.random.default_rng(47)                     # no clusters: one probed list of seven cannot hold a query's exact top-10
    d, q = rng.standard_normal((ND, DIM)).astype(np.float32), rng.standard_normal((NQ, DIM)).astype(np.float32)
    dt, qt = torch.from_numpy(d).cuda(), torch.from_numpy(q).cuda()
    exact = dense.search(q, d, DIM, K, "Flat")
    for k_factor in (None, "4"):
        if k_factor:
            monkeypatch.setenv("MEVI_REFINE_K_FACTOR", k_factor)
        index = refine.RefineIndex(ivfpq.IVFPQIndex(dt, NLIST, M, 8), dt)                         # the seeds dense.search uses
        ws, wi = index.search(qt, K, 1)
        adc = index.inner.search(qt, K, 1)[0].cpu().numpy()                                       # the bare index's scores
        for param in ("IVF7,PQ8,RFlat", "IVF7,PQ8,Refine(Flat)"):
            capfd.readouterr()
            s, i = dense.search(q, d, DIM, K, param)
            out = capfd.readouterr()
            assert f"Param {param} trained: False." in out.out
            np.testing.assert_array_equal(i, wi.cpu().numpy())
            np.testing.assert_array_equal(_bits(s), _bits(ws.cpu().numpy()))
            assert not np.array_equal(i, exact[1]) and not np.array_equal(_bits(s), _bits(adc))      # neither exact nor the bare index
            line = [l for l in out.err.splitlines() if "recall vs exact search" in l]
            assert len(line) == 1 and "IVF7,PQ8,RFlat nprobe=1" in line[0], out.err
            assert "refined @1 " in line[0] and "inner first 10 @1 " in line[0] and line[0].count("@10 ") == 2
            f = 4 if k_factor else 1
            assert f"k_factor {f}, k_base {K * f}, valid candidates per query: mean {K * f}.0" in line[0], line[0]
    monkeypatch.delenv("MEVI_REFINE_K_FACTOR")
    # what keeps the exact search
    for param, env in (("IVF7,PQ8,RFlat", ("MEVI_REFINE", "exact")), ("IVF7,PQ8,RFlat", ("MEVI_REFINE_K_FACTOR", "410")),
                       ("HNSW32,RFlat", None), ("PQ8,Refine(SQ8)", None)):
        if env:
            monkeypatch.setenv(*env)
        capfd.readouterr()
        a = dense.search(q, d, DIM, K, param)
        assert "recall vs exact" not in capfd.readouterr().err, param
        assert np.array_equal(a[1], exact[1]) and np.array_equal(_bits(a[0]), _bits(exact[0])), param
        if env:
            monkeypatch.delenv(env[0])


def test_dense_profile_returns_its_keys(cuda, monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MEVI_OPQ_NITER", "2")
    monkeypatch.setenv("MEVI_REFINE_K_FACTOR", "2")
    d, q = np.array(_corpus()[0]), np.array(_corpus()[1])
    for param in ("IVF7,PQ8,RFlat", "SQ8,Refine(Flat)", "OPQ8,PQ8x4fs,RFlat"):
        times = dense.profile(q, d, DIM, K, param, bs=[1, 4])
        assert set(times) == {"train", "add", "search_bs1", "search_bs4"}
        assert all(np.isfinite(v) and v > 0 for v in times.values()), times


def test_cli_writes_the_refined_list(cuda, tmp_path):
    nq, k = 5, 10
    d, q = np.array(_corpus()[0]), np.array(_corpus()[1][:nq])
    q.tofile(tmp_path / "q.bin")
    d.tofile(tmp_path / "d.bin")
    with open(tmp_path / "raw.tsv", "w") as f:
        for i in range(nq):
            f.write(f"q{i}\t{i}\n")
    env = {k_: v for k_, v in os.environ.items() if k_ not in ENV}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "faiss_search.py"), "--query_path", str(tmp_path / "q.bin"), "--doc_path",
                        str(tmp_path / "d.bin"), "--output_path", str(tmp_path / "out.tsv"), "--raw_query_path", str(tmp_path / "raw.tsv"),
                        "--dim", str(DIM), "--topk", str(k), "--param", "PQ8,RFlat"], capture_output=True, text=True,
                       env=dict(env, PYTHONPATH=ROOT, MEVI_REFINE_K_FACTOR="3"))
    assert r.returncode == 0, r.stderr[-1500:]
    assert "Param PQ8,RFlat trained: False." in r.stdout and f"int64 ({nq}, {k}) float32 ({nq}, {k})" in r.stdout
    line = [l for l in r.stderr.splitlines() if "recall vs exact search" in l]
    assert len(line) == 1 and "PQ8,RFlat nprobe=1" in line[0] and "refined @1 " in line[0] and "inner first 10 @1 " in line[0]
    assert "k_factor 3, k_base 30" in line[0]
    index = refine.RefineIndex(ivfpq.IVFPQIndex(_docs_on(), None, M, 8), _docs_on())
    _, want = index.search(_queries_on()[:nq], k, 1, k_factor=3)
    rows = [l.rstrip("\n").split("\t") for l in open(tmp_path / "out.tsv")]
    assert len(rows) == nq and [[int(x) for x in r_[2].split(",")] for r_ in rows] == want.cpu().numpy().tolist()
