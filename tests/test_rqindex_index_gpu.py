"""The residual-quantiser index (mevi_amd/rqindex.py) given its centroids and codebook against the oracle: lists, codes, search, graph
replay, the case in which the index is exact, the refine stage behind it, what keeps the exact search, a trained index against its own
tables, and `faiss_search.py --param IVF7,RQ8x8` through its command line.  Bar: bit equality (tests/aq_cases.py: aq_expected)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import aq_cases as ac
import refine_cases as rc
from mevi_amd import dense, refine, rqindex
from oracle import dense as odense
from oracle import rq as orq

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND, NQ, DIM, NLIST = 4096, 12, 32, 7
ENV = ("MEVI_RQINDEX", "MEVI_REFINE", "MEVI_REFINE_K_FACTOR", "MEVI_IVF_NPROBE")


def _bits(a):
    return a.view(np.uint32)


def _same(got, want):
    s, i = got
    torch.cuda.synchronize()
    np.testing.assert_array_equal(i.cpu().numpy(), want[1])
    np.testing.assert_array_equal(_bits(s.cpu().numpy()), _bits(want[0]))


@functools.lru_cache(maxsize=None)
def _corpus():
    """(docs 4096 x 32, queries, centroids): clustered rows; shared, so nobody writes to them."""
    rng = np.random.default_rng(43)
    centres = rng.standard_normal((NLIST, DIM)).astype(np.float32) * 2
    d = (centres[rng.integers(0, NLIST, size=ND)] + rng.standard_normal((ND, DIM))).astype(np.float32)
    q = (centres[rng.integers(0, NLIST, size=NQ)] + rng.standard_normal((NQ, DIM))).astype(np.float32)
    for a in (d, q, centres):
        a.setflags(write=False)
    return d, q, centres


@functools.lru_cache(maxsize=None)
def _book(M, nbits):
    """A random codebook whose levels shrink as a trained one's do; level 2 has a duplicate centroid."""
    rng = np.random.default_rng(100 * M + nbits)
    book = (rng.standard_normal((M, 1 << nbits, DIM)) * (0.8 ** np.arange(M))[:, None, None]).astype(np.float32)
    book[2, -1] = book[2, 0]
    book.setflags(write=False)
    return book


def _expected_index(d, cent, book):
    """(list_of, order, offsets, codes list-major) from the oracle: best centroid by ip_topk_exact, oracle.rq.rq_encode of the f32
    residuals over ALL levels at once."""
    if cent is None:
        list_of, res, nlist = np.zeros(len(d), np.int64), d, 1
    else:
        list_of = odense.ip_topk_exact(d, cent, 1)[1][:, 0]
        res, nlist = d - cent[list_of], len(cent)
        assert res.dtype == np.float32
    codes = orq.rq_encode(res, book)
    order = np.argsort(list_of, kind="stable")
    off = np.zeros(nlist + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(list_of, minlength=nlist))
    return list_of, order.astype(np.int64), off, codes[order].astype(np.uint8)


def _build(cuda, d, cent, book):
    M, K, _ = book.shape
    return rqindex.RQIndex(torch.from_numpy(np.array(d)).to(cuda), None if cent is None else len(cent), M, int(np.log2(K)),
                           centroids=None if cent is None else torch.from_numpy(np.array(cent)), codebook=torch.from_numpy(np.array(book)))


def _check_index(cuda, d, q, cent, book, k, nprobe):
    index = _build(cuda, d, cent, book)
    list_of, order, off, codes = _expected_index(d, cent, book)
    assert np.array_equal(index.list_of.cpu().numpy(), list_of)
    assert np.array_equal(index.offsets.numpy(), off) and np.array_equal(index.offsets_dev.cpu().numpy(), off)
    assert np.array_equal(index.ids.cpu().numpy(), order) and index.max_list_len == int(np.diff(off).max())
    got_codes = index.codes.cpu().numpy()
    assert got_codes.dtype == np.uint8 and np.array_equal(got_codes, codes)
    if cent is None:
        probe, bias, ids = np.zeros((len(q), 1), np.int32), None, None
    else:
        bias, probe = odense.ip_topk_exact(q, cent, nprobe)             # the oracle's coarse scores are the biases
        ids = order
    want = ac.aq_expected(q, book, codes, off, ids, probe, bias, k)
    _same(index.search(torch.from_numpy(np.array(q)).to(cuda), k, nprobe), want)
    return index, want


@pytest.mark.parametrize("name,k,nprobe", [("RQ8x8", 100, 1), ("IVF7,RQ8x8", 50, 2), ("IVF7,RQ8x8", 1000, 7), ("RQ12x4", 10, 1)])
def test_index_from_given_centroids_and_codebook(cuda, name, k, nprobe):
    """'RQ12x4': 12 levels are a group of 8 and a group of 4 with one residual call between them."""
    nlist, M, nbits = rqindex.parse_factory(name)
    d, q, centres = _corpus()
    index, _ = _check_index(cuda, d, q, None if nlist is None else centres, _book(M, nbits), k, nprobe)
    assert index.clamp_nprobe(100) == (1 if nlist is None else NLIST) and index.train_stats == {}


def test_an_index_whose_first_level_is_the_rows_gives_the_exact_search(cuda):
    """nd = K = 256 distinct rows, level 0 = the rows, the other levels zero: codes (row, 0, ...), scores the exact search's chain."""
    d, q, _ = _corpus()
    rows = np.array(d[:256])
    book = np.zeros((8, 256, DIM), np.float32)
    book[0] = rows
    index = _build(cuda, rows, None, book)
    codes = index.codes.cpu().numpy()
    assert np.array_equal(codes[:, 0], np.arange(256)) and (codes[:, 1:] == 0).all()
    qt = torch.from_numpy(np.array(q)).to(cuda)
    s, i = index.search(qt, 20)
    es, ei = dense.DenseIndex(torch.from_numpy(rows).to(cuda)).search(qt, 20)
    torch.cuda.synchronize()
    assert torch.equal(i, ei) and torch.equal((s + 0.0).view(torch.int32), (es + 0.0).view(torch.int32))
    want = odense.ip_topk_exact(q, rows, 20)
    np.testing.assert_array_equal(i.cpu().numpy(), want[1])
    np.testing.assert_array_equal(_bits(s.cpu().numpy()), _bits(want[0]))


@pytest.mark.parametrize("nq", [1, 32])
def test_graph_replay_equals_eager(cuda, nq):
    d, _, centres = _corpus()
    rng = np.random.default_rng(nq)
    seen = []
    for cent in (centres, None):
        index = _build(cuda, d, cent, _book(8, 8))
        graph = index.search_graph(nq, 10, 2)
        for r in range(2):
            q = torch.from_numpy(rng.standard_normal((nq, DIM)).astype(np.float32)).to(cuda)
            a = graph.run(q)
            b = index.search(q, 10, 2)
            torch.cuda.synchronize()
            assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
            seen.append(a[1].cpu().numpy())
        with pytest.raises(ValueError):
            index.search_graph(rqindex.GRAPH_MAX_QUERIES + 1, 10, 2)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[2], seen[3])


@pytest.mark.parametrize("k_factor", [1, 4])
def test_refine_behind_the_index_scores_its_candidates_exactly(cuda, k_factor):
    """'RQ8x8,RFlat': every score is a bit of the exact search, the ids the reference's over the inner index's own candidates."""
    d, q, _ = _corpus()
    K = 10
    inner = _build(cuda, d, None, _book(8, 8))
    docs = torch.from_numpy(np.array(d)).to(cuda)
    qt = torch.from_numpy(np.array(q)).to(cuda)
    index = refine.RefineIndex(refine.build_inner(docs, "rqindex", (None, 8, 8), codebook=torch.from_numpy(np.array(_book(8, 8)))), docs)
    assert isinstance(index.inner, rqindex.RQIndex) and torch.equal(index.inner.codes, inner.codes)
    _, cand = inner.search(qt, K * k_factor, 1)
    s, i = index.search(qt, K, 1, k_factor=k_factor)
    torch.cuda.synchronize()
    cand = cand.cpu().numpy()
    want = rc.refine_expected(q, d, cand, K)
    np.testing.assert_array_equal(i.cpu().numpy(), want[1])
    np.testing.assert_array_equal(_bits(s.cpu().numpy()), _bits(want[0]))
    es, ei = odense.ip_topk_exact(q, d, ND)                                   # every exact score, by id
    by_id = np.empty((NQ, ND), np.float32)
    np.put_along_axis(by_id, ei, es, axis=1)
    np.testing.assert_array_equal(_bits(s.cpu().numpy()), _bits(np.take_along_axis(by_id, i.cpu().numpy(), axis=1)))


def test_dense_search_routes_the_strings_and_what_keeps_the_exact_search(cuda, monkeypatch, capfd):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    rng = np.random.default_rng(47)                     # no clusters: a coarse code of 8 bytes cannot hold a query's exact top-10
    d, q = rng.standard_normal((ND, DIM)).astype(np.float32), rng.standard_normal((NQ, DIM)).astype(np.float32)
    dt, qt = torch.from_numpy(d).to(cuda), torch.from_numpy(q).to(cuda)
    exact = dense.search(q, d, DIM, 10, "Flat")
    for param, spec in (("RQ8x8", (None, 8, 8)), ("IVF7,RQ8x8", (7, 8, 8)), ("RQ12x4", (None, 12, 4))):
        index = rqindex.RQIndex(dt, *spec)                                    # the seeds dense.search uses
        ws, wi = index.search(qt, 10, 1)
        capfd.readouterr()
        s, i = dense.search(q, d, DIM, 10, param)
        out = capfd.readouterr()
        assert f"Param {param} trained: False." in out.out
        np.testing.assert_array_equal(i, wi.cpu().numpy())
        np.testing.assert_array_equal(_bits(s), _bits(ws.cpu().numpy()))
        assert not np.array_equal(i, exact[1])
        line = [l for l in out.err.splitlines() if "recall vs exact search" in l]
        assert len(line) == 1 and f"{param} nprobe=1" in line[0] and "@1 " in line[0] and "@10 " in line[0], out.err
        assert f"{ND * spec[1]} bytes of codes" in line[0] and "training error per level" in line[0]
        errs = [float(x) for x in line[0].split("before): ")[1].split()]
        before = float(line[0].split(" rows, ")[1].split(" before")[0])
        assert len(errs) == spec[1] and np.allclose(errs, index.train_stats["level_mse"], rtol=1e-5)      # printed with six digits
        # a level's centroids are the means of its clusters: taking them off cannot raise the mean squared norm
        assert before > errs[0] and all(a >= b for a, b in zip(errs, errs[1:])), errs
        assert index.train_stats["train_rows"] == min(ND, 256 * (1 << spec[2]))
    capfd.readouterr()
    s, i = dense.search(q, d, DIM, 10, "RQ8x8,RFlat")
    out = capfd.readouterr()
    line = [l for l in out.err.splitlines() if "recall vs exact search" in l]
    assert len(line) == 1 and "RQ8x8,RFlat nprobe=1" in line[0] and "refined @1 " in line[0], out.err
    es, ei = odense.ip_topk_exact(q, d, ND)                                   # every exact score, by id
    by_id = np.empty((NQ, ND), np.float32)
    np.put_along_axis(by_id, ei, es, axis=1)
    np.testing.assert_array_equal(_bits(s), _bits(np.take_along_axis(by_id, i, axis=1)))
    # what keeps the exact search
    for param, env, k in (("RQ8x8", ("MEVI_RQINDEX", "exact"), 10), ("RQ8x9", None, 10), ("RQ6x8", None, 10), ("RQ8", None, 10),
                          ("LSQ8x8", None, 10), ("RQ8x8_Nqint8", None, 10), ("OPQ8,RQ8x8", None, 10), ("RQ8x8", None, 5000)):
        if env:
            monkeypatch.setenv(*env)
        if k != 10:                                     # topk = 5000 needs that many rows
            d = np.concatenate([d, rng.standard_normal((6000 - ND, DIM)).astype(np.float32)])
        want = exact if k == 10 else dense.search(q, d, DIM, k, "Flat")
        capfd.readouterr()
        a = dense.search(q, d, DIM, k, param)
        assert "recall vs exact" not in capfd.readouterr().err, param
        assert np.array_equal(a[1], want[1]) and np.array_equal(_bits(a[0]), _bits(want[0])), param
        if env:
            monkeypatch.delenv(env[0])


def test_trained_index_searches_by_its_own_tables_and_profile_returns_its_keys(cuda, monkeypatch):
    """train + add + search with nothing given ('IVF7,RQ12x5' and 'RQ12x5'): whatever k-means found, lists, codes and results are the
    oracle's for the index's own centroids and codebook; the same seed builds the same index; dense.profile serves the strings."""
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    d, q, _ = _corpus()
    dt, qt = torch.from_numpy(np.array(d)).to(cuda), torch.from_numpy(np.array(q)).to(cuda)
    for nlist in (7, None):
        index = rqindex.RQIndex(dt, nlist, 12, 5)
        cent = None if nlist is None else index.centroids.cpu().numpy()
        book = index.codebook.cpu().numpy()
        assert book.shape == (12, 32, DIM) and np.isfinite(book).all()
        _, order, off, codes = _expected_index(d, cent, book)
        assert np.array_equal(index.codes.cpu().numpy(), codes) and np.array_equal(index.ids.cpu().numpy(), order)
        if nlist is None:
            want = ac.aq_expected(q, book, codes, off, None, np.zeros((NQ, 1), np.int32), None, 30)
        else:
            bias, probe = odense.ip_topk_exact(q, cent, 2)
            want = ac.aq_expected(q, book, codes, off, order, probe, bias, 30)
        _same(index.search(qt, 30, 2), want)
        again = rqindex.RQIndex(dt, nlist, 12, 5)
        assert torch.equal(again.codebook, index.codebook) and torch.equal(again.codes, index.codes)
        st = index.train_stats
        assert st["train_rows"] == ND and len(st["level_mse"]) == 12 and st["input_mse"] > st["level_mse"][0] > st["level_mse"][-1] > 0
    for param in ("IVF7,RQ8x8", "RQ8x4,RFlat"):
        times = dense.profile(np.array(q), np.array(d), DIM, 10, param, bs=[1, 4])
        assert set(times) == {"train", "add", "search_bs1", "search_bs4"}
        assert all(np.isfinite(v) and v > 0 for v in times.values()), times


def test_cli_serves_the_factory_string_and_exact_restores_flat(cuda, tmp_path):
    """`faiss_search.py --param IVF7,RQ8x8 --dim 32` on tiny files: the reference's stdout lines, the report on stderr, the TSV; with
    MEVI_RQINDEX=exact the output file is the `--param Flat` file byte for byte."""
    nq, k = 5, 10
    d, q, _ = _corpus()
    d, q = np.array(d[:1500]), np.array(q[:nq])
    q.tofile(tmp_path / "q.bin")
    d.tofile(tmp_path / "d.bin")
    with open(tmp_path / "raw.tsv", "w") as f:
        for i in range(nq):
            f.write(f"q{i}\t{i}\n")
    base = {k_: v for k_, v in os.environ.items() if k_ not in ENV}

    def run(param, out, **env):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "faiss_search.py"), "--query_path", str(tmp_path / "q.bin"), "--doc_path",
                            str(tmp_path / "d.bin"), "--output_path", str(tmp_path / out), "--raw_query_path", str(tmp_path / "raw.tsv"),
                            "--dim", str(DIM), "--topk", str(k), "--param", param], capture_output=True, text=True,
                           env=dict(base, PYTHONPATH=ROOT, **env))
        assert r.returncode == 0, r.stderr[-1500:]
        return r

    r = run("IVF7,RQ8x8", "rq.tsv")
    assert "Param IVF7,RQ8x8 trained: False." in r.stdout and f"int64 ({nq}, {k}) float32 ({nq}, {k})" in r.stdout
    line = [l for l in r.stderr.splitlines() if "recall vs exact search" in l]
    assert len(line) == 1 and "IVF7,RQ8x8 nprobe=1" in line[0] and "@1 " in line[0] and "@10 " in line[0]
    assert f"{1500 * 8} bytes of codes" in line[0] and "training error per level" in line[0]
    rows = [l.rstrip("\n").split("\t") for l in open(tmp_path / "rq.tsv")]
    assert len(rows) == nq and all(len(r_[2].split(",")) == k for r_ in rows)
    index = rqindex.RQIndex(torch.from_numpy(d).to(cuda), 7, 8, 8)
    _, want = index.search(torch.from_numpy(q).to(cuda), k, 1)
    assert [[int(x) for x in r_[2].split(",")] for r_ in rows] == want.cpu().numpy().tolist()
    exact = run("IVF7,RQ8x8", "exact.tsv", MEVI_RQINDEX="exact")
    assert "Param IVF7,RQ8x8 trained: False." in exact.stdout and "recall vs exact search" not in exact.stderr
    run("Flat", "flat.tsv")
    assert open(tmp_path / "exact.tsv", "rb").read() == open(tmp_path / "flat.tsv", "rb").read()
    assert open(tmp_path / "rq.tsv", "rb").read() != open(tmp_path / "flat.tsv", "rb").read()
