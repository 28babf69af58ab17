"""The IVF-PQ index (mevi_amd/ivfpq.py) given its centroids and codebook against the oracle: lists, codes, search, graph replay,
the flat PQ form, a trained index against its own tables, and `faiss_search.py --param IVF8,PQ4` through its command line.
Bar: bit equality (tests/ivfpq_cases.py: adc_expected)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ivfpq_cases as pc
from mevi_amd import ivfpq
from oracle import dense as odense
from oracle import rq as orq

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want):
    s, i = got
    torch.cuda.synchronize()
    np.testing.assert_array_equal(i.cpu().numpy(), want[1])
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), want[0].view(np.uint32))


def _corpus(seed, nd, nq, dim, nlist):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((nlist, dim)).astype(np.float32) * 2
    d = (centres[rng.integers(0, nlist, size=nd)] + rng.standard_normal((nd, dim))).astype(np.float32)
    q = (centres[rng.integers(0, nlist, size=nq)] + rng.standard_normal((nq, dim))).astype(np.float32)
    return d, q, centres


def _expected_index(d, cent, book):
    """(list_of, order, offsets, codes list-major) from the oracle: best centroid by ip_topk_exact, one rq_encode level per column
    slice of the f32 residuals."""
    m, _, dsub = book.shape
    if cent is None:
        list_of, res, nlist = np.zeros(len(d), np.int64), d, 1
    else:
        list_of = odense.ip_topk_exact(d, cent, 1)[1][:, 0]
        res, nlist = d - cent[list_of], len(cent)
        assert res.dtype == np.float32
    codes = np.stack([orq.rq_encode(res[:, j * dsub:(j + 1) * dsub], book[j][None])[:, 0] for j in range(m)], 1)
    order = np.argsort(list_of, kind="stable")
    off = np.zeros(nlist + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(list_of, minlength=nlist))
    return list_of, order.astype(np.int64), off, codes[order].astype(np.uint8)


def _check_index(cuda, d, q, cent, book, k, nprobe):
    nlist = None if cent is None else len(cent)
    m, K, _ = book.shape
    index = ivfpq.IVFPQIndex(torch.from_numpy(d).to(cuda), nlist, m, int(np.log2(K)), centroids=None if cent is None else torch.from_numpy(cent),
                             codebook=torch.from_numpy(book))
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
    want = pc.adc_expected(q, book, codes, off, ids, probe, bias, k)
    _same(index.search(torch.from_numpy(q).to(cuda), k, nprobe), want)
    return index, want


@pytest.mark.parametrize("dim,m,K,nlist,nprobe,k", [
    (32, 8, 16, 6, 2, 50),
    (64, 16, 256, 5, 5, 1000),          # every list
    (160, 40, 16, 7, 3, 100),           # m > 32: the encode call runs on two groups of column slices
])
def test_index_from_given_centroids_and_codebook(cuda, dim, m, K, nlist, nprobe, k):
    d, q, centres = _corpus(dim + m, 2500, 20, dim, nlist)
    rng = np.random.default_rng(dim)
    book = (rng.standard_normal((m, K, dim // m)) * 0.7).astype(np.float32)
    _check_index(cuda, d, q, centres, book, k, nprobe)


def test_flat_pq_index(cuda):
    """'PQ<m>': no coarse quantiser, the residual is the row, one list, ids = rows."""
    d, q, _ = _corpus(3, 2 * 1024 + 300, 9, 32, 4)
    book = np.random.default_rng(4).standard_normal((8, 64, 4)).astype(np.float32)
    index, _ = _check_index(cuda, d, q, None, book, 100, 1)
    assert index.centroids is None and index.offsets.tolist() == [0, len(d)] and index.clamp_nprobe(7) == 1


def test_planted_lists_and_codes_come_back(cuda):
    """Centroid l = 10 e_l; a row = its centroid + the concatenation of one codebook entry per subspace, entries being distinct
    multiples of 2^-10 in [-1, 1): 10 + c and (10 + c) - 10 are exact in f32, so the residual IS the entries, the planted code is at
    distance 0 and every other at more, and <row, 10 e_l> >= 90 beats every other centroid's <= 10."""
    rng = np.random.default_rng(8)
    nlist, m, K, dsub, nd = 6, 8, 32, 4, 1500
    dim = m * dsub
    cent = np.zeros((nlist, dim), np.float32)
    cent[np.arange(nlist), np.arange(nlist)] = 10.0
    book = (rng.integers(-1024, 1024, size=(m, K, dsub)) / 1024.0).astype(np.float32)
    assert all(len({tuple(e) for e in book[j].tolist()}) == K for j in range(m))
    planted_list = rng.integers(0, nlist, size=nd)
    planted_list[:3] = 0, nlist - 1, 2
    planted = rng.integers(0, K, size=(nd, m))
    d = (cent[planted_list] + np.concatenate([book[j][planted[:, j]] for j in range(m)], 1)).astype(np.float32)
    q = rng.standard_normal((6, dim)).astype(np.float32)
    index, _ = _check_index(cuda, d, q, cent, book, 20, 2)
    assert np.array_equal(index.list_of.cpu().numpy(), planted_list)
    order = np.argsort(planted_list, kind="stable")
    assert np.array_equal(index.codes.cpu().numpy(), planted[order].astype(np.uint8))


@pytest.mark.parametrize("nq", [1, 32])
def test_graph_replay_equals_eager(cuda, nq):
    d, _, centres = _corpus(17, 3000, 1, 64, 8)
    book = np.random.default_rng(18).standard_normal((16, 256, 4)).astype(np.float32)
    index = ivfpq.IVFPQIndex(torch.from_numpy(d).to(cuda), 8, 16, 8, centroids=torch.from_numpy(centres), codebook=torch.from_numpy(book))
    graph = index.search_graph(nq, 10, 2)
    seen = []
    for r in range(3):
        q = torch.from_numpy(_corpus(100 + r, 1, nq, 64, 8)[1]).to(cuda)
        a = graph.run(q)
        b = index.search(q, 10, 2)
        torch.cuda.synchronize()
        assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        seen.append(a[1].cpu().numpy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    with pytest.raises(ValueError):
        index.search_graph(ivfpq.GRAPH_MAX_QUERIES + 1, 10, 2)
    flat = ivfpq.IVFPQIndex(torch.from_numpy(d).to(cuda), None, 16, 8, codebook=torch.from_numpy(book))
    q = torch.from_numpy(_corpus(200, 1, nq, 64, 8)[1]).to(cuda)
    a, b = flat.search_graph(nq, 10).run(q), flat.search(q, 10)
    torch.cuda.synchronize()
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def test_trained_index_searches_by_its_own_tables(cuda):
    """train + add + search with nothing given ('IVF6,PQ4x5' and 'PQ4x5'): whatever k-means found, lists, codes and results are the
    oracle's for the index's own centroids and codebook; the same seed builds the same index."""
    d, q, _ = _corpus(23, 1200, 12, 16, 6)
    dt, qt = torch.from_numpy(d).to(cuda), torch.from_numpy(q).to(cuda)
    for nlist in (6, None):
        index = ivfpq.IVFPQIndex(dt, nlist, 4, 5)
        cent = None if nlist is None else index.centroids.cpu().numpy()
        book = index.codebook.cpu().numpy()
        assert book.shape == (4, 32, 4) and np.isfinite(book).all()
        _, order, off, codes = _expected_index(d, cent, book)
        assert np.array_equal(index.codes.cpu().numpy(), codes) and np.array_equal(index.ids.cpu().numpy(), order)
        if nlist is None:
            want = pc.adc_expected(q, book, codes, off, None, np.zeros((12, 1), np.int32), None, 30)
        else:
            bias, probe = odense.ip_topk_exact(q, cent, 2)
            want = pc.adc_expected(q, book, codes, off, order, probe, bias, 30)
        _same(index.search(qt, 30, 2), want)
        again = ivfpq.IVFPQIndex(dt, nlist, 4, 5)
        assert torch.equal(again.codebook, index.codebook) and torch.equal(again.codes, index.codes)


def test_cli_serves_the_factory_string_and_exact_restores_flat(cuda, tmp_path):
    """`faiss_search.py --param IVF8,PQ4 --dim 16` on tiny files: the reference's stdout lines, the recall line on stderr; with
    MEVI_IVFPQ=exact the output file is the `--param Flat` file byte for byte."""
    nq, nd, dim, k = 5, 700, 16, 10
    d, q, _ = _corpus(29, nd, nq, dim, 8)
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

    r = run("IVF8,PQ4", "pq.tsv")
    assert "Param IVF8,PQ4 trained: False." in r.stdout and f"int64 ({nq}, {k}) float32 ({nq}, {k})" in r.stdout
    line = [l for l in r.stderr.splitlines() if "recall vs exact search" in l]
    assert len(line) == 1 and "IVF8,PQ4 nprobe=1" in line[0] and "@1 " in line[0] and "@10 " in line[0] and f"{nd * 4} bytes of codes" in line[0]
    rows = [l.rstrip("\n").split("\t") for l in open(tmp_path / "pq.tsv")]
    assert len(rows) == nq and all(len(r_[2].split(",")) == k for r_ in rows)
    exact = run("IVF8,PQ4", "exact.tsv", MEVI_IVFPQ="exact")
    assert "Param IVF8,PQ4 trained: False." in exact.stdout and "recall vs exact search" not in exact.stderr
    run("Flat", "flat.tsv")
    assert open(tmp_path / "exact.tsv", "rb").read() == open(tmp_path / "flat.tsv", "rb").read()
    assert open(tmp_path / "pq.tsv", "rb").read() != open(tmp_path / "flat.tsv", "rb").read()
