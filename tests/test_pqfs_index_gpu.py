"""The 4-bit fast-scan PQ index (mevi_amd/pqfs.py) given its centroids and codebook: lists and packed codes against
ivfpq.IVFPQIndex(nbits=4), search against the oracle-built reference (tests/ivfpq_cases.py: adc_expected over the unpacked codes)
and against IVFPQIndex.search bit for bit, graph replay, a self-trained index against its own tables, the routing of
dense.search / dense.profile and `faiss_search.py --param IVF8,PQ8x4fs` through its command line."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ivfpq_cases as pc
import pqfs_cases as fc
from mevi_amd import dense, ivfpq, pqfs
from oracle import dense as odense

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND, NQ, DIM, M, NLIST = 4096, 20, 32, 8, 8


def _same(got, want):
    s, i = got
    torch.cuda.synchronize()
    np.testing.assert_array_equal(i.cpu().numpy(), want[1])
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), want[0].view(np.uint32))


@functools.lru_cache(maxsize=None)
def _corpus():
    """(docs, queries, centroids, codebook): clustered rows; shared, so nobody writes to them."""
    rng = np.random.default_rng(71)
    centres = rng.standard_normal((NLIST, DIM)).astype(np.float32) * 2
    d = (centres[rng.integers(0, NLIST, size=ND)] + rng.standard_normal((ND, DIM))).astype(np.float32)
    q = (centres[rng.integers(0, NLIST, size=NQ)] + rng.standard_normal((NQ, DIM))).astype(np.float32)
    book = (rng.standard_normal((M, 16, DIM // M)) * 0.7).astype(np.float32)
    return d, q, centres, book


def _pair(cuda, nlist):
    """(PQFSIndex, IVFPQIndex at 4 bits) over the shared corpus with the given centroids and codebook."""
    d, _, centres, book = _corpus()
    cent = None if nlist is None else torch.from_numpy(np.array(centres))
    dt = torch.from_numpy(np.array(d)).to(cuda)
    return (pqfs.PQFSIndex(dt, nlist, M, centroids=cent, codebook=torch.from_numpy(np.array(book))),
            ivfpq.IVFPQIndex(dt, nlist, M, 4, centroids=cent, codebook=torch.from_numpy(np.array(book))))


@pytest.mark.parametrize("nlist", [NLIST, None])
def test_lists_and_packed_codes_are_those_of_the_byte_index(cuda, nlist):
    fs, pq = _pair(cuda, nlist)
    assert torch.equal(fs.list_of, pq.list_of) and torch.equal(fs.offsets, pq.offsets) and torch.equal(fs.offsets_dev, pq.offsets_dev)
    assert torch.equal(fs.ids, pq.ids) and fs.max_list_len == pq.max_list_len and torch.equal(fs.codebook, pq.codebook)
    assert fs.codes.dtype == torch.uint8 and fs.codes.shape == (ND, M // 2)
    byte_codes = pq.codes.cpu().numpy()
    assert byte_codes.max() < 16 and len(np.unique(byte_codes)) == 16
    np.testing.assert_array_equal(fs.codes.cpu().numpy(), fc.pack(byte_codes))
    if nlist is None:
        assert fs.centroids is None and fs.offsets.tolist() == [0, ND] and fs.clamp_nprobe(7) == 1


@pytest.mark.parametrize("nlist", [NLIST, None])
def test_search_equals_adc_expected_and_the_byte_index(cuda, nlist):
    d, q, centres, book = _corpus()
    fs, pq = _pair(cuda, nlist)
    qt = torch.from_numpy(np.array(q)).to(cuda)
    codes = fc.unpack(fs.codes.cpu().numpy())
    off = fs.offsets.numpy()
    for nprobe in ((1, 3, 8) if nlist else (1,)):
        if nlist is None:
            probe, bias, ids = np.zeros((NQ, 1), np.int32), None, None
        else:
            bias, probe = odense.ip_topk_exact(q, centres, nprobe)      # the oracle's coarse scores are the biases
            ids = fs.ids.cpu().numpy()
        want = pc.adc_expected(q, book, codes, off, ids, probe, bias, 100)
        got = fs.search(qt, 100, nprobe)
        _same(got, want)
        other = pq.search(qt, 100, nprobe)
        torch.cuda.synchronize()
        assert torch.equal(got[1], other[1]) and torch.equal(got[0].view(torch.int32), other[0].view(torch.int32))


@pytest.mark.parametrize("nq", [1, 32])
def test_graph_replay_equals_eager(cuda, nq):
    fs, _ = _pair(cuda, NLIST)
    graph = fs.search_graph(nq, 10, 2)
    seen = []
    for r in range(3):
        q = torch.from_numpy(np.random.default_rng(100 + r).standard_normal((nq, DIM)).astype(np.float32)).to(cuda)
        a = graph.run(q)
        b = fs.search(q, 10, 2)
        torch.cuda.synchronize()
        assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        seen.append(a[1].cpu().numpy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    with pytest.raises(ValueError):
        fs.search_graph(pqfs.GRAPH_MAX_QUERIES + 1, 10, 2)
    flat, _ = _pair(cuda, None)
    q = torch.from_numpy(np.random.default_rng(200).standard_normal((nq, DIM)).astype(np.float32)).to(cuda)
    a, b = flat.search_graph(nq, 10).run(q), flat.search(q, 10)
    torch.cuda.synchronize()
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def test_trained_index_searches_by_its_own_tables(cuda):
    """train + add + search with nothing given: whatever k-means found, the packed codes are those of the byte index built from the
    index's own centroids and codebook, the results the reference's for them; the same seed builds the same index."""
    d, q, _, _ = _corpus()
    dt, qt = torch.from_numpy(np.array(d)).to(cuda), torch.from_numpy(np.array(q)).to(cuda)
    for nlist in (NLIST, None):
        index = pqfs.PQFSIndex(dt, nlist, M)
        book = index.codebook.cpu().numpy()
        assert book.shape == (M, 16, DIM // M) and np.isfinite(book).all()
        ref = ivfpq.IVFPQIndex(dt, nlist, M, 4, centroids=index.centroids, codebook=index.codebook)
        np.testing.assert_array_equal(index.codes.cpu().numpy(), fc.pack(ref.codes.cpu().numpy()))
        assert torch.equal(index.ids, ref.ids)
        codes, off = fc.unpack(index.codes.cpu().numpy()), index.offsets.numpy()
        if nlist is None:
            want = pc.adc_expected(q, book, codes, off, None, np.zeros((NQ, 1), np.int32), None, 30)
        else:
            bias, probe = odense.ip_topk_exact(q, index.centroids.cpu().numpy(), 2)
            want = pc.adc_expected(q, book, codes, off, index.ids.cpu().numpy(), probe, bias, 30)
        _same(index.search(qt, 30, 2), want)
        again = pqfs.PQFSIndex(dt, nlist, M)
        assert torch.equal(again.codebook, index.codebook) and torch.equal(again.codes, index.codes)


def test_dense_search_routes_the_strings_to_the_index(cuda, monkeypatch, capfd):
    d, q, _, _ = _corpus()
    monkeypatch.delenv("MEVI_PQFS", raising=False)
    monkeypatch.setenv("MEVI_IVF_NPROBE", "2")
    dt, qt = torch.from_numpy(np.array(d)).to(cuda), torch.from_numpy(np.array(q)).to(cuda)
    exact = dense.search(q, d, DIM, 10, "Flat")
    for param, nlist in (("IVF8,PQ8x4fs", 8), ("PQ8x4fs", None)):
        want = pqfs.PQFSIndex(dt, nlist, M).search(qt, 10, 2)
        capfd.readouterr()
        s, i = dense.search(q, d, DIM, 10, param)
        err = capfd.readouterr().err
        np.testing.assert_array_equal(i, want[1].cpu().numpy())
        np.testing.assert_array_equal(s.view(np.uint32), want[0].cpu().numpy().view(np.uint32))
        assert not np.array_equal(i, exact[1])                          # 4 bytes a row: approximate
        assert f"{param} nprobe={2 if nlist else 1}: recall vs exact search" in err and f"{ND * M // 2} bytes of packed codes" in err
        monkeypatch.setenv("MEVI_PQFS", "exact")
        s, i = dense.search(q, d, DIM, 10, param)
        assert np.array_equal(i, exact[1]) and np.array_equal(s.view(np.uint32), exact[0].view(np.uint32))
        monkeypatch.delenv("MEVI_PQFS")
    # m % 8 != 0 is outside the envelope: the exact search's lists, as before (48 = 12 * 4 columns)
    rng = np.random.default_rng(5)
    d48, q48 = rng.standard_normal((500, 48)).astype(np.float32), rng.standard_normal((4, 48)).astype(np.float32)
    a, b = dense.search(q48, d48, 48, 10, "PQ12x4fs"), dense.search(q48, d48, 48, 10, "Flat")
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def test_dense_profile_returns_its_keys(cuda, monkeypatch):
    d, q, _, _ = _corpus()
    monkeypatch.delenv("MEVI_PQFS", raising=False)
    for param in ("IVF8,PQ8x4fs", "PQ8x4fs"):
        times = dense.profile(q, d, DIM, 10, param, bs=[1, 4])
        assert set(times) == {"train", "add", "search_bs1", "search_bs4"}
        assert all(np.isfinite(v) and v > 0 for v in times.values()), times


def test_cli_serves_the_factory_string_and_exact_restores_flat(cuda, tmp_path):
    """`faiss_search.py --param IVF8,PQ8x4fs --dim 32` on tiny files: the reference's stdout lines, the recall line on stderr with the
    packed byte count nd * m / 2; with MEVI_PQFS=exact the output file is the `--param Flat` file byte for byte."""
    nq, nd, k = 5, 700, 10
    d, q, _, _ = _corpus()
    np.array(q[:nq]).tofile(tmp_path / "q.bin")
    np.array(d[:nd]).tofile(tmp_path / "d.bin")
    with open(tmp_path / "raw.tsv", "w") as f:
        for i in range(nq):
            f.write(f"q{i}\t{i}\n")

    def run(param, out, **env):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "faiss_search.py"), "--query_path", str(tmp_path / "q.bin"), "--doc_path",
                            str(tmp_path / "d.bin"), "--output_path", str(tmp_path / out), "--raw_query_path", str(tmp_path / "raw.tsv"),
                            "--dim", str(DIM), "--topk", str(k), "--param", param], capture_output=True, text=True,
                           env=dict(os.environ, PYTHONPATH=ROOT, **env))
        assert r.returncode == 0, r.stderr[-1500:]
        return r

    r = run("IVF8,PQ8x4fs", "fs.tsv")
    assert "Param IVF8,PQ8x4fs trained: False." in r.stdout and f"int64 ({nq}, {k}) float32 ({nq}, {k})" in r.stdout
    line = [l for l in r.stderr.splitlines() if "recall vs exact search" in l]
    assert len(line) == 1 and "IVF8,PQ8x4fs nprobe=1" in line[0] and "@1 " in line[0] and "@10 " in line[0]
    assert f"{nd * M // 2} bytes of packed codes" in line[0]
    rows = [l.rstrip("\n").split("\t") for l in open(tmp_path / "fs.tsv")]
    assert len(rows) == nq and all(len(r_[2].split(",")) == k for r_ in rows)
    exact = run("IVF8,PQ8x4fs", "exact.tsv", MEVI_PQFS="exact")
    assert "Param IVF8,PQ8x4fs trained: False." in exact.stdout and "recall vs exact search" not in exact.stderr
    run("Flat", "flat.tsv")
    assert open(tmp_path / "exact.tsv", "rb").read() == open(tmp_path / "flat.tsv", "rb").read()
    assert open(tmp_path / "fs.tsv", "rb").read() != open(tmp_path / "flat.tsv", "rb").read()
