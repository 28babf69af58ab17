"""The OPQ index (mevi_amd/opq.py): the rotation trainer on the device against the properties its float64 restatement has
(tests/test_opq_cpu.py), and -- given R, centroids and codebook -- codes and search results bit for bit against the oracle-built
references (tests/opq_cases.py: rotate_expected, tests/pq_ref.py: pq_encode, tests/ivfpq_cases.py: adc_expected), the flat index
against an IVFPQIndex over explicitly rotated rows, graph replay, the `steps` build, and the routing of dense.search /
dense.profile / `faiss_search.py --param OPQ8,PQ8x4`."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ivfpq_cases as pc
import opq_cases as oc
import pq_ref
import pqfs_cases as fc
from mevi_amd import dense, ivfpq, opq, ops, rq
from oracle import dense as odense

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND, NQ, DIM, M, NLIST = 3000, 12, 32, 8, 7
TN, TK, TNITER = 4096, 16, 10                           # the trainer's case: rows, centroids, iterations


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- the trainer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["outlier", "decaying"])
def test_trainer_on_the_device(cuda, kind):
    x = oc.GENERATORS[kind](3, TN, DIM)
    xt = torch.from_numpy(x).to(cuda)
    R, errors = opq.train_rotation(xt, M, K=TK, niter=TNITER, seed=5)
    assert R.shape == (DIM, DIM) and R.dtype == torch.float32 and len(errors) == TNITER
    assert opq.LAST_TRAIN["niter"] == TNITER and opq.LAST_TRAIN["device_s"] > 0 and opq.LAST_TRAIN["svd_s"] > 0
    print(f"{kind}: errors {errors[0]:.5g} -> {errors[-1]:.5g}")
    for a, b in zip(errors, errors[1:]):                # f32 rounding of R and of the chains
        assert b <= a * (1 + 1e-4), errors
    Rd = R.double().cpu().numpy()
    assert np.abs(Rd @ Rd.T - np.eye(DIM)).max() <= DIM * 2.0 ** -23
    book, codes = rq.train_pq_codebook(xt, M, TK, seed=5)
    plain = float(((xt.double() - opq.decode(codes, book).double()) ** 2).sum().item()) / TN
    print(f"{kind}: error OPQ {errors[-1]:.5g} / PQ {plain:.5g} = {errors[-1] / plain:.3f}")
    assert errors[-1] <= 0.75 * plain, (errors[-1], plain)
    again, errors2 = opq.train_rotation(xt, M, K=TK, niter=TNITER, seed=5)
    assert _bits_equal(again, R) and errors2 == errors
    other, _ = opq.train_rotation(xt, M, K=TK, niter=2, seed=6)
    assert not _bits_equal(other, R)


# ---- the index given R, centroids and codebook -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _corpus():
    """(docs, queries, centroids, R, {nbits: codebook}, chains of the docs, chains of the queries, rotated centroids): shared, so
    nobody writes to them.  The codebooks are random: the rotated residuals only have to land somewhere."""
    rng = np.random.default_rng(41)
    centres = rng.standard_normal((NLIST, DIM)).astype(np.float32) * 2
    d = (centres[rng.integers(0, NLIST, size=ND)] + rng.standard_normal((ND, DIM))).astype(np.float32)
    q = (centres[rng.integers(0, NLIST, size=NQ)] + rng.standard_normal((NQ, DIM))).astype(np.float32)
    R = opq.random_rotation(DIM, 17).astype(np.float32)
    books = {b: (rng.standard_normal((M, 1 << b, DIM // M)) * 0.8).astype(np.float32) for b in (8, 4)}
    return d, q, centres, R, books, oc.rotate_expected(d, R), oc.rotate_expected(q, R), oc.rotate_expected(centres, R)


@functools.lru_cache(maxsize=None)
def _index(nlist, nbits, fs):
    d, _, centres, R, books, _, _, _ = _corpus()
    cuda = torch.device("cuda:0")
    return opq.OPQIndex(torch.from_numpy(np.array(d)).to(cuda), M, nlist, M, nbits, fs, R=torch.from_numpy(np.array(R)),
                        centroids=None if nlist is None else torch.from_numpy(np.array(centres)),
                        codebook=torch.from_numpy(np.array(books[nbits])))


def _expected_codes(index, nlist, nbits):
    """u8 [ND, M] list-major from the references: pq_encode of rotate_expected over the index's own lists."""
    d, _, _, R, books, chains, _, crot = _corpus()
    if nlist is None:
        y = oc.rotate_expected(d, R)
        assert np.array_equal(y.view(np.uint32), chains.view(np.uint32))
    else:
        ids, list_of = index.ids.cpu().numpy(), index.list_of.cpu().numpy()
        y = oc.rotate_expected(d, R, ids, list_of, crot)
        assert np.array_equal(y.view(np.uint32), (chains[ids] - crot[list_of[ids]]).view(np.uint32))
    return pq_ref.pq_encode(y, books[nbits]).astype(np.uint8)


CONFIGS = [(None, 8, False), (NLIST, 8, False), (None, 4, False), (NLIST, 4, False), (None, 4, True), (NLIST, 4, True)]


@pytest.mark.parametrize("nlist,nbits,fs", CONFIGS)
def test_codes_and_search_equal_the_references(cuda, nlist, nbits, fs):
    d, q, centres, R, books, _, q_rot, crot = _corpus()
    index = _index(nlist, nbits, fs)
    want_codes = _expected_codes(index, nlist, nbits)
    got_codes = index.codes.cpu().numpy()
    np.testing.assert_array_equal(got_codes, fc.pack(want_codes) if fs else want_codes)
    assert len(np.unique(want_codes)) > (1 << nbits) // 2                    # the codes are not degenerate
    if nlist is not None:
        np.testing.assert_array_equal(index.rotation[1].cpu().numpy().view(np.uint32), crot.view(np.uint32))
    qt = torch.from_numpy(np.array(q)).to(cuda)
    off = index.offsets.numpy()
    for nprobe in ((1, 3) if nlist else (1,)):
        if nlist is None:
            probe, bias, ids = np.zeros((NQ, 1), np.int32), None, None
        else:
            bias, probe = odense.ip_topk_exact(q, centres, nprobe)           # the coarse scores of the UNROTATED queries
            ids = index.ids.cpu().numpy()
        for k in (10, 100):
            want = pc.adc_expected(q_rot, books[nbits], want_codes, off, ids, probe, bias, k)
            s, i = index.search(qt, k, nprobe)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(i.cpu().numpy(), want[1])
            np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), want[0].view(np.uint32))


@pytest.mark.parametrize("nbits", [8, 4])
def test_flat_index_is_the_pq_index_over_rotated_rows(cuda, nbits):
    d, q, _, R, books, _, _, _ = _corpus()
    index = _index(None, nbits, False)
    dt, qt, Rt = (torch.from_numpy(np.array(a)).to(cuda) for a in (d, q, R))
    ref = ivfpq.IVFPQIndex(ops.linear(dt, Rt), None, M, nbits, codebook=torch.from_numpy(np.array(books[nbits])))
    assert torch.equal(ref.codes, index.codes)
    for k in (10, 100):
        a, b = index.search(qt, k), ref.search(ops.linear(qt, Rt), k)
        torch.cuda.synchronize()
        assert torch.equal(a[1], b[1]) and _bits_equal(a[0], b[0])


@pytest.mark.parametrize("nlist,nbits,fs", [(NLIST, 8, False), (None, 4, False), (NLIST, 4, True)])
def test_graph_replay_equals_eager(cuda, nlist, nbits, fs):
    index = _index(nlist, nbits, fs)
    graph = index.search_graph(8, 10, 2)
    seen = []
    for r in range(2):
        q = torch.from_numpy(np.random.default_rng(300 + r).standard_normal((8, DIM)).astype(np.float32)).to(cuda)
        a, b = graph.run(q), index.search(q, 10, 2)
        torch.cuda.synchronize()
        assert torch.equal(a[1], b[1]) and _bits_equal(a[0], b[0])
        seen.append(a[1].cpu().numpy())
    assert not np.array_equal(seen[0], seen[1])
    with pytest.raises(ValueError):
        index.search_graph(opq.GRAPH_MAX_QUERIES + 1, 10, 2)


@pytest.mark.parametrize("nlist,fs", [(NLIST, False), (None, True)])
def test_steps_build_gives_the_same_index(cuda, monkeypatch, nlist, fs):
    """MEVI_OPQ_ROTATE=steps: the composition of existing calls trains the same codebook and writes the same codes."""
    d, _, centres, R, _, _, _, _ = _corpus()
    dt = torch.from_numpy(np.array(d)).to(cuda)
    built = {}
    for mode in ("fused", "steps"):
        monkeypatch.setenv("MEVI_OPQ_ROTATE", mode)
        built[mode] = opq.OPQIndex(dt, M, nlist, M, 4, fs, R=torch.from_numpy(np.array(R)),
                                   centroids=None if nlist is None else torch.from_numpy(np.array(centres)))
    a, b = built["fused"], built["steps"]
    assert _bits_equal(a.codebook, b.codebook) and torch.equal(a.codes, b.codes) and torch.equal(a.ids, b.ids)
    assert a.codes.shape == (ND, M // 2 if fs else M)


# ---- routing ----------------------------------------------------------------------------------------------------------------
def _recall(found, exact):
    return oc.recall_at(found, exact)


def test_dense_search_routes_the_strings_and_gains_recall(cuda, monkeypatch, capfd):
    monkeypatch.delenv("MEVI_OPQ", raising=False)
    monkeypatch.delenv("MEVI_OPQ_NITER", raising=False)
    monkeypatch.delenv("MEVI_OPQ_ROTATE", raising=False)
    d, q = oc.outlier_rows(11, 4096, DIM), oc.outlier_rows(12, 64, DIM)
    exact = dense.search(q, d, DIM, 10, "Flat")
    plain = dense.search(q, d, DIM, 10, "PQ8x4")
    capfd.readouterr()
    s, i = dense.search(q, d, DIM, 10, "OPQ8,PQ8x4")
    out = capfd.readouterr()
    assert "Param OPQ8,PQ8x4 trained: False." in out.out
    line = [l for l in out.err.splitlines() if "recall vs exact search" in l]
    assert len(line) == 1 and "OPQ8,PQ8x4 nprobe=1" in line[0] and "niter 50" in line[0] and "training error" in line[0]
    assert f"{4096 * 8} bytes of codes" in line[0]
    rec_opq, rec_pq = _recall(i, exact[1]), _recall(plain[1], exact[1])
    print(f"recall@10 OPQ8,PQ8x4 {rec_opq:.3f} / PQ8x4 {rec_pq:.3f}")
    assert rec_opq >= rec_pq + 0.2, (rec_opq, rec_pq)
    # what keeps the exact search: MEVI_OPQ=exact, a reducing rotation, dim % M != 0
    monkeypatch.setenv("MEVI_OPQ_NITER", "2")
    for param, env in (("OPQ8,PQ8x4", "exact"), ("OPQ8_16,PQ8", None), ("OPQ5,PQ8", None)):
        if env:
            monkeypatch.setenv("MEVI_OPQ", env)
        a = dense.search(q, d, DIM, 10, param)
        assert np.array_equal(a[1], exact[1]) and np.array_equal(a[0].view(np.uint32), exact[0].view(np.uint32)), param
        monkeypatch.delenv("MEVI_OPQ", raising=False)
    # ... and the IVF and fast-scan forms are served by the index
    monkeypatch.setenv("MEVI_IVF_NPROBE", "2")
    for param in ("OPQ8,IVF8,PQ8", "OPQ8_32,IVF8,PQ8x4fs"):
        capfd.readouterr()
        a = dense.search(q, d, DIM, 10, param)
        err = capfd.readouterr().err
        assert "nprobe=2: recall vs exact search" in err and "niter 2" in err and not np.array_equal(a[1], exact[1]), param


def test_dense_profile_returns_its_keys(cuda, monkeypatch):
    monkeypatch.delenv("MEVI_OPQ", raising=False)
    monkeypatch.setenv("MEVI_OPQ_NITER", "3")
    d, q = oc.outlier_rows(11, 4096, DIM), oc.outlier_rows(12, 64, DIM)
    for param in ("OPQ8,IVF8,PQ8", "OPQ8,PQ8x4fs"):
        times = dense.profile(q, d, DIM, 10, param, bs=[1, 4])
        assert set(times) == {"train", "add", "search_bs1", "search_bs4"}
        assert all(np.isfinite(v) and v > 0 for v in times.values()), times


def test_cli_serves_the_factory_string(cuda, tmp_path):
    nq, nd, k = 5, 700, 10
    d, q = oc.outlier_rows(11, nd, DIM), oc.outlier_rows(12, nq, DIM)
    q.tofile(tmp_path / "q.bin")
    d.tofile(tmp_path / "d.bin")
    with open(tmp_path / "raw.tsv", "w") as f:
        for i in range(nq):
            f.write(f"q{i}\t{i}\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "faiss_search.py"), "--query_path", str(tmp_path / "q.bin"), "--doc_path",
                        str(tmp_path / "d.bin"), "--output_path", str(tmp_path / "out.tsv"), "--raw_query_path", str(tmp_path / "raw.tsv"),
                        "--dim", str(DIM), "--topk", str(k), "--param", "OPQ8,IVF8,PQ8"], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT, MEVI_OPQ_NITER="4"))
    assert r.returncode == 0, r.stderr[-1500:]
    assert "Param OPQ8,IVF8,PQ8 trained: False." in r.stdout and f"int64 ({nq}, {k}) float32 ({nq}, {k})" in r.stdout
    line = [l for l in r.stderr.splitlines() if "recall vs exact search" in l]
    assert len(line) == 1 and "OPQ8,IVF8,PQ8 nprobe=1" in line[0] and "@1 " in line[0] and "@10 " in line[0]
    assert "niter 4" in line[0] and "training error" in line[0] and f"{nd * 8} bytes of codes" in line[0]
    rows = [l.rstrip("\n").split("\t") for l in open(tmp_path / "out.tsv")]
    assert len(rows) == nq and all(len(r_[2].split(",")) == k for r_ in rows)
