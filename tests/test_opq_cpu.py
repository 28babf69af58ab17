"""Host side of the OPQ index (mevi_amd/opq.py, include/mevi_hip_opq.h) without a GPU: the factory strings and the routing
envelope, the header and its binding, every refusal of mevi_opq_rotate_rows_f32 before a launch, and the properties of what
the GPU tests compare against (tests/opq_cases.py): the float64 trainer on both anisotropic corpora and `rotate_expected`
against float64."""
import functools
import os
import re

import numpy as np
import pytest

import opq_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, DIM, M, K, NITER, NQ = 4096, 32, 8, 16, 10, 64


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def test_parse_factory_and_wanted_table(L, monkeypatch):
    from mevi_amd import ivf, ivfpq, opq, pqfs, sq

    monkeypatch.delenv("MEVI_OPQ", raising=False)
    served = {"OPQ8,PQ8": (8, None, 8, 8, False), "OPQ8,PQ8x4": (8, None, 8, 4, False), "OPQ8,IVF8,PQ8": (8, 8, 8, 8, False),
              "OPQ8,IVF100,PQ8x6": (8, 100, 8, 6, False), "OPQ8,PQ8x4fs": (8, None, 8, 4, True),
              "OPQ8,IVF8,PQ8x4fs": (8, 8, 8, 4, True), "OPQ8_32,PQ8": (8, None, 8, 8, False), "OPQ8_32,IVF8,PQ8x4": (8, 8, 8, 4, False),
              "OPQ8_32,PQ8x4fs": (8, None, 8, 4, True), " OPQ8 , IVF8 , PQ8 ": (8, 8, 8, 8, False), " OPQ8_32 ,PQ8x4fs ": (8, None, 8, 4, True),
              "OPQ4,PQ8": (4, None, 8, 8, False)}
    for text, want in served.items():
        spec = opq.parse_factory(text)
        assert spec is not None and (spec[0],) + spec[2:] == want, text
        assert opq.wanted(text, 4096, 32, 10) == want, text
        for other in (ivf, ivfpq, pqfs, sq):                               # no other parser takes them
            assert other.parse_factory(text) is None, (text, other)
    for text in ("OPQ8_16,PQ8", "OPQ8,SQ8", "OPQ8,Flat", "OPQ8,HNSW32", "OPQ,PQ8", "opq8,PQ8", "OPQ8,PQ8x9", "OPQ8,IVF8,PQ8,RFlat",
                 "OPQ8", "OPQ8,", "PQ8", "IVF8,PQ8", "OPQ8,IVF8,Flat", "OPQ8,OPQ8,PQ8", "OPQ8_32", "OPQ8_,PQ8", "PCA32,PQ8", ""):
        assert opq.wanted(text, 4096, 32, 10) is None, text
    assert opq.parse_factory("OPQ8_16,PQ8") == (8, 16, None, 8, 8, False)       # parsed, and refused by `wanted` at dim 32 ...
    assert opq.wanted("OPQ8_16,PQ8", 4096, 16, 10) is None                       # ... and at dim 16: 16 / 8 is no multiple of 4
    assert opq.wanted("OPQ4_16,PQ4", 4096, 16, 10) == (4, None, 4, 8, False)
    for text in ("OPQ8,SQ8", "OPQ8,Flat", "OPQ8,HNSW32", "OPQ,PQ8", "opq8,PQ8", "OPQ8,PQ8x9", "OPQ8,IVF8,PQ8,RFlat"):
        assert opq.parse_factory(text) is None, text


def test_routing_envelope_of_dense_search(L, monkeypatch):
    from mevi_amd import dense, opq

    monkeypatch.delenv("MEVI_OPQ", raising=False)
    assert opq.wanted("OPQ64,IVF4096,PQ64", 8841823, 768, 1000) == (64, 4096, 64, 8, False)
    assert opq.wanted("OPQ64,PQ64x4fs", 8841823, 768, 1000) == (64, None, 64, 4, True)
    assert opq.wanted("OPQ5,PQ8", 4096, 32, 10) is None                          # dim % M != 0
    assert opq.wanted("OPQ16,PQ8", 4096, 32, 10) is None                         # dim / M = 2: outside mevi_pq_encode_f32
    assert opq.wanted("OPQ8,PQ8", 255, 32, 10) is None                           # fewer rows than the training PQ has centroids
    assert opq.wanted("OPQ8,PQ8x4", 255, 32, 10) is None and opq.wanted("OPQ8,PQ8x4", 256, 32, 10) == (8, None, 8, 4, False)
    assert opq.wanted("OPQ8,PQ5", 4096, 32, 10) is None                          # the inner index outside its own envelope
    assert opq.wanted("OPQ8,PQ4x4fs", 4096, 32, 10) is None                      # m % 8 != 0 for the fast scan
    assert opq.wanted("OPQ8,IVF5000,PQ8", 4096, 32, 10) is None                  # nlist > rows
    assert opq.wanted("OPQ8,PQ8", 4096, 32, 4097) is None                        # topk > 4096
    monkeypatch.setenv("MEVI_OPQ", "exact")
    assert opq.wanted("OPQ8,PQ8", 4096, 32, 10) is None and opq.wanted("OPQ8,IVF8,PQ8x4fs", 4096, 32, 10) is None
    assert opq.parse_factory("OPQ8,PQ8") is not None
    assert not dense.is_trained_before_train("OPQ8,PQ8") and not dense.is_trained_before_train("OPQ8,IVF8,PQ8x4fs")


def test_header_is_included_exported_and_bound(L):
    from mevi_amd import dense, hip

    assert '#include "mevi_hip_opq.h"' in open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    raw = open(os.path.join(ROOT, "include", "mevi_hip_opq.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mevi_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["mevi_opq_rotate_rows_f32"]
    assert hip.exported_symbols("mevi_hip_opq.h") == declared and not set(declared) & set(hip.exported_symbols())
    fn = L.mevi_opq_rotate_rows_f32
    args = re.search(r"mevi_opq_rotate_rows_f32\s*\(([^)]*)\)", text).group(1).split(",")
    assert len(fn.argtypes) == len(args) == 11                               # every argument of the declaration is bound
    for c_type, decl in zip(fn.argtypes, args):
        assert ("*" in decl) == (c_type.__name__ == "c_void_p") and ("int64_t " in decl or "*" in decl), decl
    assert callable(dense.opq_rotate_rows) and dense.OPQ_MAX_DIM == 4096


def test_rotate_refusals_come_before_any_launch(L):
    oc.check_refusals(L)


# ---- the float64 trainer: what the device trainer is compared with in kind --------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trained(kind, seed):
    X = oc.GENERATORS[kind](seed, N, DIM).astype(np.float64)
    Q = oc.GENERATORS[kind](1000 + seed, NQ, DIM).astype(np.float64)
    R_next, errors, R, book = oc.train_rotation64(X, M, K, NITER, seed=seed)
    plain = oc.train_pq64(X, M, K, 40 + 4 * (NITER - 1), seed=seed)          # as many Lloyd iterations as the last OPQ codebook saw
    return X, Q, R_next, errors, R, book, plain


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("kind", ["outlier", "decaying"])
def test_float64_trainer_lowers_error_and_raises_recall(kind, seed):
    X, Q, R_next, errors, R, book, plain = _trained(kind, seed)
    assert len(errors) == NITER
    for a, b in zip(errors, errors[1:]):                                      # Procrustes and Lloyd steps never raise the error
        assert b <= a * (1 + 1e-9), errors
    for rot in (R_next, R):
        assert np.abs(rot @ rot.T - np.eye(DIM)).max() <= 1e-12
    err_opq, _ = oc.pq_error64(X @ R.T, book)
    assert abs(err_opq - errors[-1]) <= 1e-9 * errors[-1]
    err_pq, _ = oc.pq_error64(X, plain)
    print(f"{kind} seed {seed}: error OPQ {err_opq:.4f} / PQ {err_pq:.4f} = {err_opq / err_pq:.3f}")
    assert err_opq <= 0.75 * err_pq, (err_opq, err_pq)
    rec_opq, rec_pq = oc.adc_recall64(X, Q, R, book), oc.adc_recall64(X, Q, None, plain)
    print(f"{kind} seed {seed}: recall@10 OPQ {rec_opq:.3f} / PQ {rec_pq:.3f}")
    assert rec_opq >= rec_pq + 0.2, (rec_opq, rec_pq)


def test_rotate_expected_agrees_with_float64():
    """The reference, not the kernel: every output within the chain's rounding bound of the float64 value (opq_cases.chain_bound),
    rows gathered in order, repeats equal, zero rows where a row id or a list is out of range and nowhere else."""
    rng = np.random.default_rng(7)
    n_src, dim, nlist = 40, 48, 5
    x = rng.standard_normal((n_src, dim)).astype(np.float32) * 3
    R = oc.random_rotation64(dim, rng).astype(np.float32)
    crot = rng.standard_normal((nlist, dim)).astype(np.float32)
    list_of = rng.integers(0, nlist, size=n_src).astype(np.int32)
    list_of[3], list_of[4] = -1, nlist
    rows = np.concatenate([rng.permutation(n_src)[:20], [7, 7, -1, n_src, 3, 4]]).astype(np.int64)
    got = oc.rotate_expected(x, R, rows, list_of, crot)
    assert got.dtype == np.float32 and got.shape == (len(rows), dim)
    for i, r in enumerate(rows.tolist()):
        if not 0 <= r < n_src or not 0 <= list_of[r] < nlist:
            assert (got[i] == 0).all()
            continue
        exact = R.astype(np.float64) @ x[r].astype(np.float64) - crot[list_of[r]].astype(np.float64)
        assert (np.abs(got[i] - exact) <= oc.chain_bound(x[r], R, crot[list_of[r]])).all()
        assert np.abs(got[i]).max() > 0
    assert np.array_equal(got[20], got[21])
    plain = oc.rotate_expected(x, R)
    assert plain.shape == (n_src, dim)
    assert (np.abs(plain - x.astype(np.float64) @ R.astype(np.float64).T) <= oc.chain_bound(x, R)).all()
    want = plain[7] - crot[list_of[7]]
    assert np.array_equal(got[20].view(np.uint32), want.view(np.uint32))      # the chain, then one f32 subtraction
