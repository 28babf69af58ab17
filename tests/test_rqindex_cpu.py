"""Host side of the residual-quantiser indexes (mevi_amd/rqindex.py, include/mevi_hip_aq.h) without a GPU: the factory strings, the
header and its bindings, the workspace and tile arithmetic (monotone, capped, 0 just outside every bound), every documented refusal
with its status and message before anything is launched (the pointers handed over are null or fake), the routing envelope, and the
references of the GPU tests (tests/aq_cases.py): the tables against pair_dot, the scan against a float64 ADC, the rule by which
levels are encoded in groups against the oracle's encoder over all levels, and the case in which the index is exact."""
import os
import re

import numpy as np
import pytest

import aq_cases as ac
import ivfpq_cases as pc
from oracle import dense as odense
from oracle import rq as orq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def test_parse_factory_table():
    from mevi_amd import dense, ivf, ivfpq, opq, pqfs, refine, rqindex, sq

    table = {"RQ64x8": (None, 64, 8), "IVF100,RQ64x8": (100, 64, 8), "RQ8x8": (None, 8, 8), "RQ12x4": (None, 12, 4), "RQ32x1": (None, 32, 1),
             " IVF7 , RQ8x8 ": (7, 8, 8), "IVF4096,RQ96x8": (4096, 96, 8), "RQ6x8": (None, 6, 8)}
    for text, want in table.items():
        assert rqindex.parse_factory(text) == want, text
        assert all(m.parse_factory(text) is None for m in (ivf, ivfpq, pqfs, sq, opq, refine)), text
        assert rqindex.factory_name(*want) == text.replace(" ", "")
        assert refine.parse_factory(text + ",RFlat") == ("rqindex", want) and refine.parse_factory(text + ",Refine(Flat)") == ("rqindex", want)
        assert dense.is_trained_before_train(text) is False
    for text in ("RQ8", "RQ", "RQ8x", "RQ8x0", "RQ8x9", "RQ8x16", "RQ1x16-6x8", "RQ8x8_Nqint8", "RQ8x8_Nfloat", "RQ8x8_Nnone", "LSQ8x8",
                 "PRQ2x4x8", "PLSQ2x4x8", "OPQ8,RQ8x8", "OPQ8,IVF7,RQ8x8", "IVF7,RQ8", "IVF,RQ8x8", "IVF7_HNSW32,RQ8x8", "RQ8x8,Flat",
                 "RQ8x8,RFlat", "rq8x8", "RQ8x8x8", "PQ8x8", "IVF7,PQ8", "Flat", ""):
        assert rqindex.parse_factory(text) is None, text
    for text in ("RQ8,RFlat", "LSQ8x8,RFlat", "OPQ8,RQ8x8,RFlat", "RQ8x8_Nqint8,RFlat", "RQ8x8,Refine(SQ8)", "RQ8x8,RFlat,RFlat"):
        assert refine.parse_factory(text) is None, text
    assert dense.is_trained_before_train("RQ8x8") is False and dense.is_trained_before_train("IVF7,RQ8x8,RFlat") is False


def test_header_is_included_exported_and_bound(L):
    from mevi_amd import dense, hip

    assert '#include "mevi_hip_aq.h"' in open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    raw = open(os.path.join(ROOT, "include", "mevi_hip_aq.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mevi_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["mevi_aq_lut_f32", "mevi_aq_scan_query_tile", "mevi_aq_scan_topk_f32", "mevi_aq_scan_workspace_bytes",
                        "mevi_rq_residual_f32"]
    assert hip.exported_symbols("mevi_hip_aq.h") == declared and declared == sorted(hip._AQ_SIGNATURES)
    for other in ("mevi_hip.h", "mevi_hip_fine_agg.h", "mevi_hip_attn_long.h", "mevi_hip_ivfpq.h", "mevi_hip_pqfs.h", "mevi_hip_sq.h",
                  "mevi_hip_opq.h", "mevi_hip_graph.h", "mevi_hip_graph_levels.h", "mevi_hip_refine.h"):
        assert not set(declared) & set(hip.exported_symbols(other)), other
    assert all(callable(getattr(L, n)) for n in declared)
    for name in declared:                          # argument counts of the declarations = those of the signature table
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text, flags=re.S).group(1)
        assert len([a for a in args.split(",") if a.strip()]) == len(hip._AQ_SIGNATURES[name][1]), name
    assert int(re.search(r"#define MEVI_AQ_LUT_QUERY_TILE (\d+)", text).group(1)) == dense.AQ_LUT_QUERY_TILE
    assert int(re.search(r"#define MEVI_AQ_LUT_FEW_QUERIES (\d+)", text).group(1)) == dense.AQ_LUT_FEW_QUERIES
    # the scan takes the arguments of the product quantiser's, one for one
    both = [re.sub(r"\s+", " ", re.search(r"\b" + n + r"\s*\(([^)]*)\)", t, flags=re.S).group(1)).replace("int64_t m,", "int64_t M,")
            for n, t in (("mevi_aq_scan_topk_f32", text),
                         ("mevi_ivfpq_scan_topk_f32", open(os.path.join(ROOT, "include", "mevi_hip_ivfpq.h")).read()))]
    assert [a.split()[-1] for a in both[0].split(",")] == [a.split()[-1] for a in both[1].split(",")]
    assert L.mevi_abi_version() == 1
    for name in ("aq_lut", "aq_scan_topk", "aq_scan_workspace_bytes", "aq_scan_query_tile", "rq_residual"):
        assert callable(getattr(dense, name))
    # what the header says a clamped code subtracts
    assert "a code < 0 subtracts codebook[g][0], a code >= K subtracts codebook[g][K-1]" in re.sub(r"\s*\n \*\s*", " ", raw)


#        nq, nprobe, k, dim, M, K, nlist, max_list_len
C2 = (6980, 16, 1000, 768, 64, 256, 100, 200000)


def test_workspace_and_tile_are_host_arithmetic_monotone_and_capped(L):
    from mevi_amd import dense

    f, tile = L.mevi_aq_scan_workspace_bytes, L.mevi_aq_scan_query_tile
    cap = dense.IVF_WORKSPACE_CAP
    assert 0 < f(*C2) <= cap and f(*C2) == dense.aq_scan_workspace_bytes(*C2)
    # the same rows of M bytes and the same tables as the product quantiser's scan: the same bytes and tiles
    assert f(*C2) == L.mevi_ivfpq_scan_workspace_bytes(*C2) and tile(*C2) == L.mevi_ivfpq_scan_query_tile(*C2)
    assert tile(*C2) == dense.aq_scan_query_tile(*C2) == (2 << 30) // (16 * 200000 * 4)
    assert tile(6980, 1, 10, 16, 4, 16, 8, 1000) == 4096 and tile(33, 1, 10, 16, 4, 16, 8, 1000) == 33
    assert tile(6980, 1, 10, 768, 64, 256, 8, 1000) == (128 << 20) // (64 * 256 * 4) == 2048
    assert tile(6980, 1, 10, 768, 96, 256, 8, 1000) == (128 << 20) // (96 * 256 * 4) == 1365
    assert tile(20, 256, 4096, 4, 4, 16, 300, 262144) == 8               # the tiling case of the GPU tests: 8, 8, 4
    grids = {0: [1, 2, 31, 32, 33, 1365, 1366, 2048, 2049, 4096, 4097, 6980, 100000], 1: [1, 2, 3, 16, 255, 256], 2: [1, 10, 1000, 4096],
             3: [4, 8, 36, 100, 768, 4096], 4: [4, 8, 12, 16, 64, 96], 5: [1, 2, 16, 200, 255, 256], 6: [1, 2, 100, 4096, 262144],
             7: [0, 1, 1023, 1024, 1025, 5000, 200000, 2000000]}
    bases = (C2, (1, 1, 1, 4, 4, 1, 1, 1), (33, 3, 10, 36, 12, 200, 8, 3000), (5, 3, 100, 768, 96, 256, 10, 2000))
    for axis, values in grids.items():
        for other in bases:
            sizes = []
            for v in values:
                shape = list(other)
                shape[axis] = v
                sizes.append(f(*shape))
            assert all(s > 0 for s in sizes), (axis, other, sizes)
            assert sizes == sorted(sizes), (axis, other, sizes)          # never shrinks when an argument grows
            assert max(sizes) <= cap
    assert f(1 << 40, 256, 4096, 4096, 96, 256, 262144, (2 << 30) // (4 * 256)) <= cap      # the largest shape of the envelope
    assert f(1, 256, 4096, 768, 96, 256, 262144, (2 << 30) // (4 * 256)) > 0


def test_sizes_are_zero_just_outside_every_bound(L):
    inside = (8, 2, 10, 36, 16, 256, 8, 1000)
    assert L.mevi_aq_scan_workspace_bytes(*inside) > 0 and L.mevi_aq_scan_query_tile(*inside) == 8
    edges = {"nq 0": (0, 2, 10, 36, 16, 256, 8, 1000), "nprobe 0": (8, 0, 10, 36, 16, 256, 8, 1000),
             "nprobe 257": (8, 257, 10, 36, 16, 256, 8, 1000), "k 0": (8, 2, 0, 36, 16, 256, 8, 1000),
             "k 4097": (8, 2, 4097, 36, 16, 256, 8, 1000), "dim % 4": (8, 2, 10, 38, 16, 256, 8, 1000), "dim 0": (8, 2, 10, 0, 16, 256, 8, 1000),
             "dim 2": (8, 2, 10, 2, 16, 256, 8, 1000), "dim 2^24": (8, 2, 10, 1 << 24, 16, 256, 8, 1000),
             "M % 4": (8, 2, 10, 36, 18, 256, 8, 1000), "M 0": (8, 2, 10, 36, 0, 256, 8, 1000), "M 2": (8, 2, 10, 36, 2, 256, 8, 1000),
             "M 100": (8, 2, 10, 36, 100, 16, 8, 1000), "K 0": (8, 2, 10, 36, 16, 0, 8, 1000), "K 257": (8, 2, 10, 36, 16, 257, 8, 1000),
             "nlist 0": (8, 2, 10, 36, 16, 256, 0, 1000), "nlist 262145": (8, 2, 10, 36, 16, 256, 262145, 1000),
             "max_list_len -1": (8, 2, 10, 36, 16, 256, 8, -1), "candidates": (8, 256, 10, 36, 16, 256, 8, (2 << 30) // (4 * 256) + 4)}
    for name, shape in edges.items():
        assert L.mevi_aq_scan_workspace_bytes(*shape) == 0 and L.mevi_aq_scan_query_tile(*shape) == 0, name
    # ... and the last shapes inside: 96 levels of 256 centroids are the 96 KiB table, 4 x 1 at dim 4 the smallest
    for shape in [(8, 256, 4096, (1 << 24) - 4, 96, 256, 262144, (2 << 30) // (4 * 256)), (1, 1, 1, 4, 4, 1, 1, 0)]:
        assert L.mevi_aq_scan_workspace_bytes(*shape) > 0, shape


def test_scan_refusals_come_before_any_launch(L):
    from mevi_amd import hip

    A = 1 << 20                                    # a fake, well-aligned device address: nothing may dereference it

    def call(q=A, nq=8, dim=36, book=A, M=16, K=256, codes=A, off=A, ids=A, nd=5000, nlist=8, longest=1000, probe=A, bias=A, nprobe=2,
             k=10, out_s=A, out_i=A, ws=A, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.mevi_aq_scan_workspace_bytes(nq, nprobe, k, dim, M, K, nlist, longest)
        st = L.mevi_aq_scan_topk_f32(q, nq, dim, book, M, K, codes, off, ids, nd, nlist, longest, probe, bias, nprobe, k, out_s, out_i,
                                     ws, ws_bytes, None)
        return st, L.mevi_last_error().decode()

    def refused(code, word, **kw):
        st, msg = call(**kw)
        assert st == code and word in msg and msg.startswith("aq_scan:"), (kw, st, msg)
        with pytest.raises(hip.MeviHipError, match="aq_scan"):
            hip.check(st, "mevi_aq_scan_topk_f32")

    for nq in (8, 0):                              # the shape is judged with and without queries
        refused(UNSUPPORTED, "M=18", M=18, nq=nq)
        refused(UNSUPPORTED, "M=2", M=2, nq=nq)
        refused(UNSUPPORTED, "M=100", M=100, K=16, nq=nq)
        refused(UNSUPPORTED, "K=0", K=0, nq=nq)
        refused(UNSUPPORTED, "K=257", K=257, nq=nq)
        refused(UNSUPPORTED, "dim=38", dim=38, nq=nq)
        refused(UNSUPPORTED, "dim=2", dim=2, nq=nq)
        refused(UNSUPPORTED, "dim=16777216", dim=1 << 24, nq=nq)
        refused(UNSUPPORTED, "k=0", k=0, nq=nq)
        refused(UNSUPPORTED, "k=4097", k=4097, nq=nq)
        refused(UNSUPPORTED, "nprobe=0", nprobe=0, nq=nq)
        refused(UNSUPPORTED, "nprobe=257", nprobe=257, nq=nq)
        refused(UNSUPPORTED, "32 bits", nd=1 << 31, nq=nq)
        refused(UNSUPPORTED, "nlist=262145", nlist=262145, nq=nq)
        refused(UNSUPPORTED, "max_list_len", nd=(1 << 31) - 1, longest=(2 << 30) // (4 * 256) + 4, nprobe=256, nq=nq)
        refused(INVALID, "max_list_len", longest=5001, nq=nq)
    for name in ("q", "book", "codes", "off", "probe", "out_s", "out_i", "ws"):
        refused(INVALID, "null", **{name: None})
    for name, step in (("q", 8), ("book", 4), ("codes", 4), ("off", 4), ("ids", 4), ("out_i", 4), ("probe", 2), ("bias", 2), ("out_s", 2),
                       ("ws", 128)):
        refused(INVALID, "align", **{name: A + step})
    refused(INVALID, "align", M=12, codes=A + 2)   # M % 16 != 0: rows are read as dwords
    refused(INVALID, "nq=-1", nq=-1, ws_bytes=0)
    need = L.mevi_aq_scan_workspace_bytes(8, 2, 10, 36, 16, 256, 8, 1000)
    refused(WORKSPACE, str(need), ws_bytes=need - 1)
    refused(WORKSPACE, str(need), ws_bytes=0)
    # what is optional: no row ids, no bias, dword-aligned codes when M % 16 != 0; no queries: nothing to do, whatever the pointers
    assert call(nq=0, q=None, ws=None, ws_bytes=0, ids=None, bias=None)[0] == 0
    assert call(nq=0, M=12, codes=A + 4)[0] == 0


def test_lut_and_residual_refusals_come_before_any_launch(L):
    A = 1 << 20

    def lut(q=A, nq=8, dim=36, book=A, M=4, K=16, out=A):
        return L.mevi_aq_lut_f32(q, nq, dim, book, M, K, out, None), L.mevi_last_error().decode()

    def res(x=A, n=8, dim=36, book=A, G=3, K=16, codes=A, stride=3, out=A):
        return L.mevi_rq_residual_f32(x, n, dim, book, G, K, codes, stride, out, None), L.mevi_last_error().decode()

    def refused(fn, prefix, code, word, **kw):
        st, msg = fn(**kw)
        assert st == code and word in msg and msg.startswith(prefix), (kw, st, msg)

    for nq in (8, 0):
        refused(lut, "aq_lut:", UNSUPPORTED, "dim=38", dim=38, nq=nq)
        refused(lut, "aq_lut:", UNSUPPORTED, "dim=0", dim=0, nq=nq)
        refused(lut, "aq_lut:", UNSUPPORTED, "dim=16777216", dim=1 << 24, nq=nq)
        refused(lut, "aq_lut:", UNSUPPORTED, "M * K", M=1 << 16, K=1 << 15, nq=nq)
        refused(lut, "aq_lut:", INVALID, "M=0", M=0, nq=nq)
        refused(lut, "aq_lut:", INVALID, "K=-1", K=-1, nq=nq)
        refused(lut, "aq_lut:", INVALID, "dim=-4", dim=-4, nq=nq)
    refused(lut, "aq_lut:", INVALID, "nq=-1", nq=-1)
    refused(lut, "aq_lut:", UNSUPPORTED, "nq=", nq=1 << 31)
    for name in ("q", "book", "out"):
        refused(lut, "aq_lut:", INVALID, "null", **{name: None})
    for name, step in (("q", 8), ("book", 4), ("out", 2)):
        refused(lut, "aq_lut:", INVALID, "align", **{name: A + step})
    assert lut(nq=0, q=None, book=None, out=None)[0] == 0 and lut(nq=0, q=A + 1)[0] == 0

    for n in (8, 0):
        refused(res, "rq_residual:", UNSUPPORTED, "dim=38", dim=38, n=n)
        refused(res, "rq_residual:", UNSUPPORTED, "dim=0", dim=0, n=n)
        refused(res, "rq_residual:", UNSUPPORTED, "G=257", G=257, stride=257, n=n)
        refused(res, "rq_residual:", INVALID, "code_stride=2", stride=2, n=n)
        refused(res, "rq_residual:", INVALID, "G=0", G=0, n=n)
        refused(res, "rq_residual:", INVALID, "K=0", K=0, n=n)
    refused(res, "rq_residual:", INVALID, "n=-1", n=-1)
    refused(res, "rq_residual:", UNSUPPORTED, "n=", n=1 << 31)
    for name in ("x", "book", "codes", "out"):
        refused(res, "rq_residual:", INVALID, "null", **{name: None})
    for name, step in (("x", 8), ("book", 4), ("out", 4), ("codes", 2)):
        refused(res, "rq_residual:", INVALID, "align", **{name: A + step})
    assert res(n=0, x=None, book=None, codes=None, out=None)[0] == 0 and res(stride=7, n=0)[0] == 0


def test_routing_envelope_of_dense_search(L, monkeypatch):
    """`rqindex.wanted`: which (string, shape) pairs dense.search serves with the index; the others keep the exact search."""
    from mevi_amd import refine, rqindex

    monkeypatch.delenv("MEVI_RQINDEX", raising=False)
    monkeypatch.delenv("MEVI_REFINE", raising=False)
    monkeypatch.delenv("MEVI_REFINE_K_FACTOR", raising=False)
    assert rqindex.wanted("RQ8x8", 4096, 32, 10) == (None, 8, 8) and rqindex.wanted("RQ64x8", 8841823, 768, 1000) == (None, 64, 8)
    assert rqindex.wanted("IVF100,RQ64x8", 8841823, 768, 1000) == (100, 64, 8) and rqindex.wanted("RQ96x8", 5000, 768, 4096) == (None, 96, 8)
    assert rqindex.wanted("RQ12x4", 4096, 36, 10) == (None, 12, 4)       # any dim % 4 == 0: the levels are full-width
    assert rqindex.wanted("RQ6x8", 4096, 32, 10) is None                 # M % 4 != 0
    assert rqindex.wanted("RQ8x8", 4096, 30, 10) is None                 # dim % 4 != 0
    assert rqindex.wanted("RQ8x9", 4096, 32, 10) is None and rqindex.wanted("RQ8", 4096, 32, 10) is None
    assert rqindex.wanted("RQ8x8", 255, 32, 10) is None and rqindex.wanted("RQ8x4", 255, 32, 10) == (None, 8, 4)      # fewer rows than K
    assert rqindex.wanted("IVF5000,RQ8x8", 4096, 32, 10) is None         # nlist > nd
    assert rqindex.wanted("RQ8x8", 4096, 32, 4097) is None and rqindex.wanted("RQ8x8", 4096, 32, 5000) is None        # topk > 4096
    assert rqindex.wanted("RQ100x8", 5000, 768, 10) is None and rqindex.wanted("RQ128x7", 5000, 768, 10) is None      # M > 96
    assert rqindex.wanted("RQ8x8,RFlat", 4096, 32, 10) is None           # the suffixed string is the refine module's
    assert refine.wanted("RQ8x8,RFlat", 4096, 32, 10) == ("rqindex", (None, 8, 8))
    assert refine.wanted("IVF7,RQ8x8,Refine(Flat)", 4096, 32, 10) == ("rqindex", (7, 8, 8)) and refine.wanted("RQ6x8,RFlat", 4096, 32, 10) is None
    monkeypatch.setenv("MEVI_RQINDEX", "exact")
    assert rqindex.wanted("RQ8x8", 4096, 32, 10) is None and refine.wanted("RQ8x8,RFlat", 4096, 32, 10) is None
    assert refine.wanted("PQ8,RFlat", 4096, 32, 10) == ("ivfpq", (None, 8, 8))       # the switch is this family's alone


def test_docstrings_state_what_is_and_is_not_built():
    import faiss_search
    from mevi_amd import dense, rqindex

    for word in ("greedy", "GREEDY", "max_beam_size", "seeded from our own RNG", "LSQ", "PRQ", "torchrun", "MEVI_RQINDEX=exact"):
        assert word.lower() in rqindex.__doc__.lower(), word
    assert "RQ<M>x<b>" in dense.search.__doc__ and "RQ<M>x<b>" in faiss_search.__doc__


def test_lookup_tables_are_pair_dot_bit_for_bit():
    """`luts` (one oracle call per level), the tables tests/ivfpq_cases.py builds for `as_product`, and the definition
    (oracle.dense.pair_dot per entry): the same bits, with repeated centroids, a zero centroid, a zero query, K no power of two."""
    rng = np.random.default_rng(9)
    for dim, M, K, nq in ((4, 4, 16, 3), (36, 12, 200, 4), (100, 8, 1, 2), (768, 8, 256, 2)):
        q = rng.standard_normal((nq, dim)).astype(np.float32)
        book = rng.standard_normal((M, K, dim)).astype(np.float32)
        book[:, K // 2] = book[:, 0]
        book[0, K - 1] = 0.0
        q[-1] = 0.0
        a, b, c = ac.luts(q, book), ac.luts_by_pair_dot(q, book), pc.luts(*ac.as_product(q, book))
        assert a.shape == (nq, M, K) and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (dim, M, K)
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), (dim, M, K)


def test_aq_expected_agrees_with_float64():
    """The reference, not the kernel: every score within the sum of the rounding bounds of its M adds and M chains of dim fmas (each
    of the M + dim roundings on a row's path at most 2^-24 of the sum of the absolute terms) of bias + <q, reconstruct(codes)> in
    float64; the order the float64 order wherever float64 scores differ by more than both bounds; the probe rules; padding."""
    q, book, codes, off, ids, probe, bias = ac.random_index(5, 36, 8, 16, 6, 400, 5, 3)
    probe[1, 1] = -1
    probe[2, 2] = 5                                   # past the last list
    probe[3, 1] = probe[3, 0]                         # a list named twice: the first slot's bias counts
    probe[4] = -1
    k = 60
    s, i = ac.aq_expected(q, book, codes, off, ids, probe, bias, k)
    assert s.dtype == np.float32 and i.dtype == np.int64 and (i[4] == -1).all() and (s[4] == -np.finfo(np.float32).max).all()
    row_of = np.argsort(ids)
    M, _, dim = book.shape
    for n in range(len(q)):
        slots = ac.clean_slots(probe[n], 5)
        if n == 3:
            assert [s_ for s_, _ in slots] == [0, 2]
        rows = np.concatenate([np.arange(off[l], off[l + 1]) for _, l in slots]) if slots else np.zeros(0, np.int64)
        b = np.concatenate([np.full(off[l + 1] - off[l], bias[n, s_], np.float64) for s_, l in slots]) if slots else np.zeros(0)
        exact = ac.aq_float64(q[n], book, codes[rows], 0.0) + b
        mag = np.abs(b) + sum((np.abs(book[j][codes[rows, j]].astype(np.float64)) * np.abs(q[n].astype(np.float64))).sum(1) for j in range(M))
        bound = (M + dim + 1) * 2.0 ** -24 * mag
        found = i[n][i[n] >= 0]
        assert len(found) == min(k, len(rows)) and len(set(found.tolist())) == len(found) and set(found.tolist()) <= set(ids[rows].tolist())
        where = {int(r): t for t, r in enumerate(rows)}
        at = np.array([where[int(row_of[d])] for d in found], np.int64)
        assert (np.abs(s[n][:len(found)].astype(np.float64) - exact[at]) <= bound[at]).all()
        assert (np.diff(s[n][:len(found)]) <= 0).all()
        ties = np.flatnonzero(np.diff(s[n][:len(found)]) == 0)
        assert (found[ties] < found[ties + 1]).all()
        if len(rows) > k:                             # nothing left out beats the last one kept by more than both bounds
            out = np.setdiff1d(np.arange(len(rows)), at)
            assert (exact[out] - bound[out] <= exact[at[-1]] + bound[at[-1]]).all()


def test_encoding_levels_in_groups_is_encoding_them_at_once():
    """oracle.rq.rq_encode of 12 levels = 8 levels, the sequential f32 subtraction of their centroids, 4 levels: the rule
    `rqindex.encode` follows on the device.  With duplicate centroids (the lowest index wins in both) and groups of other sizes."""
    rng = np.random.default_rng(17)
    for dim, M, K, n in ((36, 12, 16, 300), (128, 12, 256, 200), (32, 16, 7, 150)):
        x = rng.standard_normal((n, dim)).astype(np.float32)
        book = (rng.standard_normal((M, K, dim)) * (0.7 ** np.arange(M))[:, None, None]).astype(np.float32)
        book[:, K - 1] = book[:, 0]
        book[3, K // 2] = book[3, 1]
        whole = orq.rq_encode(x, book)
        first = orq.rq_encode(x, book[:8])
        left = x.copy()
        for j in range(8):                           # reconstruct-style, level by level: one rounded subtraction each
            left = left - book[j][first[:, j]]
        assert np.array_equal(left.view(np.uint32), ac.residual_expected(x, book[:8], first).view(np.uint32))
        assert np.array_equal(whole, np.concatenate([first, orq.rq_encode(left, book[8:])], axis=1)), (dim, M, K)
        for group in (1, 3, 8):
            assert np.array_equal(whole, ac.chained_encode(x, book, group)), (dim, M, K, group)
        assert (whole != K - 1).all() or K == 1          # a duplicate never takes the higher index
    # the residual restated: what x - reconstruct would NOT give (it rounds the sum of centroids first)
    assert not np.array_equal(left, x - orq.reconstruct(first, book[:8]))
    clamped = ac.residual_expected(x[:4], book[:2], np.array([[-5, 0], [K, 99], [0, K - 1], [1, -1]]))
    assert np.array_equal(clamped, ac.residual_expected(x[:4], book[:2], np.array([[0, 0], [K - 1, K - 1], [0, K - 1], [1, 0]])))


def test_an_index_whose_first_level_is_the_rows_is_exact():
    """nd = K distinct rows, level 0 of the codebook = the rows, every other level zero: every row encodes to (its own index, 0, ...),
    its table entry is the exact search's chain and the adds of +0 keep it, so the reference's top-k are oracle.dense.ip_topk_exact's."""
    rng = np.random.default_rng(23)
    K, dim, M = 64, 36, 8
    rows = rng.standard_normal((K, dim)).astype(np.float32)
    q = rng.standard_normal((5, dim)).astype(np.float32)
    book = np.zeros((M, K, dim), np.float32)
    book[0] = rows
    codes = orq.rq_encode(rows, book)
    assert np.array_equal(codes[:, 0], np.arange(K)) and (codes[:, 1:] == 0).all()
    off = np.array([0, K], np.int64)
    s, i = ac.aq_expected(q, book, codes.astype(np.uint8), off, None, np.zeros((5, 1), np.int32), None, 10)
    es, ei = odense.ip_topk_exact(q, rows, 10)
    assert np.array_equal(i, ei) and np.array_equal(s.view(np.uint32), (es + np.float32(0)).view(np.uint32))
