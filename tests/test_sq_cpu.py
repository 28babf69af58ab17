"""Host side of the scalar-quantised index (mevi_amd/sq.py, include/mevi_hip_sq.h) without a GPU: the factory strings, the header
and its bindings, the workspace and tile arithmetic (monotone, capped, 0 outside every bound of the envelope), every documented
refusal with its status and the word that names the argument before anything is launched (the pointers handed over are null or
fake), and the properties of the reference of the GPU tests (tests/sq_cases.py)."""
import os
import re

import numpy as np
import pytest

import sq_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
U = 2.0 ** -24                                     # the relative error bound of one f32 rounding


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def test_parse_factory_table():
    from mevi_amd import ivf, ivfpq, sq

    table = {"SQ8": (None, 8), "SQ4": (None, 4), "IVF8,SQ8": (8, 8), "IVF100,SQ4": (100, 4), "IVF4096,SQ8": (4096, 8),
             " IVF8 , SQ4 ": (8, 4), " SQ8 ": (None, 8)}
    for text, want in table.items():
        assert sq.parse_factory(text) == want, text
        assert ivf.parse_factory(text) is None and ivfpq.parse_factory(text) is None, text      # no other parser takes them
    for text in ("SQ6", "SQfp16", "SQbf16", "SQ8_direct", "SQ4np", "SQ", "IVF8,SQ", "IVF8_HNSW32,SQ8", "HNSW32,SQ8", "SQ8,RFlat",
                 "OPQ16,SQ8", "", "Flat", "IVF8,Flat", "IVF8,PQ4", "PQ8", "HNSW32", "SQ84", "SQ48", "IVF,SQ8", "IVF8,SQ8,Flat", "sq8"):
        assert sq.parse_factory(text) is None, text


def test_header_is_included_exported_and_bound(L):
    from mevi_amd import dense, hip

    assert '#include "mevi_hip_sq.h"' in open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    raw = open(os.path.join(ROOT, "include", "mevi_hip_sq.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mevi_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["mevi_sq_encode_f32", "mevi_sq_scan_query_tile", "mevi_sq_scan_topk_f32", "mevi_sq_scan_workspace_bytes"]
    assert hip.exported_symbols("mevi_hip_sq.h") == declared and not set(declared) & set(hip.exported_symbols())
    assert all(callable(getattr(L, n)) for n in declared)
    for name in ("sq_scan_topk", "sq_scan_workspace_bytes", "sq_scan_query_tile", "sq_encode"):
        assert callable(getattr(dense, name))


#        nq, nprobe, k, dim, bits, nlist, max_list_len
C2 = (6980, 16, 1000, 768, 8, 100, 200000)


def test_workspace_and_tile_are_host_arithmetic_monotone_and_capped(L):
    from mevi_amd import dense

    f, tile = L.mevi_sq_scan_workspace_bytes, L.mevi_sq_scan_query_tile
    cap = dense.IVF_WORKSPACE_CAP
    assert 0 < f(*C2) <= cap and f(*C2) == dense.sq_scan_workspace_bytes(*C2)
    assert tile(*C2) == dense.sq_scan_query_tile(*C2) == (2 << 30) // (16 * 200000 * 4)
    assert tile(6980, 1, 10, 16, 8, 8, 1000) == 4096 and tile(33, 1, 10, 16, 4, 8, 1000) == 33
    assert tile(20, 256, 4096, 16, 4, 300, 262144) == 8                  # the tiling case of the GPU tests: 8, 8, 4
    assert tile(6980, 1, 1000, 768, 8, 1, 8841823) == (2 << 30) // (4 * 8841824) == 60      # flat SQ8 over the C2 corpus
    # the plan is the IVF-Flat scan's for the same shape, at both widths
    for shape in (C2, (33, 3, 10, 48, 4, 8, 3000), (1, 1, 1, 8, 4, 1, 0)):
        flat = shape[:4] + shape[5:]
        assert f(*shape) == dense.ivf_scan_workspace_bytes(*flat) > 0 and tile(*shape) == dense.ivf_scan_query_tile(*flat)
    grids = {0: [1, 2, 31, 32, 33, 4096, 4097, 6980, 100000], 1: [1, 2, 3, 16, 255, 256], 2: [1, 10, 1000, 4096],
             3: [8, 16, 24, 48, 768, 4096], 5: [1, 2, 100, 4096, 262144], 6: [0, 1, 127, 128, 129, 5000, 200000, 2000000]}
    bases = (C2, (1, 1, 1, 16, 4, 1, 1), (33, 3, 10, 48, 8, 8, 3000), (5, 3, 100, 768, 4, 10, 2000))
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
    assert f(1 << 40, 256, 4096, 4096, 8, 262144, (2 << 30) // (4 * 256)) <= cap       # the largest shape of the envelope
    assert f(1, 256, 4096, 4096, 4, 262144, (2 << 30) // (4 * 256)) > 0


def test_sizes_are_zero_just_outside_every_bound(L):
    inside = (8, 2, 10, 64, 8, 8, 1000)
    assert L.mevi_sq_scan_workspace_bytes(*inside) > 0 and L.mevi_sq_scan_query_tile(*inside) == 8
    edges = {"nq 0": (0, 2, 10, 64, 8, 8, 1000), "nprobe 0": (8, 0, 10, 64, 8, 8, 1000), "nprobe 257": (8, 257, 10, 64, 8, 8, 1000),
             "k 0": (8, 2, 0, 64, 8, 8, 1000), "k 4097": (8, 2, 4097, 64, 8, 8, 1000), "bits 0": (8, 2, 10, 64, 0, 8, 1000),
             "bits 6": (8, 2, 10, 64, 6, 8, 1000), "bits 16": (8, 2, 10, 64, 16, 8, 1000), "bits -8": (8, 2, 10, 64, -8, 8, 1000),
             "dim 0": (8, 2, 10, 0, 8, 8, 1000), "dim % 4 at 8 bits": (8, 2, 10, 66, 8, 8, 1000),
             "dim % 8 at 4 bits": (8, 2, 10, 20, 4, 8, 1000), "dim 4 at 4 bits": (8, 2, 10, 4, 4, 8, 1000),
             "dim 4100": (8, 2, 10, 4100, 8, 8, 1000), "dim 4104 at 4 bits": (8, 2, 10, 4104, 4, 8, 1000),
             "nlist 0": (8, 2, 10, 64, 8, 0, 1000), "nlist 262145": (8, 2, 10, 64, 8, 262145, 1000),
             "max_list_len -1": (8, 2, 10, 64, 8, 8, -1), "candidates": (8, 256, 10, 64, 8, 8, (2 << 30) // (4 * 256) + 4)}
    for name, shape in edges.items():
        assert L.mevi_sq_scan_workspace_bytes(*shape) == 0 and L.mevi_sq_scan_query_tile(*shape) == 0, name
    # ... and the last shapes inside
    for shape in [(8, 256, 4096, 4096, 8, 262144, (2 << 30) // (4 * 256)), (8, 256, 4096, 4096, 4, 262144, (2 << 30) // (4 * 256)),
                  (1, 1, 1, 4, 8, 1, 0), (1, 1, 1, 8, 4, 1, 0), (8, 2, 10, 20, 8, 8, 1000)]:
        assert L.mevi_sq_scan_workspace_bytes(*shape) > 0, shape


def test_scan_refusals_come_before_any_launch(L):
    from mevi_amd import hip

    A = 1 << 20                                    # a fake, well-aligned device address: nothing may dereference it

    def call(q=A, nq=8, dim=64, codes=A, vmin=A, vdiff=A, bits=8, off=A, ids=A, nd=5000, nlist=8, longest=1000, probe=A, bias=A,
             nprobe=2, k=10, out_s=A, out_i=A, ws=A, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.mevi_sq_scan_workspace_bytes(nq, nprobe, k, dim, bits, nlist, longest)
        st = L.mevi_sq_scan_topk_f32(q, nq, dim, codes, vmin, vdiff, bits, off, ids, nd, nlist, longest, probe, bias, nprobe, k,
                                     out_s, out_i, ws, ws_bytes, None)
        return st, L.mevi_last_error().decode()

    def refused(code, word, **kw):
        st, msg = call(**kw)
        assert st == code and word in msg and msg.startswith("sq_scan:"), (kw, st, msg)
        with pytest.raises(hip.MeviHipError, match="sq_scan"):
            hip.check(st, "mevi_sq_scan_topk_f32")

    refused(UNSUPPORTED, "bits=6", bits=6)
    refused(UNSUPPORTED, "bits=0", bits=0)
    refused(UNSUPPORTED, "bits=16", bits=16)
    refused(UNSUPPORTED, "dim=66", dim=66)
    refused(UNSUPPORTED, "dim=20", dim=20, bits=4)
    refused(UNSUPPORTED, "dim=4100", dim=4100)
    refused(UNSUPPORTED, "k=0", k=0)
    refused(UNSUPPORTED, "k=4097", k=4097)
    refused(UNSUPPORTED, "nprobe=0", nprobe=0)
    refused(UNSUPPORTED, "nprobe=257", nprobe=257)
    refused(UNSUPPORTED, "32 bits", nd=1 << 31)
    refused(UNSUPPORTED, "nlist=262145", nlist=262145)
    refused(UNSUPPORTED, "max_list_len", nd=(1 << 31) - 1, longest=(2 << 30) // (4 * 256) + 4, nprobe=256)
    for name in ("q", "codes", "vmin", "vdiff", "off", "probe", "out_s", "out_i", "ws"):
        refused(INVALID, "null", **{name: None})
    for name, step in (("q", 8), ("vmin", 4), ("vdiff", 8), ("codes", 4), ("off", 4), ("ids", 4), ("out_i", 4), ("probe", 2), ("bias", 2),
                       ("out_s", 2), ("ws", 128)):
        refused(INVALID, "align", **{name: A + step})
    refused(INVALID, "align", dim=20, codes=A + 2)            # row bytes % 16 != 0: rows are read as dwords
    refused(INVALID, "align", dim=48, bits=4, codes=A + 2)    # 24 bytes a row
    refused(INVALID, "align", dim=32, bits=4, codes=A + 4)    # 16 bytes a row
    refused(INVALID, "max_list_len", longest=5001)
    refused(INVALID, "nq=-1", nq=-1, ws_bytes=0)
    refused(INVALID, "nd=-1", nd=-1, longest=0)
    refused(INVALID, "nlist=0", nlist=0, ws_bytes=0)
    refused(INVALID, "max_list_len=-1", longest=-1, ws_bytes=0)
    need = L.mevi_sq_scan_workspace_bytes(8, 2, 10, 64, 8, 8, 1000)
    refused(WORKSPACE, str(need), ws_bytes=need - 1)
    refused(WORKSPACE, str(need), ws_bytes=0)
    # what is optional: no row ids, no bias, dword-aligned codes when a row is no multiple of 16 bytes; no queries: nothing to do
    assert call(nq=0, q=None, ws=None, ws_bytes=0, ids=None, bias=None)[0] == 0
    assert call(nq=0, dim=20, codes=A + 4)[0] == 0
    assert call(nq=0, bits=6)[0] == UNSUPPORTED               # ... but the envelope still holds


def test_encode_refusals_come_before_any_launch(L):
    A = 1 << 20

    def call(x=A, n_src=100, dim=64, rows=A, n=50, list_of=A, cent=A, nlist=4, vmin=A, vdiff=A, bits=8, codes=A):
        st = L.mevi_sq_encode_f32(x, n_src, dim, rows, n, list_of, cent, nlist, vmin, vdiff, bits, codes, None)
        return st, L.mevi_last_error().decode()

    def refused(code, word, **kw):
        st, msg = call(**kw)
        assert st == code and word in msg and msg.startswith("sq_encode:"), (kw, st, msg)

    refused(UNSUPPORTED, "bits=6", bits=6)
    refused(UNSUPPORTED, "dim=66", dim=66)
    refused(UNSUPPORTED, "dim=20", dim=20, bits=4)
    refused(UNSUPPORTED, "dim=4100", dim=4100)
    refused(INVALID, "n=-1", n=-1)
    refused(INVALID, "n_src=-1", n_src=-1)
    refused(INVALID, "n=101", n=101, rows=None)
    refused(INVALID, "centroids", cent=None)
    refused(INVALID, "centroids", list_of=None)
    refused(INVALID, "nlist=0", nlist=0)
    for name in ("x", "vmin", "vdiff", "codes"):
        refused(INVALID, "null", **{name: None})
    for name, step in (("x", 8), ("cent", 4), ("vmin", 4), ("vdiff", 8), ("rows", 4), ("list_of", 2), ("codes", 2)):
        refused(INVALID, "align", **{name: A + step})
    assert call(n=0, x=None, codes=None, rows=None)[0] == 0
    assert call(n=0, list_of=None, cent=None, nlist=0)[0] == 0


def test_routing_envelope_of_dense_search(L, monkeypatch):
    """`sq.wanted`: which (string, shape) pairs dense.search serves with the index; the others keep the exact search."""
    from mevi_amd import sq

    monkeypatch.delenv("MEVI_SQ", raising=False)
    assert sq.wanted("SQ8", 1000, 16, 10) == (None, 8) and sq.wanted("SQ8", 8841823, 768, 1000) == (None, 8)
    assert sq.wanted("IVF100,SQ4", 8841823, 768, 1000) == (100, 4) and sq.wanted("IVF8,SQ8", 1000, 20, 4096) == (8, 8)
    assert sq.wanted("IVF8,SQ4", 1000, 20, 10) is None                  # dim % 8 != 0 at 4 bits
    assert sq.wanted("SQ8", 1000, 18, 10) is None                       # dim % 4 != 0
    assert sq.wanted("SQ8", 1000, 4100, 10) is None                     # dim > 4096
    assert sq.wanted("IVF2000,SQ8", 1000, 16, 10) is None               # nlist > nd
    assert sq.wanted("IVF1000,SQ8", 1000, 16, 10) == (1000, 8)
    assert sq.wanted("SQ8", 1000, 16, 4097) is None                     # topk > 4096
    assert sq.wanted("SQ8", (2 << 30) // 4 + 1, 16, 10) is None         # one query's candidates above the cap
    assert sq.wanted("SQ6", 1000, 16, 10) is None and sq.wanted("HNSW32,SQ8", 1000, 16, 10) is None
    assert sq.wanted("IVF8,Flat", 1000, 16, 10) is None and sq.wanted("IVF8,PQ4", 1000, 16, 10) is None
    monkeypatch.setenv("MEVI_SQ", "exact")
    assert sq.wanted("SQ8", 1000, 16, 10) is None and sq.wanted("IVF8,SQ4", 1000, 16, 10) is None


# ---- the reference's own properties -----------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,differ", [(8, 191), (4, 11)])
def test_levels_are_the_f32_quotients_and_not_the_reciprocal_products(bits, differ):
    """T[c] = (c + 0.5f) / L for every level, against the float64 quotient rounded once (the f32 operands are exact in float64 and
    a quotient of two 24-bit numbers never lies close enough to a rounding boundary for a second rounding to matter); the
    reciprocal product (c + 0.5f) * (1.0f / L) is another number for most levels: the trap the header names."""
    from mevi_amd import sq

    Lv = (1 << bits) - 1
    t = sc.levels(bits)
    assert t.dtype == np.float32 and t.shape == (Lv + 1,)
    want = np.array([np.float32((c + 0.5) / Lv) for c in range(Lv + 1)], np.float32)
    assert np.array_equal(t.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(sq.levels(bits).view(np.uint32), t.view(np.uint32))          # the module's table is the same
    trap = (np.arange(Lv + 1, dtype=np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(Lv))
    assert trap.dtype == np.float32 and int((trap != t).sum()) == differ
    assert (np.diff(t) > 0).all() and 0 < t[0] and t[-1] > 1                            # the top level's centre lies past vmax


@pytest.mark.parametrize("bits", [8, 4])
def test_round_trip_stays_within_half_a_step(bits):
    """|decode(encode(x)) - x| <= vdiff / (2L) + slack for rows inside the trained range.  With u = 2^-24 and t = (x - vmin) / vdiff
    exact: the encoder's three roundings (difference, quotient, product with L) move L * t by at most a factor (1 + u)^3, so the
    truncated level c satisfies c - 3.01 u L <= L t <= c + 1 + 3.01 u L, i.e. |(c + 0.5) / L - t| <= 1 / (2L) + 3.01 u; the decoder's
    three roundings (T, product, sum) add 2.01 u * vdiff * T with T < 1.04 and u * |result|.  In all
      slack = u * (3.01 + 2.1) * vdiff + 2 u * max(|x|, |decoded|) <= u * (6 * vdiff + 2 * max(|x|, |decoded|))."""
    rng = np.random.default_rng(3 + bits)
    x = (rng.standard_normal((4000, 24)) * np.array([1e-3, 1.0, 50.0] * 8)).astype(np.float32)
    x[:, 5] += 1000.0                                  # a column far from zero: the ulp of the result dominates its slack
    vmin, vdiff = sc.train_range(x)
    Lv = (1 << bits) - 1
    back = sc.decode(sc.encode(x, vmin, vdiff, bits), vmin, vdiff, bits)
    err = np.abs(back.astype(np.float64) - x.astype(np.float64))
    slack = U * (6 * vdiff.astype(np.float64) + 2 * np.maximum(np.abs(x), np.abs(back)).astype(np.float64))
    assert (err <= vdiff.astype(np.float64) / (2 * Lv) + slack).all()
    assert err.max() > 0.4 * vdiff.max() / Lv          # the bound is not vacuous: errors do reach most of half a step


@pytest.mark.parametrize("bits", [8, 4])
def test_extremes_constant_columns_and_clamping(bits):
    Lv = (1 << bits) - 1
    rng = np.random.default_rng(5)
    x = rng.standard_normal((300, 16)).astype(np.float32)
    x[:, 3] = -2.5                                     # a constant column: vdiff == 0
    x[:, 7] = 0.0
    vmin, vdiff = sc.train_range(x)
    assert vdiff[3] == 0 and vdiff[7] == 0 and (np.delete(vdiff, [3, 7]) > 0).all()
    lo, hi = x.min(0), x.max(0)
    lev = sc.unpack(sc.encode(np.stack([lo, hi]), vmin, vdiff, bits), bits)
    assert (lev[0] == 0).all()                         # a row at vmin codes 0
    assert (np.delete(lev[1], [3, 7]) == Lv).all() and lev[1][3] == 0 and lev[1][7] == 0      # a row at vmax codes L
    back = sc.decode(sc.encode(x, vmin, vdiff, bits), vmin, vdiff, bits)
    assert (back[:, 3] == np.float32(-2.5)).all() and (back[:, 7] == 0).all()                 # ... and decodes to vmin
    # values outside a SUPPLIED range clamp to the end levels
    out = np.stack([lo - 10.0, hi + 10.0, np.full(16, -np.inf), np.full(16, np.inf)]).astype(np.float32)
    lev = sc.unpack(sc.encode(out, vmin, vdiff, bits), bits)
    live = np.delete(np.arange(16), [3, 7])
    assert (lev[0] == 0).all() and (lev[2] == 0).all() and (lev[1][live] == Lv).all() and (lev[3][live] == Lv).all()
    assert (lev[:, [3, 7]] == 0).all()


def test_nibble_order_of_four_bits():
    """Byte i holds dimension 2i in its LOW nibble (faiss Codec4bit), pinned by a row whose levels are all different."""
    vmin, vdiff = np.zeros(16, np.float32), np.full(16, 15.0, np.float32)
    row = np.arange(16, dtype=np.float32)[None, :]     # level d in dimension d
    assert sc.quantise(row, vmin, vdiff, 4).tolist() == [list(range(16))]
    codes = sc.encode(row, vmin, vdiff, 4)
    assert codes.shape == (1, 8) and codes[0].tolist() == [0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE]
    assert sc.unpack(codes, 4).tolist() == [list(range(16))]
    assert sc.pack(sc.unpack(codes, 4), 4).tolist() == codes.tolist()
    back = sc.decode(codes, vmin, vdiff, 4)
    assert np.array_equal(back[0], np.float32(15.0) * sc.levels(4))


def test_residuals_rows_and_range_of_an_ivf():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((500, 8)).astype(np.float32)
    cent = rng.standard_normal((4, 8)).astype(np.float32)
    list_of = rng.integers(0, 4, size=500)
    vmin, vdiff = sc.train_range(x, list_of, cent)
    r = x - cent[list_of]
    assert np.array_equal(vmin, r.min(0)) and np.array_equal(vdiff, r.max(0) - r.min(0))
    rows = rng.permutation(500)[:200]
    a = sc.encode(x, vmin, vdiff, 8, list_of, cent, rows)
    assert np.array_equal(a, sc.encode(r, vmin, vdiff, 8)[rows])
    assert not np.array_equal(a, sc.encode(x, vmin, vdiff, 8, rows=rows))


def test_both_chain_routes_of_the_reference_are_equal_bit_for_bit():
    """sq_expected takes the chains of a list from one oracle.dense.ip_topk_exact call (k = all rows, put back by row) and, for
    the smallest lists, from oracle.dense.pair_dot: the same bits, over decoded rows with repeated rows, a zero row and a zero query."""
    from oracle import dense as odense

    rng = np.random.default_rng(9)
    for dim, bits, n in ((16, 4, 70), (20, 8, 33), (768, 8, 40)):
        q, codes, vmin, vdiff, _, off, _, _, _ = sc.random_index(dim + bits, dim, bits, 4, 0, 1, 1, lens=[n])
        q[-1] = 0.0
        codes[n // 2] = codes[0]
        rows = sc.decode(codes, vmin, vdiff, bits)
        rows[1] = 0.0
        s, c = odense.ip_topk_exact(q, rows, n)
        back = np.empty_like(s)
        np.put_along_axis(back, c, s, axis=1)
        for i in range(len(q)):
            assert np.array_equal(back[i].view(np.uint32), odense.pair_dot(q[i], rows).view(np.uint32)), (dim, bits, i)
    # and through sq_expected itself: 70 rows x 4 queries on one list take the first route, 3 x 4 the second
    for n in (70, 3):
        q, codes, vmin, vdiff, bits, off, ids, _, bias = sc.random_index(n, 16, 8, 4, 0, 1, 1, lens=[n])
        probe = np.zeros((4, 1), np.int32)
        s, i = sc.sq_expected(q, codes, vmin, vdiff, bits, off, ids, probe, bias, n)
        rows = sc.decode(codes, vmin, vdiff, bits)
        for t in range(4):
            chain = odense.pair_dot(q[t], rows) + bias[t, 0]
            order = np.lexsort((ids, -chain))
            assert np.array_equal(i[t], ids[order]) and np.array_equal(s[t].view(np.uint32), chain[order].view(np.uint32))


@pytest.mark.parametrize("bits", [8, 4])
def test_sq_expected_agrees_with_float64(bits):
    """The reference, not the kernel: scores within the chain's rounding bound of the float64 inner product of the decoded rows
    (dim fmas and one add, each rounding at most 2^-24 of a partial sum bounded by the sum of absolute terms), the order the
    float64 order wherever float64 scores differ by more than that, the probe rules, padding."""
    q, codes, vmin, vdiff, _, off, ids, probe, bias = sc.random_index(5 + bits, 32, bits, 6, 400, 5, 3)
    probe[1, 1] = -1
    probe[2, 2] = 5                                   # past the last list
    probe[3, 1] = probe[3, 0]                         # a list named twice: the first slot's bias counts
    probe[4] = -1
    k = 60
    s, i = sc.sq_expected(q, codes, vmin, vdiff, bits, off, ids, probe, bias, k)
    assert s.dtype == np.float32 and i.dtype == np.int64 and (i[4] == -1).all() and (s[4] == -np.finfo(np.float32).max).all()
    row_of = np.argsort(ids)
    decoded = sc.decode(codes, vmin, vdiff, bits).astype(np.float64)
    for n in range(len(q)):
        slots = sc.clean_slots(probe[n], 5)
        if n == 3:
            assert [s_ for s_, _ in slots] == [0, 2]
        rows = np.concatenate([np.arange(off[l], off[l + 1]) for _, l in slots]) if slots else np.zeros(0, np.int64)
        b = np.concatenate([np.full(off[l + 1] - off[l], bias[n, s_], np.float64) for s_, l in slots]) if slots else np.zeros(0)
        exact = sc.float64_scores(q[n], codes[rows], vmin, vdiff, bits, 0.0) + b
        mag = np.abs(b) + (np.abs(decoded[rows]) * np.abs(q[n].astype(np.float64))).sum(1)
        bound = (32 + 1) * U * mag
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
