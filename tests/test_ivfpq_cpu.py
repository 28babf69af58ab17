"""Host side of the IVF-PQ index (mevi_amd/ivfpq.py, include/mevi_hip_ivfpq.h) without a GPU: the factory strings, the header
and its bindings, the workspace and tile arithmetic (monotone, capped, 0 outside every bound of the envelope), every documented
refusal with its status and message before anything is launched (the pointers handed over are null or fake), and the
reference of the GPU tests (tests/ivfpq_cases.py: adc_expected) against a float64 ADC."""
import os
import re

import numpy as np
import pytest

import ivfpq_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def test_parse_factory_table():
    from mevi_amd import ivf, ivfpq

    table = {"IVF8,PQ4": (8, 4, 8), "IVF100,PQ64": (100, 64, 8), "IVF4096,PQ64x8": (4096, 64, 8), "IVF16,PQ12x5": (16, 12, 5),
             "PQ64": (None, 64, 8), "PQ8x1": (None, 8, 1), " IVF8 , PQ4 ": (8, 4, 8), "PQ96x8": (None, 96, 8)}
    for text, want in table.items():
        assert ivfpq.parse_factory(text) == want, text
    for text in ("HNSW256", "IVF8,Flat", "PQ8x12", "OPQ16,PQ16", "Flat", "PQ8x0", "PQ8x9", "IVF8,PQ", "PQ", "IVF,PQ8", "IVF8,PQ8,Flat",
                 "PQ8x", "IVF8,PQ8x8x8", "IVF8_HNSW32,PQ8", "PQ8np", ""):
        assert ivfpq.parse_factory(text) is None, text
    assert ivf.parse_factory("IVF8,PQ4") is None                       # the IVF-Flat parser is not the one that takes it


def test_header_is_included_exported_and_bound(L):
    from mevi_amd import dense, hip

    assert '#include "mevi_hip_ivfpq.h"' in open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    raw = open(os.path.join(ROOT, "include", "mevi_hip_ivfpq.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mevi_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["mevi_ivfpq_scan_query_tile", "mevi_ivfpq_scan_topk_f32", "mevi_ivfpq_scan_workspace_bytes"]
    assert hip.exported_symbols("mevi_hip_ivfpq.h") == declared and not set(declared) & set(hip.exported_symbols())
    assert all(callable(getattr(L, n)) for n in declared)
    assert int(re.search(r"#define MEVI_IVFPQ_SCAN_ROW_BLOCK (\d+)", text).group(1)) == dense.IVFPQ_ROW_BLOCK
    for name in ("ivfpq_scan_topk", "ivfpq_scan_workspace_bytes", "ivfpq_scan_query_tile"):
        assert callable(getattr(dense, name))


#        nq, nprobe, k, dim, m, K, nlist, max_list_len
C2 = (6980, 16, 1000, 768, 64, 256, 100, 200000)


def test_workspace_and_tile_are_host_arithmetic_monotone_and_capped(L):
    from mevi_amd import dense

    f, tile = L.mevi_ivfpq_scan_workspace_bytes, L.mevi_ivfpq_scan_query_tile
    cap = dense.IVF_WORKSPACE_CAP
    assert 0 < f(*C2) <= cap and f(*C2) == dense.ivfpq_scan_workspace_bytes(*C2)
    # the tile: queries whose candidates fit 2 GiB, whose tables fit 128 MiB, at most 4096 and at most nq
    assert tile(*C2) == dense.ivfpq_scan_query_tile(*C2) == (2 << 30) // (16 * 200000 * 4)
    assert tile(6980, 1, 10, 16, 4, 16, 8, 1000) == 4096 and tile(33, 1, 10, 16, 4, 16, 8, 1000) == 33
    assert tile(6980, 1, 10, 768, 64, 256, 8, 1000) == (128 << 20) // (64 * 256 * 4) == 2048
    assert tile(6980, 1, 10, 768, 96, 256, 8, 1000) == (128 << 20) // (96 * 256 * 4) == 1365
    assert tile(20, 256, 4096, 16, 4, 16, 300, 262144) == 8              # the tiling case of the GPU tests: 8, 8, 4
    grids = {0: [1, 2, 31, 32, 33, 1365, 1366, 2048, 2049, 4096, 4097, 6980, 100000], 1: [1, 2, 3, 16, 255, 256], 2: [1, 10, 1000, 4096],
             5: [1, 2, 16, 200, 255, 256], 6: [1, 2, 100, 4096, 262144], 7: [0, 1, 1023, 1024, 1025, 5000, 200000, 2000000]}
    bases = (C2, (1, 1, 1, 16, 4, 1, 1, 1), (33, 3, 10, 48, 12, 200, 8, 3000), (5, 3, 100, 768, 96, 256, 10, 2000))
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
    # m and dim grow together (dim == m * dsub)
    for dsub in (4, 12):
        sizes = [f(6980, 4, 100, m * dsub, m, 256, 100, 50000) for m in range(4, 97, 4)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and max(sizes) <= cap
    assert f(1 << 40, 256, 4096, 96 * 8, 96, 256, 262144, (2 << 30) // (4 * 256)) <= cap      # the largest shape of the envelope
    assert f(1, 256, 4096, 96 * 8, 96, 256, 262144, (2 << 30) // (4 * 256)) > 0


def test_sizes_are_zero_just_outside_every_bound(L):
    inside = (8, 2, 10, 64, 16, 256, 8, 1000)
    assert L.mevi_ivfpq_scan_workspace_bytes(*inside) > 0 and L.mevi_ivfpq_scan_query_tile(*inside) == 8
    edges = {"nq 0": (0, 2, 10, 64, 16, 256, 8, 1000), "nprobe 0": (8, 0, 10, 64, 16, 256, 8, 1000),
             "nprobe 257": (8, 257, 10, 64, 16, 256, 8, 1000), "k 0": (8, 2, 0, 64, 16, 256, 8, 1000),
             "k 4097": (8, 2, 4097, 64, 16, 256, 8, 1000), "dim != m * dsub": (8, 2, 10, 68, 16, 256, 8, 1000),
             "dsub % 4": (8, 2, 10, 96, 16, 256, 8, 1000), "m % 4": (8, 2, 10, 72, 18, 256, 8, 1000), "m 0": (8, 2, 10, 64, 0, 256, 8, 1000),
             "m 2": (8, 2, 10, 64, 2, 256, 8, 1000), "m 100": (8, 2, 10, 800, 100, 16, 8, 1000), "K 0": (8, 2, 10, 64, 16, 0, 8, 1000),
             "K 257": (8, 2, 10, 64, 16, 257, 8, 1000), "nlist 0": (8, 2, 10, 64, 16, 256, 0, 1000),
             "nlist 262145": (8, 2, 10, 64, 16, 256, 262145, 1000), "max_list_len -1": (8, 2, 10, 64, 16, 256, 8, -1),
             "candidates": (8, 256, 10, 64, 16, 256, 8, (2 << 30) // (4 * 256) + 4)}
    for name, shape in edges.items():
        assert L.mevi_ivfpq_scan_workspace_bytes(*shape) == 0 and L.mevi_ivfpq_scan_query_tile(*shape) == 0, name
    # ... and the last shapes inside: 96 subspaces of 256 centroids are the 96 KiB table, 4 x 1 the smallest
    for shape in [(8, 256, 4096, 768, 96, 256, 262144, (2 << 30) // (4 * 256)), (1, 1, 1, 16, 4, 1, 1, 0)]:
        assert L.mevi_ivfpq_scan_workspace_bytes(*shape) > 0, shape


def test_refusals_come_before_any_launch(L):
    from mevi_amd import hip

    A = 1 << 20                                    # a fake, well-aligned device address: nothing may dereference it

    def call(q=A, nq=8, dim=64, book=A, m=16, K=256, codes=A, off=A, ids=A, nd=5000, nlist=8, longest=1000, probe=A, bias=A, nprobe=2,
             k=10, out_s=A, out_i=A, ws=A, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.mevi_ivfpq_scan_workspace_bytes(nq, nprobe, k, dim, m, K, nlist, longest)
        st = L.mevi_ivfpq_scan_topk_f32(q, nq, dim, book, m, K, codes, off, ids, nd, nlist, longest, probe, bias, nprobe, k, out_s, out_i,
                                        ws, ws_bytes, None)
        return st, L.mevi_last_error().decode()

    def refused(code, word, **kw):
        st, msg = call(**kw)
        assert st == code and word in msg and msg.startswith("ivfpq_scan:"), (kw, st, msg)
        with pytest.raises(hip.MeviHipError, match="ivfpq_scan"):
            hip.check(st, "mevi_ivfpq_scan_topk_f32")

    refused(UNSUPPORTED, "m=18", m=18, dim=72)
    refused(UNSUPPORTED, "m=2", m=2)
    refused(UNSUPPORTED, "m=100", m=100, dim=800, K=16)
    refused(UNSUPPORTED, "K=0", K=0)
    refused(UNSUPPORTED, "K=257", K=257)
    refused(UNSUPPORTED, "dim=68", dim=68)
    refused(UNSUPPORTED, "dim=96", dim=96)                  # dsub = 6
    refused(UNSUPPORTED, "k=0", k=0)
    refused(UNSUPPORTED, "k=4097", k=4097)
    refused(UNSUPPORTED, "nprobe=0", nprobe=0)
    refused(UNSUPPORTED, "nprobe=257", nprobe=257)
    refused(UNSUPPORTED, "32 bits", nd=1 << 31)
    refused(UNSUPPORTED, "nlist=262145", nlist=262145)
    refused(UNSUPPORTED, "max_list_len", nd=(1 << 31) - 1, longest=(2 << 30) // (4 * 256) + 4, nprobe=256)
    for name in ("q", "book", "codes", "off", "probe", "out_s", "out_i", "ws"):
        refused(INVALID, "null", **{name: None})
    for name, step in (("q", 8), ("book", 4), ("codes", 4), ("off", 4), ("ids", 4), ("out_i", 4), ("probe", 2), ("bias", 2), ("out_s", 2),
                       ("ws", 128)):
        refused(INVALID, "align", **{name: A + step})
    refused(INVALID, "align", m=12, dim=48, codes=A + 2)    # m % 16 != 0: rows are read as dwords
    refused(INVALID, "max_list_len", longest=5001)
    refused(INVALID, "nq=-1", nq=-1, ws_bytes=0)
    need = L.mevi_ivfpq_scan_workspace_bytes(8, 2, 10, 64, 16, 256, 8, 1000)
    refused(WORKSPACE, str(need), ws_bytes=need - 1)
    refused(WORKSPACE, str(need), ws_bytes=0)
    # what is optional: no row ids, no bias, dword-aligned codes when m % 16 != 0; no queries: nothing to do, whatever the pointers
    assert call(nq=0, q=None, ws=None, ws_bytes=0, ids=None, bias=None)[0] == 0
    assert call(nq=0, m=12, dim=48, codes=A + 4)[0] == 0


def test_routing_envelope_of_dense_search(L, monkeypatch):
    """`ivfpq.wanted`: which (string, shape) pairs dense.search serves with the index; the others keep the exact search."""
    from mevi_amd import ivfpq

    monkeypatch.delenv("MEVI_IVFPQ", raising=False)
    assert ivfpq.wanted("IVF8,PQ4", 1000, 16, 10) == (8, 4, 8) and ivfpq.wanted("PQ64", 8841823, 768, 1000) == (None, 64, 8)
    assert ivfpq.wanted("IVF100,PQ64", 8841823, 768, 1000) == (100, 64, 8) and ivfpq.wanted("PQ96", 5000, 768, 4096) == (None, 96, 8)
    assert ivfpq.wanted("IVF8,PQ5", 1000, 20, 10) is None               # m % 4 != 0
    assert ivfpq.wanted("IVF8,PQ4", 1000, 18, 10) is None               # dim % m != 0
    assert ivfpq.wanted("IVF8,PQ4", 1000, 24, 10) is None               # dsub % 4 != 0
    assert ivfpq.wanted("IVF8,PQ4", 255, 16, 10) is None                # fewer rows than K
    assert ivfpq.wanted("IVF8,PQ4x4", 255, 16, 10) == (8, 4, 4)
    assert ivfpq.wanted("IVF2000,PQ4", 1000, 16, 10) is None            # nlist > nd
    assert ivfpq.wanted("IVF8,PQ4", 1000, 16, 4097) is None             # topk > 4096
    assert ivfpq.wanted("PQ128", 5000, 1024, 10) is None                # m > 96
    assert ivfpq.wanted("HNSW32", 1000, 16, 10) is None and ivfpq.wanted("IVF8,Flat", 1000, 16, 10) is None
    monkeypatch.setenv("MEVI_IVFPQ", "exact")
    assert ivfpq.wanted("IVF8,PQ4", 1000, 16, 10) is None


def test_lookup_tables_are_pair_dot_bit_for_bit():
    """`luts` (one oracle call per subspace) against `luts_by_pair_dot` (the definition: oracle.dense.pair_dot per entry), with
    repeated centroids, a zero centroid, a zero query and K no power of two."""
    rng = np.random.default_rng(9)
    for dim, m, K, nq in ((16, 4, 16, 3), (48, 12, 200, 4), (96, 8, 1, 2), (768, 64, 256, 2)):
        q = rng.standard_normal((nq, dim)).astype(np.float32)
        book = rng.standard_normal((m, K, dim // m)).astype(np.float32)
        book[:, K // 2] = book[:, 0]
        book[0, K - 1] = 0.0
        q[-1] = 0.0
        a, b = pc.luts(q, book), pc.luts_by_pair_dot(q, book)
        assert a.shape == (nq, m, K) and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (dim, m, K)


def test_adc_expected_agrees_with_float64():
    """The reference, not the kernel: scores within a few ulp-sized steps of the float64 ADC (m adds + m chains of dsub fmas, each
    rounding at most half an ulp of a partial sum bounded by the sum of absolute terms), the order the float64 order wherever
    float64 scores differ by more than that, the probe rules, padding."""
    q, book, codes, off, ids, probe, bias = pc.random_index(5, 32, 8, 16, 6, 400, 5, 3)
    probe[1, 1] = -1
    probe[2, 2] = 5                                   # past the last list
    probe[3, 1] = probe[3, 0]                         # a list named twice: the first slot's bias counts
    probe[4] = -1
    k = 60
    s, i = pc.adc_expected(q, book, codes, off, ids, probe, bias, k)
    assert s.dtype == np.float32 and i.dtype == np.int64 and (i[4] == -1).all() and (s[4] == -np.finfo(np.float32).max).all()
    row_of = np.argsort(ids)
    for n in range(len(q)):
        slots = pc.clean_slots(probe[n], 5)
        if n == 3:
            assert [s_ for s_, _ in slots] == [0, 2]
        rows = np.concatenate([np.arange(off[l], off[l + 1]) for _, l in slots]) if slots else np.zeros(0, np.int64)
        b = np.concatenate([np.full(off[l + 1] - off[l], bias[n, s_], np.float64) for s_, l in slots]) if slots else np.zeros(0)
        exact = pc.adc_float64(q[n], book, codes[rows], 0.0) + b
        m, _, dsub = book.shape
        mag = np.abs(b) + sum((np.abs(book[j][codes[rows, j]].astype(np.float64)) * np.abs(q[n].reshape(m, dsub)[j].astype(np.float64))).sum(1)
                              for j in range(m))
        bound = (m + dsub + 1) * 2.0 ** -24 * mag      # every one of the m + dsub roundings on a row's path <= 2^-24 * (sum of |terms|)
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
