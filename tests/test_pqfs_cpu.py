"""Host side of the 4-bit fast-scan PQ index (mevi_amd/pqfs.py, include/mevi_hip_pqfs.h) without a GPU: the factory strings, the
header and its bindings, the workspace and tile arithmetic (monotone, capped, 0 outside every bound of the envelope), every
documented refusal with its status and message before anything is launched (the pointers handed over are null or fake), the
routing envelope, the numpy packer of the GPU tests and their reference over unpacked codes against a float64 ADC."""
import os
import re

import numpy as np
import pytest

import ivfpq_cases as pc
import pqfs_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def test_parse_factory_table():
    from mevi_amd import ivf, ivfpq, pqfs, sq

    table = {"PQ8x4fs": (None, 8), "PQ64x4fs": (None, 64), "IVF100,PQ64x4fs": (100, 64), "IVF4096,PQ96x4fs": (4096, 96),
             " IVF8 , PQ8x4fs ": (8, 8), "PQ12x4fs": (None, 12), "IVF1,PQ2x4fs": (1, 2)}
    for text, want in table.items():
        assert pqfs.parse_factory(text) == want, text
        assert ivfpq.parse_factory(text) is None and sq.parse_factory(text) is None and ivf.parse_factory(text) is None, text
    for text in ("PQ8x8fs", "PQ8x4fsr", "PQ8x4fs_64", "PQ8fs", "PQ8x4", "PQ8", "IVF8,PQ8x4", "IVF8,PQ8", "PQx4fs", "IVF,PQ8x4fs",
                 "IVF8,PQ8x4fs,RFlat", "IVF8,PQ8x4fs,Refine(Flat)", "OPQ8,PQ8x4fs", "PQ8x4FS", "PQ8 x4fs", "IVF8_HNSW32,PQ8x4fs", "Flat",
                 "SQ4", "HNSW32", "PQ8x5fs", "PQ-8x4fs", ""):
        assert pqfs.parse_factory(text) is None, text
    assert ivfpq.parse_factory("PQ8x4") == (None, 8, 4)                 # the byte-code index keeps its strings


def test_header_is_included_exported_and_bound(L):
    from mevi_amd import dense, hip

    assert '#include "mevi_hip_pqfs.h"' in open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    raw = open(os.path.join(ROOT, "include", "mevi_hip_pqfs.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mevi_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["mevi_pq4_pack", "mevi_pqfs_scan_query_tile", "mevi_pqfs_scan_topk_f32", "mevi_pqfs_scan_workspace_bytes"]
    assert hip.exported_symbols("mevi_hip_pqfs.h") == declared and not set(declared) & set(hip.exported_symbols())
    assert not set(declared) & set(hip.exported_symbols("mevi_hip_ivfpq.h"))
    assert all(callable(getattr(L, n)) for n in declared)
    assert int(re.search(r"#define MEVI_PQFS_SCAN_ROW_BLOCK (\d+)", text).group(1)) == dense.PQFS_ROW_BLOCK
    assert L.mevi_abi_version() == 1
    for name in ("pq4_pack", "pqfs_scan_topk", "pqfs_scan_workspace_bytes", "pqfs_scan_query_tile"):
        assert callable(getattr(dense, name))


#        nq, nprobe, k, dim, m, nlist, max_list_len
C2 = (6980, 16, 1000, 768, 64, 100, 200000)


def test_workspace_and_tile_are_host_arithmetic_monotone_and_capped(L):
    from mevi_amd import dense

    f, tile = L.mevi_pqfs_scan_workspace_bytes, L.mevi_pqfs_scan_query_tile
    cap = dense.IVF_WORKSPACE_CAP
    assert 0 < f(*C2) <= cap and f(*C2) == dense.pqfs_scan_workspace_bytes(*C2)
    # the tile: queries whose candidates fit 2 GiB, at most 4096 and at most nq
    assert tile(*C2) == dense.pqfs_scan_query_tile(*C2) == (2 << 30) // (16 * 200000 * 4)
    assert tile(6980, 1, 10, 32, 8, 8, 1000) == 4096 and tile(33, 1, 10, 32, 8, 8, 1000) == 33
    assert tile(6980, 1, 10, 768, 96, 8, 1000) == 4096
    assert tile(20, 256, 4096, 32, 8, 300, 262144) == 8                  # the tiling case of the GPU tests: 8, 8, 4
    grids = {0: [1, 2, 31, 32, 33, 2048, 2049, 4096, 4097, 6980, 100000], 1: [1, 2, 3, 16, 255, 256], 2: [1, 10, 1000, 4096],
             5: [1, 2, 100, 4096, 262144], 6: [0, 1, 2047, 2048, 2049, 5000, 200000, 2000000]}
    bases = (C2, (1, 1, 1, 32, 8, 1, 1), (33, 3, 10, 96, 24, 8, 3000), (5, 3, 100, 768, 96, 10, 2000))
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
        sizes = [f(6980, 4, 100, m * dsub, m, 100, 50000) for m in range(8, 97, 8)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and max(sizes) <= cap
    assert f(1 << 40, 256, 4096, 96 * 8, 96, 262144, (2 << 30) // (4 * 256)) <= cap          # the largest shape of the envelope
    assert f(1, 256, 4096, 96 * 8, 96, 262144, (2 << 30) // (4 * 256)) > 0


def test_sizes_are_zero_just_outside_every_bound(L):
    inside = (8, 2, 10, 64, 16, 8, 1000)
    assert L.mevi_pqfs_scan_workspace_bytes(*inside) > 0 and L.mevi_pqfs_scan_query_tile(*inside) == 8
    edges = {"nq 0": (0, 2, 10, 64, 16, 8, 1000), "nprobe 0": (8, 0, 10, 64, 16, 8, 1000), "nprobe 257": (8, 257, 10, 64, 16, 8, 1000),
             "k 0": (8, 2, 0, 64, 16, 8, 1000), "k 4097": (8, 2, 4097, 64, 16, 8, 1000), "dim != m * dsub": (8, 2, 10, 68, 16, 8, 1000),
             "dsub % 4": (8, 2, 10, 96, 16, 8, 1000), "m 12": (8, 2, 10, 48, 12, 8, 1000), "m 4": (8, 2, 10, 16, 4, 8, 1000),
             "m 0": (8, 2, 10, 64, 0, 8, 1000), "m 100": (8, 2, 10, 400, 100, 8, 1000), "m 104": (8, 2, 10, 416, 104, 8, 1000),
             "nlist 0": (8, 2, 10, 64, 16, 0, 1000), "nlist 262145": (8, 2, 10, 64, 16, 262145, 1000),
             "max_list_len -1": (8, 2, 10, 64, 16, 8, -1), "candidates": (8, 256, 10, 64, 16, 8, (2 << 30) // (4 * 256) + 4)}
    for name, shape in edges.items():
        assert L.mevi_pqfs_scan_workspace_bytes(*shape) == 0 and L.mevi_pqfs_scan_query_tile(*shape) == 0, name
    # ... and the last shapes inside: 96 and 8 subspaces, every other argument at its bound
    for shape in [(8, 256, 4096, 768, 96, 262144, (2 << 30) // (4 * 256)), (1, 1, 1, 32, 8, 1, 0), (1, 1, 1, 256, 64, 1, 1),
                  (1, 1, 1, 288, 72, 1, 1)]:
        assert L.mevi_pqfs_scan_workspace_bytes(*shape) > 0, shape


def test_scan_refusals_come_before_any_launch(L):
    from mevi_amd import hip

    A = 1 << 20                                    # a fake, well-aligned device address: nothing may dereference it

    def call(q=A, nq=8, dim=64, book=A, m=16, codes=A, off=A, ids=A, nd=5000, nlist=8, longest=1000, probe=A, bias=A, nprobe=2, k=10,
             out_s=A, out_i=A, ws=A, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.mevi_pqfs_scan_workspace_bytes(nq, nprobe, k, dim, m, nlist, longest)
        st = L.mevi_pqfs_scan_topk_f32(q, nq, dim, book, m, codes, off, ids, nd, nlist, longest, probe, bias, nprobe, k, out_s, out_i, ws,
                                       ws_bytes, None)
        return st, L.mevi_last_error().decode()

    def refused(code, word, **kw):
        st, msg = call(**kw)
        assert st == code and word in msg and msg.startswith("pqfs_scan:"), (kw, st, msg)
        with pytest.raises(hip.MeviHipError, match="pqfs_scan"):
            hip.check(st, "mevi_pqfs_scan_topk_f32")

    refused(UNSUPPORTED, "m=12", m=12, dim=48)
    refused(UNSUPPORTED, "m=4", m=4)
    refused(UNSUPPORTED, "m=100", m=100, dim=400)
    refused(UNSUPPORTED, "m=104", m=104, dim=416)
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
    for name, step in (("q", 8), ("book", 4), ("codes", 2), ("off", 4), ("ids", 4), ("out_i", 4), ("probe", 2), ("bias", 2), ("out_s", 2),
                       ("ws", 128)):
        refused(INVALID, "align", **{name: A + step})
    refused(INVALID, "align", m=32, dim=128, codes=A + 4)   # m % 32 == 0: rows are read as 16-byte words
    refused(INVALID, "align", m=64, dim=256, codes=A + 8)
    refused(INVALID, "max_list_len", longest=5001)
    refused(INVALID, "nq=-1", nq=-1, ws_bytes=0)
    refused(INVALID, "nd=-1", nd=-1, longest=0)
    need = L.mevi_pqfs_scan_workspace_bytes(8, 2, 10, 64, 16, 8, 1000)
    refused(WORKSPACE, str(need), ws_bytes=need - 1)
    refused(WORKSPACE, str(need), ws_bytes=0)
    # what is optional: no row ids, no bias, dword-aligned rows when m % 32 != 0; no queries: nothing to do, whatever the pointers
    assert call(nq=0, q=None, ws=None, ws_bytes=0, ids=None, bias=None)[0] == 0
    assert call(nq=0, m=16, codes=A + 4)[0] == 0 and call(nq=0, m=24, dim=96, codes=A + 12)[0] == 0


def test_pack_refusals_come_before_any_launch(L):
    A = 1 << 20

    def call(codes=A, n=10, m=16, packed=A + 4096):
        st = L.mevi_pq4_pack(codes, n, m, packed, None)
        return st, L.mevi_last_error().decode()

    for code, word, kw in ((INVALID, "n=-1", dict(n=-1)), (UNSUPPORTED, "m=12", dict(m=12)), (UNSUPPORTED, "m=4", dict(m=4)),
                           (UNSUPPORTED, "m=104", dict(m=104)), (UNSUPPORTED, "m=0", dict(m=0)), (INVALID, "null", dict(codes=None)),
                           (INVALID, "null", dict(packed=None)), (INVALID, "align", dict(codes=A + 2)),
                           (INVALID, "align", dict(packed=A + 4097))):
        st, msg = call(**kw)
        assert st == code and word in msg and msg.startswith("pq4_pack:"), (kw, st, msg)
    assert call(n=0, codes=None, packed=None)[0] == 0                   # nothing to pack: no launch


def test_routing_envelope_of_dense_search(L, monkeypatch):
    """`pqfs.wanted`: which (string, shape) pairs dense.search serves with the index; the others keep the exact search."""
    from mevi_amd import ivfpq, pqfs

    monkeypatch.delenv("MEVI_PQFS", raising=False)
    monkeypatch.delenv("MEVI_IVFPQ", raising=False)
    assert pqfs.wanted("IVF8,PQ8x4fs", 1000, 32, 10) == (8, 8) and pqfs.wanted("PQ64x4fs", 8841823, 768, 1000) == (None, 64)
    assert pqfs.wanted("IVF100,PQ64x4fs", 8841823, 768, 1000) == (100, 64) and pqfs.wanted("PQ96x4fs", 5000, 768, 4096) == (None, 96)
    assert pqfs.wanted("PQ12x4fs", 1000, 48, 10) is None                # m % 8 != 0
    assert pqfs.wanted("PQ4x4fs", 1000, 16, 10) is None                 # m < 8
    assert pqfs.wanted("IVF8,PQ8x4fs", 1000, 36, 10) is None            # dim % m != 0
    assert pqfs.wanted("IVF8,PQ8x4fs", 1000, 48, 10) is None            # dsub % 4 != 0
    assert pqfs.wanted("IVF8,PQ8x4fs", 15, 32, 10) is None              # fewer rows than 16 centroids
    assert pqfs.wanted("IVF8,PQ8x4fs", 16, 32, 10) == (8, 8)
    assert pqfs.wanted("IVF2000,PQ8x4fs", 1000, 32, 10) is None         # nlist > nd
    assert pqfs.wanted("IVF0,PQ8x4fs", 1000, 32, 10) is None
    assert pqfs.wanted("IVF8,PQ8x4fs", 10000, 32, 5000) is None         # topk > 4096
    assert pqfs.wanted("PQ128x4fs", 5000, 1024, 10) is None             # m > 96
    assert pqfs.wanted("PQ8x4", 1000, 32, 10) is None and pqfs.wanted("IVF8,Flat", 1000, 32, 10) is None
    assert ivfpq.wanted("PQ8x4fs", 1000, 32, 10) is None and ivfpq.wanted("PQ8x4", 1000, 32, 10) == (None, 8, 4)
    monkeypatch.setenv("MEVI_PQFS", "exact")
    assert pqfs.wanted("IVF8,PQ8x4fs", 1000, 32, 10) is None and pqfs.wanted("PQ64x4fs", 8841823, 768, 1000) is None
    assert ivfpq.wanted("PQ8x4", 1000, 32, 10) == (None, 8, 4)          # the switch is this family's alone


def test_is_trained_before_train_and_docstrings_name_the_family():
    import faiss_search
    from mevi_amd import dense

    assert dense.is_trained_before_train("PQ8x4fs") is False and dense.is_trained_before_train("IVF8,PQ8x4fs") is False
    assert "x4fs" in dense.search.__doc__ and "MEVI_PQFS" in dense.search.__doc__
    assert "x4fs" in faiss_search.__doc__ and "MEVI_PQFS" in faiss_search.__doc__


def test_numpy_pack_round_trip_and_nibble_convention():
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 16, size=(257, 24)).astype(np.uint8)
    packed = fc.pack(codes)
    assert packed.shape == (257, 12) and packed.dtype == np.uint8
    assert np.array_equal(fc.unpack(packed), codes)
    assert np.array_equal(fc.pack(fc.unpack(packed)), packed)
    one = fc.pack(np.array([[1, 2, 3, 4, 5, 6, 7, 15]], np.uint8))
    assert one.tolist() == [[0x21, 0x43, 0x65, 0xF7]]                   # code 2t low, code 2t + 1 high
    assert np.array_equal(fc.pack(codes | 0xF0), packed)                 # only the low 4 bits of an input byte are kept
    anyb = rng.integers(0, 256, size=(50, 8)).astype(np.uint8)
    assert np.array_equal(fc.unpack(fc.pack(anyb)), anyb & 15)
    assert np.array_equal(fc.unpack_swapped(packed)[:, 0::2], codes[:, 1::2])
    assert fc.pack(np.zeros((0, 8), np.uint8)).shape == (0, 4)


def test_adc_expected_on_unpacked_codes_agrees_with_float64():
    """The reference of the GPU tests, not the kernel: adc_expected with K = 16 over unpack(pack(codes)) within the rounding of its
    m adds and m chains of dsub fmas (each at most 2^-24 of the sum of absolute terms), sorted, ties by id, probe rules, padding."""
    q, book, codes, off, ids, probe, bias = pc.random_index(6, 32, 8, 16, 6, 400, 5, 3)
    codes = fc.unpack(fc.pack(codes))
    probe[1, 1] = -1
    probe[2, 2] = 5                                   # past the last list
    probe[3, 1] = probe[3, 0]                         # a list named twice: the first slot's bias counts
    probe[4] = -1
    k = 60
    s, i = pc.adc_expected(q, book, codes, off, ids, probe, bias, k)
    assert s.dtype == np.float32 and i.dtype == np.int64 and (i[4] == -1).all() and (s[4] == -np.finfo(np.float32).max).all()
    row_of = np.argsort(ids)
    m, _, dsub = book.shape
    for n in range(len(q)):
        slots = pc.clean_slots(probe[n], 5)
        rows = np.concatenate([np.arange(off[l], off[l + 1]) for _, l in slots]) if slots else np.zeros(0, np.int64)
        b = np.concatenate([np.full(off[l + 1] - off[l], bias[n, s_], np.float64) for s_, l in slots]) if slots else np.zeros(0)
        exact = pc.adc_float64(q[n], book, codes[rows], 0.0) + b
        mag = np.abs(b) + sum((np.abs(book[j][codes[rows, j]].astype(np.float64)) * np.abs(q[n].reshape(m, dsub)[j].astype(np.float64))).sum(1)
                              for j in range(m))
        bound = (m + dsub + 1) * 2.0 ** -24 * mag
        found = i[n][i[n] >= 0]
        assert len(found) == min(k, len(rows)) and len(set(found.tolist())) == len(found)
        where = {int(r): t for t, r in enumerate(rows)}
        at = np.array([where[int(row_of[d])] for d in found], np.int64)
        assert (np.abs(s[n][:len(found)].astype(np.float64) - exact[at]) <= bound[at]).all()
        assert (np.diff(s[n][:len(found)]) <= 0).all()
        ties = np.flatnonzero(np.diff(s[n][:len(found)]) == 0)
        assert (found[ties] < found[ties + 1]).all()
        if len(rows) > k:                             # nothing left out beats the last one kept by more than both bounds
            out = np.setdiff1d(np.arange(len(rows)), at)
            assert (exact[out] - bound[out] <= exact[at[-1]] + bound[at[-1]]).all()
