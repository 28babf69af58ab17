"""Host side of the refine stage (mevi_amd/refine.py, include/mevi_hip_refine.h) without a GPU: the factory strings, the header and
its bindings, the workspace and tile arithmetic (monotone, capped, 0 just outside every bound), every documented refusal with its
status before anything is launched (the pointers handed over are null or fake), the routing envelope and k_factor, and the
reference of the GPU tests against a float64 ranking."""
import os
import re

import numpy as np
import pytest

import refine_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def test_parse_factory_table():
    from mevi_amd import ivfpq, opq, pqfs, refine, sq

    table = {"PQ8,RFlat": ("ivfpq", (None, 8, 8)), "IVF7,PQ8,RFlat": ("ivfpq", (7, 8, 8)), "PQ8x4,Refine(Flat)": ("ivfpq", (None, 8, 4)),
             "IVF4096,PQ64,RFlat": ("ivfpq", (4096, 64, 8)), "IVF7,PQ8x4fs,RFlat": ("pqfs", (7, 8)), "PQ64x4fs,Refine(Flat)": ("pqfs", (None, 64)),
             "OPQ8,IVF7,PQ8,RFlat": ("opq", (8, None, 7, 8, 8, False)), "OPQ64,PQ64x4fs,Refine(Flat)": ("opq", (64, None, None, 64, 4, True)),
             "OPQ8_32,PQ8,RFlat": ("opq", (8, 32, None, 8, 8, False)), "SQ8,RFlat": ("sq", (None, 8)), "IVF7,SQ4,Refine(Flat)": ("sq", (7, 4)),
             " IVF8 , PQ8 , RFlat ": ("ivfpq", (8, 8, 8)), "SQ4 ,  Refine( Flat ) ": ("sq", (None, 4)), "PQ8,\tRFlat": ("ivfpq", (None, 8, 8))}
    for text, want in table.items():
        assert refine.parse_factory(text) == want, text
        # the four inner parsers keep refusing the suffixed string: it is this module that takes the suffix off
        assert all(m.parse_factory(text) is None for m in (opq, ivfpq, pqfs, sq)), text
        inner, found = refine.split_factory(text)
        assert found and getattr({"ivfpq": ivfpq, "pqfs": pqfs, "opq": opq, "sq": sq}[want[0]], "parse_factory")(inner) == want[1]
    for text in ("PQ8", "IVF7,PQ8", "SQ8", "Flat", "PQ8,Refine(SQ8)", "PQ8,Refine(PQ8)", "IVF7,PQ8,Refine(PQ16x4)", "PQ8,Refine(SQfp16)",
                 "Flat,RFlat", "Flat,Refine(Flat)", "IVF7,Flat,RFlat", "IVF7,Flat,Refine(Flat)", "HNSW32,RFlat", "HNSW32,Flat,RFlat",
                 "HNSW32,Refine(Flat)", "PQ8,RFlat,RFlat", "PQ8,RFlat,Refine(Flat)", "PQ8,Refine(Flat),Refine(Flat)", "RFlat", ",RFlat",
                 "PQ8 RFlat", "PQ8,rflat", "PQ8,RFlat8", "PQ8,Refine(Flat", "PQ8,Refine()", "PQ8,RFlat,", "SQ6,RFlat", "PQ8x9,RFlat",
                 "PQ8x8fs,RFlat", "OPQ8,SQ8,RFlat", "PCA16,PQ8,RFlat", ""):
        assert refine.parse_factory(text) is None, text
    assert refine.split_factory("PQ8") == ("PQ8", False) and refine.split_factory("PQ8,Refine(SQ8)") == ("PQ8,Refine(SQ8)", False)


def test_header_is_included_exported_and_bound(L):
    from mevi_amd import dense, hip

    assert '#include "mevi_hip_refine.h"' in open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    raw = open(os.path.join(ROOT, "include", "mevi_hip_refine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mevi_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["mevi_refine_topk_f32", "mevi_refine_topk_query_tile", "mevi_refine_topk_set_score_body",
                        "mevi_refine_topk_workspace_bytes"]
    assert hip.exported_symbols("mevi_hip_refine.h") == declared and declared == sorted(hip._REFINE_SIGNATURES)
    for other in ("mevi_hip.h", "mevi_hip_fine_agg.h", "mevi_hip_attn_long.h", "mevi_hip_ivfpq.h", "mevi_hip_pqfs.h", "mevi_hip_sq.h",
                  "mevi_hip_opq.h", "mevi_hip_graph.h", "mevi_hip_graph_levels.h"):
        assert not set(declared) & set(hip.exported_symbols(other)), other
    assert all(callable(getattr(L, n)) for n in declared)
    # argument counts of the declarations = those of the signature table
    for name in declared:
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text, flags=re.S).group(1)
        assert len([a for a in args.split(",") if a.strip()]) == len(hip._REFINE_SIGNATURES[name][1]), name
    assert eval(re.search(r"#define MEVI_REFINE_TOPK_WORKSPACE_CAP \(\(size_t\)(\d+ << \d+)\)", text).group(1)) == dense.REFINE_WORKSPACE_CAP
    assert int(re.search(r"#define MEVI_REFINE_TOPK_MAX_CAND (\d+)", text).group(1)) == dense.REFINE_MAX_CAND == 16384
    assert L.mevi_abi_version() == 1
    for name in ("refine_topk", "refine_topk_workspace_bytes", "refine_topk_query_tile"):
        assert callable(getattr(dense, name))


#        nq, n_cand, k, dim
C2 = (6980, 4000, 1000, 768)


def test_workspace_and_tile_are_host_arithmetic_monotone_and_capped(L):
    from mevi_amd import dense

    f, tile = L.mevi_refine_topk_workspace_bytes, L.mevi_refine_topk_query_tile
    cap = dense.REFINE_WORKSPACE_CAP
    assert 0 < f(*C2) <= cap and f(*C2) == dense.refine_topk_workspace_bytes(*C2)
    # the tile: queries whose scores (4 bytes a candidate, the row rounded up to 4 candidates) fit the cap, at most 4096 and at most nq
    assert tile(*C2) == dense.refine_topk_query_tile(*C2) == cap // (4000 * 4)
    assert tile(6980, 1000, 1000, 768) == 4096 and tile(33, 1000, 10, 768) == 33 and f(33, 1000, 10, 768) == -(-33 * 4000 // 256) * 256
    assert f(1, 1, 1, 4) == 256 and f(3, 5, 1, 4) == 256                 # 3 rows of 8 candidates, rounded up to 256 bytes
    assert tile(1 << 40, 16384, 4096, 4096) == 512 and f(1 << 40, 16384, 4096, 4096) == cap
    assert tile(515, 16384, 4, 4) == 512                                 # the tiling case of the GPU tests: 512 + 3
    grids = {0: [1, 2, 31, 32, 33, 511, 512, 513, 2048, 4095, 4096, 4097, 6980, 100000], 1: [1, 2, 3, 4, 5, 63, 64, 65, 2047, 2048, 2049,
                                                                                             4000, 4096, 8191, 8193, 16383, 16384],
             2: [1, 10, 1000, 4096], 3: [4, 8, 32, 36, 100, 768, 4092, 4096]}
    for axis, values in grids.items():
        for other in (C2, (1, 1, 1, 4), (33, 100, 10, 96), (5000, 16384, 4096, 4096), (600, 9000, 10, 32)):
            sizes = []
            for v in values:
                shape = list(other)
                shape[axis] = v
                sizes.append(f(*shape))
            assert all(s > 0 for s in sizes), (axis, other, sizes)
            assert sizes == sorted(sizes), (axis, other, sizes)          # never shrinks when an argument grows
            assert max(sizes) <= cap


def test_sizes_are_zero_just_outside_every_bound(L):
    inside = (8, 100, 10, 64)
    assert L.mevi_refine_topk_workspace_bytes(*inside) > 0 and L.mevi_refine_topk_query_tile(*inside) == 8
    edges = {"nq 0": (0, 100, 10, 64), "nq -1": (-1, 100, 10, 64), "dim 0": (8, 100, 10, 0), "dim 5": (8, 100, 10, 5),
             "dim 4100": (8, 100, 10, 4100), "dim 2": (8, 100, 10, 2), "k 0": (8, 100, 0, 64), "k 4097": (8, 100, 4097, 64),
             "n_cand 0": (8, 0, 10, 64), "n_cand 16385": (8, 16385, 10, 64), "n_cand -1": (8, -1, 10, 64)}
    for name, shape in edges.items():
        assert L.mevi_refine_topk_workspace_bytes(*shape) == 0 and L.mevi_refine_topk_query_tile(*shape) == 0, name
    for shape in [(1, 1, 1, 4), (8, 16384, 4096, 4096), (8, 1, 4096, 4), (1 << 40, 16384, 1, 4096)]:     # the last shapes inside
        assert L.mevi_refine_topk_workspace_bytes(*shape) > 0, shape


def test_refusals_come_before_any_launch(L):
    from mevi_amd import hip

    A = 1 << 20                                    # a fake, well-aligned device address: nothing may dereference it

    def call(q=A, ldq=None, nq=8, docs=A, nd=5000, dim=64, cand=A, ld_cand=None, n_cand=100, k=10, out_s=A, out_i=A, out_n=A, ws=A,
             ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.mevi_refine_topk_workspace_bytes(nq, n_cand, k, dim)
        st = L.mevi_refine_topk_f32(q, dim if ldq is None else ldq, nq, docs, nd, dim, cand, n_cand if ld_cand is None else ld_cand,
                                    n_cand, k, out_s, out_i, out_n, ws, ws_bytes, None)
        return st, L.mevi_last_error().decode()

    def refused(code, word, **kw):
        st, msg = call(**kw)
        assert st == code and word in msg and msg.startswith("refine_topk:"), (kw, st, msg)
        with pytest.raises(hip.MeviHipError, match="refine_topk"):
            hip.check(st, "mevi_refine_topk_f32")

    for nq in (8, 0):                              # the shape is judged with and without queries
        refused(UNSUPPORTED, "dim=0", dim=0, nq=nq, ws_bytes=0)
        refused(UNSUPPORTED, "dim=5", dim=5, ldq=8, nq=nq, ws_bytes=0)
        refused(UNSUPPORTED, "dim=4100", dim=4100, nq=nq, ws_bytes=0)
        refused(UNSUPPORTED, "k=0", k=0, nq=nq, ws_bytes=0)
        refused(UNSUPPORTED, "k=4097", k=4097, nq=nq, ws_bytes=0)
        refused(UNSUPPORTED, "n_cand=0", n_cand=0, nq=nq, ws_bytes=0)
        refused(UNSUPPORTED, "n_cand=16385", n_cand=16385, nq=nq, ws_bytes=0)
        refused(UNSUPPORTED, "31 bits", nd=1 << 31, nq=nq)
        refused(INVALID, "ldq=60", ldq=60, nq=nq)
        refused(INVALID, "ldq=66", ldq=66, nq=nq)
        refused(INVALID, "ld_cand=99", ld_cand=99, nq=nq)
        refused(INVALID, "n_docs=-1", nd=-1, nq=nq)
        refused(INVALID, "n_cand=-1", n_cand=-1, nq=nq, ws_bytes=0)
        refused(INVALID, "k=-1", k=-1, nq=nq, ws_bytes=0)
        refused(INVALID, "dim=-4", dim=-4, nq=nq, ws_bytes=0)
    refused(INVALID, "nq=-1", nq=-1, ws_bytes=0)
    for name in ("q", "docs", "cand", "out_s", "out_i", "ws"):
        refused(INVALID, "null", **{name: None})
    for name, step in (("q", 8), ("docs", 4), ("cand", 4), ("out_i", 4), ("out_s", 2), ("out_n", 2), ("ws", 128)):
        refused(INVALID, "align", **{name: A + step})
    need = L.mevi_refine_topk_workspace_bytes(8, 100, 10, 64)
    assert need == -(-8 * 100 * 4 // 256) * 256
    refused(WORKSPACE, str(need), ws_bytes=need - 1)
    refused(WORKSPACE, str(need), ws_bytes=0)
    # what is optional: out_nvalid, docs of an empty corpus (checked before the workspace, which is then refused as too short: no
    # launch); no queries: nothing to do, whatever the pointers
    assert call(out_n=None, ws_bytes=0)[0] == WORKSPACE and call(docs=None, nd=0, ws_bytes=0)[0] == WORKSPACE
    assert call(nq=0, q=None, docs=None, cand=None, out_s=None, out_i=None, out_n=None, ws=None, ws_bytes=0)[0] == 0
    assert call(nq=0, q=A + 2, ws=A + 1)[0] == 0
    # larger strides are fine
    assert call(ldq=68, ld_cand=101, ws_bytes=0)[0] == WORKSPACE


def test_routing_envelope_and_k_factor(L, monkeypatch):
    """`refine.wanted`: which (string, shape) pairs dense.search serves with a RefineIndex; the others keep the exact search."""
    from mevi_amd import ivfpq, refine

    for name in ("MEVI_REFINE", "MEVI_REFINE_K_FACTOR", "MEVI_IVFPQ", "MEVI_PQFS", "MEVI_SQ", "MEVI_OPQ"):
        monkeypatch.delenv(name, raising=False)
    assert refine.wanted("IVF7,PQ8,RFlat", 3000, 32, 10) == ("ivfpq", (7, 8, 8))
    assert refine.wanted("PQ64,Refine(Flat)", 8841823, 768, 1000) == ("ivfpq", (None, 64, 8))
    assert refine.wanted("IVF7,PQ8x4fs,RFlat", 3000, 32, 10) == ("pqfs", (7, 8))
    assert refine.wanted("OPQ8_32,IVF7,PQ8,RFlat", 3000, 32, 10) == ("opq", (8, 7, 8, 8, False))     # opq.wanted's form: no <dout>
    assert refine.wanted("IVF7,SQ4,RFlat", 3000, 32, 10) == ("sq", (7, 4))
    assert refine.wanted("IVF7,PQ8", 3000, 32, 10) is None and refine.wanted("HNSW32,RFlat", 30000, 32, 10) is None
    assert refine.wanted("PQ8,Refine(SQ8)", 3000, 32, 10) is None and refine.wanted("Flat,RFlat", 3000, 32, 10) is None
    assert ivfpq.wanted("IVF7,PQ8,RFlat", 3000, 32, 10) is None                 # the inner family does not see the suffixed string
    # the inner family's own envelope, evaluated at k_base
    assert refine.wanted("PQ12,RFlat", 3000, 32, 10) is None                     # dim % m != 0
    assert refine.wanted("IVF4000,PQ8,RFlat", 3000, 32, 10) is None              # nlist > nd
    assert refine.wanted("OPQ8_16,PQ8,RFlat", 3000, 32, 10) is None              # a reducing rotation
    assert refine.wanted("PQ8,RFlat", 3000, 32, 4096) == ("ivfpq", (None, 8, 8)) and refine.wanted("PQ8,RFlat", 3000, 32, 4097) is None
    # k_factor: a float, below 1 is 1, k_base = int(k * k_factor); k_base 4096 is served, 4097 is not
    assert refine.default_k_factor() == 1.0 and refine.k_base(10) == 10
    for text, factor, k3 in (("0.5", 1.0, 3), ("2.5", 2.5, 7), ("4", 4.0, 12), ("1", 1.0, 3), ("-3", 1.0, 3), ("nan", 1.0, 3)):
        monkeypatch.setenv("MEVI_REFINE_K_FACTOR", text)
        assert refine.default_k_factor() == factor and refine.k_base(3) == k3, text
    assert refine.k_base(3, 2.5) == 7 and refine.k_base(3, 0.1) == 3 and refine.k_base(1000, 4) == 4000
    monkeypatch.setenv("MEVI_REFINE_K_FACTOR", "4")
    assert refine.wanted("PQ8,RFlat", 3000, 32, 1024) == ("ivfpq", (None, 8, 8))  # k_base 4096
    assert refine.wanted("PQ8,RFlat", 3000, 32, 1025) is None                    # k_base 4100
    monkeypatch.setenv("MEVI_REFINE_K_FACTOR", "4.004")
    assert refine.wanted("PQ8,RFlat", 3000, 32, 1023) == ("ivfpq", (None, 8, 8))  # int(4096.09) = 4096
    assert refine.wanted("PQ8,RFlat", 3000, 32, 1024) is None                    # int(4100.1) = 4100
    monkeypatch.delenv("MEVI_REFINE_K_FACTOR")
    monkeypatch.setenv("MEVI_IVFPQ", "exact")                                    # the inner family's switch refuses for the refine too
    assert refine.wanted("PQ8,RFlat", 3000, 32, 10) is None and refine.wanted("SQ8,RFlat", 3000, 32, 10) == ("sq", (None, 8))
    monkeypatch.delenv("MEVI_IVFPQ")
    monkeypatch.setenv("MEVI_REFINE", "exact")
    for text in ("IVF7,PQ8,RFlat", "PQ64,Refine(Flat)", "SQ8,RFlat", "OPQ8,PQ8,RFlat", "PQ8x4fs,RFlat"):
        assert refine.wanted(text, 3000, 32, 10) is None, text
    assert ivfpq.wanted("IVF7,PQ8", 3000, 32, 10) == (7, 8, 8)                   # the switch is this family's alone


def test_docstrings_name_the_family_and_is_trained_is_unchanged():
    import faiss_search
    from mevi_amd import dense, refine

    for text in ("PQ8,RFlat", "IVF8,PQ8x4fs,Refine(Flat)", "SQ8,RFlat", "OPQ8,PQ8,RFlat"):
        assert dense.is_trained_before_train(text) is False
    assert dense.is_trained_before_train("Flat,RFlat") is True and dense.is_trained_before_train("HNSW32,RFlat") is True
    for doc in (dense.search.__doc__, faiss_search.__doc__):
        assert "RFlat" in doc and "Refine(Flat)" in doc and "MEVI_REFINE_K_FACTOR" in doc and "MEVI_REFINE=exact" in doc
    assert "RFlat" in dense.is_trained_before_train.__doc__
    for word in ("Refine(<anything but Flat>)", "search_graph", "torchrun"):     # what is out of scope is said
        assert word in refine.__doc__, word


def test_refine_expected_agrees_with_float64():
    """The reference of the GPU tests, not the kernel: on data without near-ties the ids are those of a float64 ranking of the valid
    candidates, the scores within dim roundings of the float64 products, padding and counts as documented."""
    rng = np.random.default_rng(5)
    nd, dim, nq, n_cand, k = 500, 24, 6, 70, 80
    docs = rng.standard_normal((nd, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    cand = np.stack([rng.permutation(nd)[:n_cand] for _ in range(nq)]).astype(np.int64)
    cand[0, 3] = -1
    cand[1, -5:] = -1
    cand[2, 10] = nd
    cand[2, 11] = nd + 7
    cand[3, 20] = cand[3, 4]                          # a repeat: listed twice, side by side
    cand[4] = -1
    s, i, nv = rc.refine_expected(q, docs, cand, k)
    assert s.dtype == np.float32 and i.dtype == np.int64 and nv.dtype == np.int32 and s.shape == i.shape == (nq, k)
    assert nv.tolist() == [69, 65, 68, 70, 0, 70]
    exact = q.astype(np.float64) @ docs.astype(np.float64).T
    mag = np.abs(q.astype(np.float64)) @ np.abs(docs.astype(np.float64)).T
    for b in range(nq):
        valid = cand[b][(cand[b] >= 0) & (cand[b] < nd)]
        order = valid[np.lexsort((valid, -exact[b, valid]))]
        gaps = np.diff(np.unique(exact[b, valid]))
        assert len(gaps) == 0 or gaps.min() > 4 * dim * 2.0 ** -24 * mag[b].max()          # no near-ties: f32 and f64 rank alike
        n = min(k, len(valid))
        assert np.array_equal(i[b, :n], order[:n]) and (i[b, n:] == -1).all() and (s[b, n:] == -rc.FLT_MAX).all()
        assert (np.abs(s[b, :n].astype(np.float64) - exact[b, order[:n]]) <= dim * 2.0 ** -24 * mag[b, order[:n]]).all()
    at = np.flatnonzero(i[3] == cand[3, 4])
    assert len(at) == 2 and at[1] == at[0] + 1 and s[3, at[0]] == s[3, at[1]]
    s2, i2, _ = rc.refine_expected(q, docs, cand, 7)                                          # truncation keeps the head
    assert np.array_equal(i2, i[:, :7]) and np.array_equal(s2.view(np.uint32), s[:, :7].view(np.uint32))
