"""Host side of the device fine stage's merge and weight modes (mevi_fine_topk_agg_workspace_bytes / _query_tile /
mevi_fine_topk_agg_f32): every new refusal comes back with its code and a message that names the argument before anything is
launched (the pointers handed over are null or fake), the sizing functions are host arithmetic that equals the plain call's and
ends at the merge's 16384 places, the numpy restatement of tests/fine_agg_cases.py equals the oracle where no new mode is set,
and every case provably has the input condition it is named for."""
import os
import re

import numpy as np
import pytest

import fine_agg_cases as ac
import fine_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def test_python_constants_are_the_headers_and_the_kernels():
    from mevi_amd import fine, hip, ops
    from mevi_amd.build import build

    # the three entry points are declared in mevi_hip_fine_agg.h, which mevi_hip.h includes; each is exported and bound
    assert '#include "mevi_hip_fine_agg.h"' in open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mevi_hip_fine_agg.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mevi_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["mevi_fine_topk_agg_f32", "mevi_fine_topk_agg_query_tile", "mevi_fine_topk_agg_workspace_bytes"]
    assert hip.exported_symbols("mevi_hip_fine_agg.h") == declared and not set(declared) & set(hip.exported_symbols())
    build()
    for name in declared:
        assert getattr(hip.lib(), name).argtypes is not None, name
    src = open(os.path.join(ROOT, "mevi_amd", "csrc", "fine_topk.hip")).read()
    assert f"FINE_SMALL_MAX = {ac.SMALL_MAX};" in src and f"FINE_SORT_MAX = {ac.SORT_MAX};" in src
    assert ops.FINE_AGGREGATE == ac.AGG and ops.FINE_TOPK_SORT_MAX == ac.SORT_MAX == fine.MAX_SEGMENT


def test_sizing_equals_the_plain_call_and_ends_at_the_merge_envelope(L):
    from mevi_amd import ops

    f, tile = L.mevi_fine_topk_agg_workspace_bytes, L.mevi_fine_topk_agg_query_tile
    f0, tile0 = L.mevi_fine_topk_workspace_bytes, L.mevi_fine_topk_query_tile
    grids = [[1, 2, 33, 6980, 8192, 8195, 16385, 1 << 40], [1, 2, 10, 128], [1, 10, 1000, 4096], [4, 36, 768, 4096],
             [1, 2, 255, 2048, 2049, 16383, 16384]]
    above = [16385, 100000, fc.TILE_MAX_CAND, 1 << 27]
    bases = ((6980, 10, 1000, 768, 5000), (1, 1, 1, 4, 1), (33, 128, 4096, 64, 3000), (8195, 2, 4, 4, 16384))
    for axis, values in enumerate(grids):
        for other in bases:
            for agg in (0, 1, 2):
                sizes = []
                for v in values + (above if axis == 4 and agg == 0 else []):
                    shape = list(other)
                    shape[axis] = v
                    sizes.append(f(*shape, agg))
                    assert sizes[-1] == f0(*shape) > 0 and tile(*shape, agg) == tile0(*shape) >= 1, (shape, agg)
                assert sizes == sorted(sizes), (axis, agg, sizes)                 # never shrinks when an argument grows
    assert tile(ac.TILE_QUERIES, 2, 4, 4, ac.TILE_MAX_CAND, 1) == ac.TILE_QUERIES - 3 == fc.query_tile(ac.TILE_QUERIES, ac.TILE_MAX_CAND)
    # outside the envelope: 0 -- the plain call's envelope, an aggregate outside 0..2, a merge above 16384 places
    for shape in [(0, 10, 10, 64, 100), (8, 129, 10, 64, 100), (8, 10, 4097, 64, 100), (8, 10, 10, 66, 100), (8, 10, 10, 64, 0),
                  (8, 10, 10, 64, (1 << 27) + 1)]:
        for agg in (0, 1, 2):
            assert f(*shape, agg) == 0 and tile(*shape, agg) == 0, (shape, agg)
    for agg in (-1, 3, 100):
        assert f(8, 10, 10, 64, 100, agg) == 0 and tile(8, 10, 10, 64, 100, agg) == 0
    for max_cand in above:
        for agg in (1, 2):
            assert f(8, 10, 10, 64, max_cand, agg) == 0 and tile(8, 10, 10, 64, max_cand, agg) == 0
        assert f(8, 10, 10, 64, max_cand, 0) > 0
    assert ops.fine_topk_agg_workspace_bytes(8, 10, 10, 64, 16384, "add") == f0(8, 10, 10, 64, 16384)
    assert ops.fine_topk_agg_workspace_bytes(8, 10, 10, 64, 16385, "max") == 0 == ops.fine_topk_agg_query_tile(8, 10, 10, 64, 16385, "add")
    assert ops.fine_topk_agg_query_tile(8, 10, 10, 64, 16385) == 8 == ops.fine_topk_agg_query_tile(8, 10, 10, 64, 300, "max")


def test_refusals_come_before_any_launch(L):
    from mevi_amd import hip

    A = 1 << 20                                    # a fake, well-aligned device address: nothing may dereference it

    def call(q=A, ldq=64, per_beam=0, nq=8, R=10, emb=A, n_docs=5000, dim=64, keys=A, offs=A, docs=A, n_clusters=100, beam=A,
             max_cand=300, k=10, agg=1, w=A, dp=A, ratio=0.3, out_s=A, out_i=A, out_n=A, out_u=A, ws=A, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.mevi_fine_topk_workspace_bytes(nq, R, k, dim, max_cand)
        st = L.mevi_fine_topk_agg_f32(q, ldq, per_beam, nq, R, emb, n_docs, dim, keys, offs, docs, n_clusters, beam, max_cand, k, agg,
                                      w, dp, ratio, 1.0 - ratio, out_s, out_i, out_n, out_u, ws, ws_bytes, None)
        return st, L.mevi_last_error().decode()

    def refused(code, word, **kw):
        st, msg = call(**kw)
        assert st == code and word in msg and msg.startswith("fine_topk:"), (kw, st, msg)
        with pytest.raises(hip.MeviHipError, match="fine_topk"):
            hip.check(st, "mevi_fine_topk_agg_f32")

    for nq in (8, 0):                              # the shape refusals hold without queries too
        refused(INVALID, "aggregate=3", agg=3, nq=nq)
        refused(INVALID, "aggregate=-1", agg=-1, nq=nq)
        refused(INVALID, "doc_proba", w=None, nq=nq)
        refused(INVALID, "doc_proba", w=None, agg=0, nq=nq)
        for agg in (1, 2):
            refused(UNSUPPORTED, "max_cand=16385", max_cand=16385, agg=agg, nq=nq, ws_bytes=1 << 40)
            refused(UNSUPPORTED, f"max_cand={1 << 20}", max_cand=1 << 20, agg=agg, nq=nq, ws_bytes=1 << 40)
        # the plain call's refusals, through the new entry point
        refused(UNSUPPORTED, "dim=66", dim=66, ldq=68, nq=nq)
        refused(UNSUPPORTED, "k=4097", k=4097, nq=nq)
        refused(UNSUPPORTED, "R=129", R=129, nq=nq)
        refused(UNSUPPORTED, f"max_cand={(1 << 27) + 1}", max_cand=(1 << 27) + 1, agg=0, nq=nq, ws_bytes=1 << 40)
        refused(INVALID, "max_cand=0", max_cand=0, nq=nq)
        refused(INVALID, "ldq=60", ldq=60, nq=nq)
    for agg in (1, 2):
        refused(INVALID, "out_nuniq", out_u=None, agg=agg)
    for name in ("w", "dp", "out_u"):
        refused(INVALID, "4 bytes", **{name: A + 2})
        refused(INVALID, "misaligned", **{name: A + 1})
    for name in ("q", "emb", "beam", "out_s", "out_i", "out_n", "ws"):
        refused(INVALID, "null", **{name: None})
    need = L.mevi_fine_topk_agg_workspace_bytes(8, 10, 10, 64, 300, 1)
    assert need > 0
    refused(WORKSPACE, str(need), ws_bytes=need - 1)
    # what is no refusal: the workspace check is the last one, so these reach it and nothing before them objects
    for kw in (dict(agg=0, out_u=None), dict(agg=0, w=None, dp=None, out_u=None), dict(dp=None), dict(max_cand=16384),
               dict(agg=0, max_cand=16385)):
        st, msg = call(ws_bytes=0, **kw)
        assert st == WORKSPACE and "needed" in msg, (kw, st, msg)
    assert call(nq=0, q=None, ws=None, ws_bytes=0, out_n=None, out_u=None)[0] == 0


def test_restatement_without_a_mode_equals_the_plain_cases_expected_values():
    """fine_agg_cases.expected with no merge and no weights on every plain case: fine_cases.expected, which tests/
    test_fine_topk_cpu.py holds against oracle.dense.fine_stage."""
    for builder, args in fc.ALL:
        got = ac.expected(ac._agg(builder(*args)))
        want = fc.expected_of(builder, *args)
        assert got[3] is None
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1]), builder.__name__
        assert np.array_equal(got[2], want[2])


@pytest.mark.parametrize("entry", ac.ALL, ids=ac.case_id)
def test_case_reaches_the_path_it_is_named_for(L, entry):
    builder, args = entry
    case = builder(*args)
    base = case.base
    B, R = base.beam.shape
    name = builder.__name__
    places = fc.places(base)
    tile = L.mevi_fine_topk_agg_query_tile(B, R, base.k, base.q.shape[1], base.max_cand, ac.AGG[case.aggregate])
    assert tile >= 1 and L.mevi_fine_topk_agg_workspace_bytes(B, R, base.k, base.q.shape[1], base.max_cand, ac.AGG[case.aggregate]) > 0
    want = ac.expected_of(builder, *args)
    # which selection launch takes the longest query: 256 threads up to 2048 places, 1024 threads up to 16384 (the LDS sort),
    # above that the radix selection, which only the unmerged modes have
    reach = "small" if places.max() <= ac.SMALL_MAX else "sort" if places.max() <= ac.SORT_MAX else "radix"
    assert reach == {"full_sort": "sort", "weights_above_lds_sort": "radix"}.get(name, "sort" if name == "seams" and args[0] else "small")
    if case.aggregate:
        assert base.max_cand <= ac.SORT_MAX
        for b in range(min(B, 16)):
            docs = ac.occurrences(case, b)[0]
            assert want[3][b] == len(set(docs.tolist()))
    if name == "query_tiles":
        assert tile == B - 3 and B == ac.TILE_QUERIES and places.max() <= 6
    else:
        assert tile == B
    if name == "minimal":
        assert (B, R, base.q.shape[1], len(base.docs)) == (1, 2, 4, 2) and want[3][0] == 1 and want[1][0].tolist() == [0, -1]
    if name == "longest_run":
        docs, slot, sc, _ = ac.occurrences(case, 0)
        assert R == 128 and base.per_beam and (docs == 0).sum() == 128 and len(set(slot[docs == 0].tolist())) == 128
        assert set(np.diff(base.offsets).tolist()) <= {1, 2, 3} and len(set(sc[docs == 0].view(np.uint32).tolist())) == 128
        if case.aggregate == "add":                                  # the order of the adds shows
            fwd = ac.fold(docs, sc, "add")[1][0]
            rev = ac.fold(docs, sc, "add", reverse=True)[1][0]
            assert fwd.view(np.uint32) != rev.view(np.uint32), (fwd, rev)
    if name == "seams":
        ids = ac.sorted_ids(case, 0)
        for seam in ac.SEAMS[args[0]]:
            assert len(set(ids[seam - 2:seam + 2].tolist())) == 1 and ids[seam - 3] != ids[seam - 2] and ids[seam + 1] != ids[seam + 2]
        assert len(ids) == places[0] and ids[-1] == ids[-3] != ids[-4]
    if name == "k_edges":
        assert places[0] == 55 and want[3][0] == ac.K_EDGE_UNIQUE
        assert base.k - want[3][0] == {"below": -1, "equal": 0, "above": 1, "far above": 4096 - 45}[args[0]]
        assert (want[1][0, :min(base.k, 45)] >= 0).all() and (want[1][0, 45:] == -1).all()
    if name == "full_sort":
        assert places[0] == ac.SORT_MAX == base.max_cand and want[3][0] == 12288
    if name == "ties":
        lo, hi = ac.TIE_IDS
        row = want[1][0].tolist()
        at = row.index(lo)
        assert row[at + 1] == hi and want[0][0, at].view(np.uint32) == want[0][0, at + 1].view(np.uint32)
        docs, _, sc, _ = ac.occurrences(case, 0)
        assert (docs == lo).sum() == 2 == (docs == hi).sum()
    if name == "negative_max":
        assert (ac.occurrences(case, 0)[2] < 0).all() and (want[0][0, :want[3][0]] < 0).all() and want[3][0] == 9
    if name == "minus_zero_add":
        docs, _, sc, _ = ac.occurrences(case, 0)
        assert (docs == 2).sum() == 1 and sc[docs == 2].view(np.uint32)[0] == 0x80000000
        assert want[0][0, want[1][0].tolist().index(2)].view(np.uint32) == 0
    if name == "repeated_key":
        assert all(len(set(row[row >= 0].tolist())) < (row >= 0).sum() for row in base.beam[:2])
    if name == "cut_between":
        whole = fc.walk(base, 0)[0]
        assert len(whole) == 15 > base.max_cand == 13 and whole[13] == 5 and (whole[:13] == 5).sum() == 1 and (whole[:13] == 3).sum() == 2
        assert want[2][0] == 15 and want[3][0] == 12
    if name == "bad_ids":
        assert ((base.docs < 0) | (base.docs >= len(base.emb))).sum() == 5 and want[3].tolist() == [3, 3]
    if name == "weights_above_lds_sort":
        assert case.aggregate is None and (case.weights < 0).all() and places[0] == 18000 > base.k
    if name == "blend":
        docs, _, plain, _ = ac.occurrences(case._replace(weights=None, doc_proba=None), 0)     # q.d alone
        r, omr = ac.blend_terms(case)
        apart = (r * case.doc_proba[docs]).astype(np.float32) + (omr * plain).astype(np.float32)
        fused = (np.float64(r) * case.doc_proba[docs].astype(np.float64) + np.float64(omr) * plain.astype(np.float64)).astype(np.float32)
        assert (apart.view(np.uint32) != fused.view(np.uint32)).any()            # a contracted blend would show
        assert r == np.float32(0.3) and omr == np.float32(0.7)
