"""Host side of the device fine stage (mevi_fine_topk_workspace_bytes / _query_tile / mevi_fine_topk_f32): the workspace query
is pure arithmetic and capped, every documented refusal comes back with its code and a message that names the argument before
anything is launched (the pointers handed over here are null or fake, so a launch would not go unnoticed), every case of
tests/fine_cases.py provably reaches the path it is named for, and oracle.dense.fine_stage reproduces its expected lists."""
import os
import re

import numpy as np
import pytest

import fine_cases as fc
from oracle import dense as odense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def test_python_constants_are_the_headers_and_the_kernels():
    from mevi_amd import fine, ops

    text = open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    assert "#define MEVI_FINE_TOPK_WORKSPACE_CAP (((size_t)1 << 30) + ((size_t)16 << 20))" in text
    assert ops.FINE_TOPK_WORKSPACE_CAP == (1 << 30) + (16 << 20)
    assert len(re.findall(r"\bmevi_fine_topk_[a-z0-9_]+\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))) == 3
    src = open(os.path.join(ROOT, "mevi_amd", "csrc", "fine_topk.hip")).read()
    assert f"FINE_SORT_MAX = {fc.SORT_MAX};" in src and ops.FINE_TOPK_SORT_MAX == fc.SORT_MAX == fine.MAX_SEGMENT
    assert f"FINE_MAX_QT = {fc.MAX_QUERY_TILE};" in src and "FINE_CAND_CAP = (size_t)1 << 30;" in src and fc.CAND_CAP == 1 << 30
    assert f"SCORE_THREADS = {fc.SCORE_CHUNK};" in src


def test_workspace_query_is_host_arithmetic_monotone_and_capped(L):
    from mevi_amd import ops

    f, tile = L.mevi_fine_topk_workspace_bytes, L.mevi_fine_topk_query_tile
    base = (6980, 10, 1000, 768, 5000)
    assert 0 < f(*base) <= ops.FINE_TOPK_WORKSPACE_CAP
    assert f(*base) == f(*base) == ops.fine_topk_workspace_bytes(*base)
    assert tile(*base) == ops.fine_topk_query_tile(*base) == 6980 == fc.query_tile(6980, 5000)
    assert tile(100000, 10, 10, 64, 100) == 16384 and tile(33, 1, 1, 4, 1) == 33
    assert tile(70, 10, 10, 8, fc.TILE_MAX_CAND) == 67 == fc.query_tile(70, fc.TILE_MAX_CAND)
    assert tile(5, 10, 10, 8, (1 << 27) - 3) == 1 and tile(5, 10, 10, 8, 1 << 27) == 1 and tile(5, 10, 10, 8, (1 << 27) + 1) == 0
    grids = [[1, 2, 31, 32, 33, 66, 67, 68, 6980, 16384, 16385, 100000, 1 << 40], [1, 2, 10, 127, 128], [1, 10, 1000, 4096],
             [4, 36, 64, 768, 1024, 4096], [1, 2, 3, 4, 5, 255, 256, 257, 16384, 16385, 100000, fc.TILE_MAX_CAND, 1 << 27]]
    for axis, values in enumerate(grids):
        for other in (base, (1, 1, 1, 4, 1), (70, 10, 10, 8, fc.TILE_MAX_CAND), (33, 128, 4096, 64, 3000)):
            sizes, tiles = [], []
            for v in values:
                shape = list(other)
                shape[axis] = v
                sizes.append(f(*shape))
                tiles.append(tile(*shape))
                assert tiles[-1] == fc.query_tile(shape[0], shape[4]), shape
            assert all(s > 0 for s in sizes) and all(t >= 1 for t in tiles), (axis, sizes, tiles)
            assert sizes == sorted(sizes), (axis, sizes)                    # never shrinks when an argument grows
            assert max(sizes) <= ops.FINE_TOPK_WORKSPACE_CAP
    assert f(1 << 40, 128, 4096, 4096, 1 << 27) <= ops.FINE_TOPK_WORKSPACE_CAP           # the largest shape of the envelope
    # outside the envelope: 0
    for shape in [(0, 10, 10, 64, 100), (8, 0, 10, 64, 100), (8, 129, 10, 64, 100), (8, 10, 0, 64, 100), (8, 10, 4097, 64, 100),
                  (8, 10, 10, 66, 100), (8, 10, 10, 0, 100), (8, 10, 10, 64, 0), (8, 10, 10, 64, (1 << 27) + 1), (8, 10, 10, 64, 1 << 62)]:
        assert f(*shape) == 0 and tile(*shape) == 0, shape


def test_refusals_come_before_any_launch(L):
    from mevi_amd import hip

    A = 1 << 20                                    # a fake, well-aligned device address: nothing may dereference it

    def call(q=A, ldq=64, per_beam=0, nq=8, R=10, emb=A, n_docs=5000, dim=64, keys=A, offs=A, docs=A, n_clusters=100, beam=A,
             max_cand=300, k=10, out_s=A, out_i=A, out_n=A, ws=A, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.mevi_fine_topk_workspace_bytes(nq, R, k, dim, max_cand)
        st = L.mevi_fine_topk_f32(q, ldq, per_beam, nq, R, emb, n_docs, dim, keys, offs, docs, n_clusters, beam, max_cand, k, out_s,
                                  out_i, out_n, ws, ws_bytes, None)
        return st, L.mevi_last_error().decode()

    def refused(code, word, **kw):
        st, msg = call(**kw)
        assert st == code and word in msg and msg.startswith("fine_topk:"), (kw, st, msg)
        with pytest.raises(hip.MeviHipError, match="fine_topk"):
            hip.check(st, "mevi_fine_topk_f32")

    # the shape refusals hold without queries too
    for nq in (8, 0):
        refused(UNSUPPORTED, "dim=66", dim=66, ldq=68, nq=nq)
        refused(UNSUPPORTED, "k=0", k=0, nq=nq)
        refused(UNSUPPORTED, "k=4097", k=4097, nq=nq)
        refused(UNSUPPORTED, "R=0", R=0, nq=nq)
        refused(UNSUPPORTED, "R=129", R=129, nq=nq)
        refused(UNSUPPORTED, "n_docs=2147483648", n_docs=1 << 31, nq=nq)
        refused(UNSUPPORTED, f"max_cand={(1 << 27) + 1}", max_cand=(1 << 27) + 1, nq=nq, ws_bytes=1 << 40)
        refused(INVALID, "max_cand=0", max_cand=0, nq=nq, ws_bytes=1 << 40)
        refused(INVALID, "max_cand=-5", max_cand=-5, nq=nq, ws_bytes=1 << 40)
        refused(INVALID, "ldq=60", ldq=60, nq=nq)
        refused(INVALID, "ldq=66", ldq=66, nq=nq)
    assert call(n_docs=(1 << 31) - 1, nq=0)[0] == 0
    for name in ("q", "emb", "beam", "out_s", "out_i", "out_n", "keys", "offs", "docs", "ws"):
        refused(INVALID, "null", **{name: None})
    for name, step in (("q", 8), ("emb", 4)):
        refused(INVALID, "16-byte", **{name: A + step})
    for name in ("keys", "offs", "docs", "beam", "out_i"):
        refused(INVALID, "8 bytes", **{name: A + 4})
    for name in ("out_s", "out_n"):
        refused(INVALID, "misaligned", **{name: A + 2})
    refused(INVALID, "256-byte", ws=A + 128)
    need = L.mevi_fine_topk_workspace_bytes(8, 10, 10, 64, 300)
    assert need > 0
    refused(WORKSPACE, str(need), ws_bytes=need - 1)
    refused(WORKSPACE, str(need), ws_bytes=0)
    # no queries: nothing to do, whatever the pointers; null CSR arrays are the index without clusters, not an error of their own
    assert call(nq=0, q=None, ws=None, ws_bytes=0, out_n=None)[0] == 0
    st, msg = call(keys=None, offs=None, docs=None, n_clusters=0, ws_bytes=need - 1)
    assert st == WORKSPACE and str(need) in msg


@pytest.mark.parametrize("entry", fc.ALL, ids=fc.case_id)
def test_case_reaches_the_path_it_is_named_for(L, entry):
    """Host arithmetic alone: the tile count, candidates above or below the LDS sort, the walk against max_cand."""
    builder, args = entry
    case = builder(*args)
    B, R = case.beam.shape
    dim = case.q.shape[1]
    tile = L.mevi_fine_topk_query_tile(B, R, case.k, dim, case.max_cand)
    assert tile == fc.query_tile(B, case.max_cand) >= 1
    assert 0 < L.mevi_fine_topk_workspace_bytes(B, R, case.k, dim, case.max_cand)
    assert (np.diff(case.keys) > 0).all() and len(case.offsets) == len(case.keys) + 1 and case.offsets[-1] == len(case.docs)
    walks = np.array([len(fc.walk(case, b)[0]) for b in range(B)])
    kept = fc.places(case)
    name = builder.__name__
    if name == "query_tiles":
        assert tile == 67 < B and -(-B // tile) == 2 and B % tile == 3           # two tiles, the second ragged
        assert walks.max() <= 60 and kept.max() <= fc.SORT_MAX
    else:
        assert tile == B                                                         # one tile
    if name == "short_bound":
        assert (walks > case.max_cand).sum() == 2 and (walks == case.max_cand).sum() == 1 and (walks < case.max_cand).sum() == 1
        cl = fc.clusters_of(case)
        first = [np.cumsum([0] + [len(cl.get(int(c), ())) for c in row]) for row in case.beam]
        assert first[0][1] < case.max_cand < first[0][2] < first[0][3]          # cut inside the second cluster, third dropped
    else:
        assert walks.max() <= case.max_cand
    if name == "bad_ids":
        assert ((case.docs < 0) | (case.docs >= len(case.emb))).sum() == 6
    else:
        assert case.docs.size == 0 or (case.docs.min() >= 0 and case.docs.max() < len(case.emb))
    large = name in ("above_lds_sort", "repeated_key_large") or (name in ("ties", "zero_query") and args[0])
    assert (kept.max() > fc.SORT_MAX) == large
    if large:
        assert case.max_cand >= kept[0] > fc.SORT_MAX and kept[0] > case.k       # the selection really has to cut
    if name == "above_lds_sort":
        assert kept[1] == 6000                                                   # both selections under one launch
    if name == "cluster_sizes":
        assert sorted(len(v) for v in fc.clusters_of(case).values()) == list(fc.EDGE_SIZES) and R == 10
        assert walks[0] == sum(fc.EDGE_SIZES) > 20 * fc.SCORE_CHUNK
    if name == "many_beams":
        assert R == 128 and set(np.diff(case.offsets)) == {1}
    if name == "k_edges":
        assert case.k - walks[0] == {"below": -1, "equal": 0, "above": 1, "far above": 4096 - 42}[args[0]]
    if name == "k4096_of_5000":
        assert case.k == 4096 and walks[0] == 5000
    if name == "no_clusters":
        assert len(case.keys) == 0 and walks.max() == 0
    if name == "one_cluster":
        assert len(case.keys) == 1
    if name == "minimal":
        assert (B, R, case.k, dim, len(case.docs)) == (1, 1, 1, 4, 1)
    if name == "key_kinds":
        beam, keys = case.beam, case.keys
        assert (beam < 0).any() and (beam == keys[0]).any() and (beam == keys[-1]).any() and (beam > keys[-1]).any()
        assert ((beam >= 0) & (beam < keys[0])).any() and walks[3] == 0
        assert set(beam[4][beam[4] >= 0]) == {keys[0]} and np.isin(beam[5], keys).sum() == 1 and keys[-1] in beam[5]
    if name == "repeated_key":
        assert all(len(set(row[row >= 0].tolist())) < (row >= 0).sum() for row in case.beam[:2])
    if name == "repeated_key_large":
        assert (case.beam[0] == case.beam[0, 0]).all() and case.k % 3 == 1


@pytest.mark.parametrize("entry", fc.ALL, ids=fc.case_id)
def test_oracle_fine_stage_reproduces_the_expected_lists(entry):
    """oracle.dense.fine_stage (pinned by the reference goldens) on every query: directly where the case is what it models (one
    embedding per query, the whole walk), else on the equivalent inputs -- per-beam embeddings: one call per beam, lists merged by
    (score desc, id asc); a walk cut by max_cand: the clusters cut the same way (keys are distinct in those rows); ids outside
    [0, N): the index without them."""
    builder, args = entry
    case = builder(*args)
    want_s, want_i, want_n = fc.expected_of(builder, *args)
    B, R = case.beam.shape
    n = len(case.emb)
    for b in range(B):
        cl = {(c,): d[(d >= 0) & (d < n)] for c, d in fc.clusters_of(case).items()}
        ndoc = sum(len(cl.get((int(c),), ())) for c in case.beam[b])
        room = case.max_cand                                     # entries of the walk still to come, ids outside [0, N) included
        if len(fc.walk(case, b)[0]) > case.max_cand:
            assert len(set(case.beam[b].tolist())) == R and builder.__name__ == "short_bound"
            cut = {}
            for c in case.beam[b]:
                if (int(c),) in cl:
                    cut[(int(c),)] = cl[(int(c),)][:room]
                    room -= len(cl[(int(c),)])
                    room = max(room, 0)
            cl = cut
        codes = [[int(c)] for c in case.beam[b]]
        if case.per_beam:
            parts = [odense.fine_stage(case.q[b * R + j], case.emb, cl, [codes[j]]) for j in range(R)]
            docs, sc = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
            order = np.lexsort((docs, -sc))
            docs, sc = docs[order], sc[order]
        else:
            docs, sc, got_n = odense.fine_stage(case.q[b], case.emb, cl, codes)
            assert got_n == len(docs)
        assert ndoc == want_n[b]
        m = min(case.k, len(docs))
        assert np.array_equal(docs[:m], want_i[b, :m]) and np.array_equal(sc[:m].view(np.uint32), want_s[b, :m].view(np.uint32))
        assert (want_i[b, m:] == -1).all() and (want_s[b, m:] == -odense.FLT_MAX).all()


def test_tie_cases_cut_their_run_of_equal_scores():
    for large in (False, True):
        case = fc.ties(large)
        want_s, want_i, _ = fc.expected_of(fc.ties, large)
        run = fc.tie_run_ids(large)
        assert len(run) == fc.TIE_RUN and case.k <= 4096
        tail = want_i[0, case.k - fc.TIE_RUN // 3:]
        assert np.array_equal(tail, run[:fc.TIE_RUN // 3]) and (want_s[0, case.k - fc.TIE_RUN // 3:] == want_s[0, -1]).all()
        assert want_s[0, case.k - fc.TIE_RUN // 3 - 1] > want_s[0, -1]
    for large in (False, True):
        want_s, want_i, want_n = fc.expected_of(fc.zero_query, large)
        assert (want_s.view(np.uint32) == 0).all() and np.array_equal(want_i[0], np.arange(40)) and want_n[0] == len(fc.zero_query(large).emb)
