"""Every case of tests/ivf_cases.py reaches the path of csrc/ivf_scan.hip it is named for: proven from plan_geometry (the host's
and the plan kernel's arithmetic restated) and from the oracle's result alone, so that shrinking a shape below its edge
fails here, without a GPU.  tests/test_ivf_scan_edges_gpu.py runs the same cases through the kernels."""
import os

import numpy as np
import pytest

import ivf_cases as ic
from oracle import dense as odense

CASES = ([("tiles by query count", ic.tiles_by_query_count, ()), ("tiles by candidate cap", ic.tiles_by_candidate_cap, ()),
          ("item walk, many lists", ic.item_walk_many_lists, ()), ("item walk, long lists", ic.item_walk_long_lists, ())] +
         [(f"plan carry {n}", ic.plan_carry, (n,)) for n in (1024, 1025, 2049)] +
         [(f"pair and row edges {c}", ic.pair_and_row_edges, (c,)) for c in ic.EDGE_PAIR_COUNTS] +
         [(f"select k={k}", ic.select_k, (k,)) for k in ic.SELECT_KS] +
         [(f"select overflow k={k}", ic.select_overflow, (k,)) for k in (100, 2600)] +
         [("select crowded top", ic.select_crowded_top, ())] +
         [(f"ties {place} ids={given}", ic.ties, (place, given)) for place in ic.TIE_PLACES for given in (True, False)] +
         [(f"nothing to scan: {kind}", ic.nothing_to_scan, (kind,)) for kind in ("no probes", "empty lists", "normal")])


def _tile_of_the_library(case):
    from mevi_amd import dense

    nq, dim = case.q.shape
    return dense.ivf_scan_query_tile(nq, case.probe.shape[1], case.k, dim, case.nlist, case.max_list_len)


def test_constants_are_the_kernels():
    from mevi_amd import dense

    assert (ic.PAIR_TILE, ic.ROW_BLOCK) == (dense.IVF_PAIR_TILE, dense.IVF_ROW_BLOCK)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shared = open(os.path.join(root, "mevi_amd", "csrc", "list_scan.h")).read()      # the limits and grid rule of every list scan
    assert "SCAN_MAX_QT = 4096" in shared and "SCAN_CAND_CAP = (size_t)2 << 30" in shared and "if (grid > 768) grid = 768" in shared
    text = open(os.path.join(root, "mevi_amd", "csrc", "ivf_scan.hip")).read()
    assert "base += 1024" in text


@pytest.mark.parametrize("name,builder,args", CASES, ids=[c[0] for c in CASES])
def test_every_case_is_well_formed(name, builder, args):
    """The tile of plan_geometry is the library's, the lists respect max_list_len, ids are unique and inside [0, 2^32), and no
    expected score is inf or NaN."""
    case = builder(*args)
    g = ic.geometry(case)
    assert g.tile == _tile_of_the_library(case) > 0
    assert sum(g.tiles) == len(case.q) and all(t == g.tile for t in g.tiles[:-1]) and 0 < g.tiles[-1] <= g.tile
    assert ic.list_lengths(case).max() <= case.max_list_len <= len(case.d) and case.q.shape[1] % 4 == 0
    assert 1 <= case.k <= 4096 and 1 <= case.probe.shape[1] <= 256
    if case.row_ids is not None:
        assert len(np.unique(case.row_ids)) == len(case.d) and case.row_ids.min() >= 0 and case.row_ids.max() < 1 << 32
    s, i = ic.expected_of(builder, *args)
    assert np.isfinite(s).all() and np.isfinite(case.q).all() and np.isfinite(case.d).all()
    assert ((i == -1) == (s == -odense.FLT_MAX)).all()
    pad = (i == -1)
    assert (pad[:, :-1] <= pad[:, 1:]).all()                                      # padding only at the end of a row
    assert (s[:, :-1] >= s[:, 1:]).all()


def test_both_routes_to_the_expected_values_agree():
    """Subset ip_topk_exact (rows ascending, or every score + lexsort over the caller's ids) against one oracle_dot_f32 per row
    + lexsort: the same bits, with the original rows as ids and with shuffled ids."""
    case = ic.small_for_both_routes()
    shuffled = case._replace(row_ids=np.random.default_rng(1).permutation(len(case.d)).astype(np.int64) * 10_000_019 % (1 << 32))
    assert len(np.unique(shuffled.row_ids)) == len(case.d)
    for c in (case, shuffled):
        a, b = ic.expected(c), ic.expected_by_pair_dot(c)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
        assert (a[1] == -1).any() and (a[1][3] == -1).all()
        run = a[0][:, :-1] == a[0][:, 1:]
        assert (run & (a[1][:, :-1] >= 0)).any()                                       # ties are present ...
        assert (a[1][:, :-1][run & (a[1][:, 1:] >= 0)] < a[1][:, 1:][run & (a[1][:, 1:] >= 0)]).all()    # ... and ascend by id
    assert not np.array_equal(ic.expected(case)[1], ic.expected(shuffled)[1])


def test_clean_probe_keeps_the_first_slot_of_a_list():
    probe = np.array([[3, 3, -1, 7, 0, 3], [5, 4, 5, 4, 8, -2]])
    assert ic.clean_probe(probe, 8).tolist() == [[3, -1, -1, 7, 0, -1], [5, 4, -1, -1, -1, -1]]


def test_tiles_by_query_count():
    case = ic.tiles_by_query_count()
    g = ic.geometry(case)
    assert (g.tile, g.tiles) == (4096, [4096, 65])
    assert -(-g.tiles[1] // 64) < -(-g.tiles[0] // 64)                    # the second tile's bitmap rows are narrower
    assert not set(case.probe[4095]) & set(case.probe[4096]) and not set(case.probe[4094]) & set(case.probe[4097])
    want = ic.expected_of(ic.tiles_by_query_count)
    assert not np.array_equal(want[1][4095], want[1][4096]) and (want[1][4090:4161, 0] >= 0).sum() > 40
    assert case.nlist > ic.PLAN_CHUNK
    for t in range(2):                                                    # both tiles carry pairs and items over the 1024 seam
        assert g.pairs[t][:1024].sum() > 0 and g.pairs[t][1024:].sum() > 0 and g.items[t][1024:].sum() > 0
    assert g.item_totals[0] > ic.SCAN_GRID == g.grids[0] and g.grids[1] == 65 * 2 * 1


def test_tiles_by_candidate_cap():
    from mevi_amd import dense

    case = ic.tiles_by_candidate_cap()
    g = ic.geometry(case)
    assert (g.tile, g.tiles) == (8, [8, 8, 4]) and case.probe.shape == (20, 256) and case.max_list_len == len(case.d) == 262144
    clean = ic.clean_probe(case.probe, case.nlist)
    assert (clean[0] >= 0).sum() == 256 and all(250 <= (row >= 0).sum() < 256 for row in clean[1:])
    assert (case.probe[1:] == -1).any(1).all() and ((clean == -1) & (case.probe >= 0)).any(1)[1:].all()    # -1s and repeats
    lens = ic.list_lengths(case)
    assert 300 <= lens.min() and lens.max() <= 1500 and lens.max() > 1400
    assert (g.item_totals > ic.SCAN_GRID).all() and g.grids == [ic.SCAN_GRID] * 3
    ws = dense.ivf_scan_workspace_bytes(20, 256, case.k, 4, case.nlist, case.max_list_len)
    assert ic.CAND_CAP < ws <= dense.IVF_WORKSPACE_CAP                    # the whole candidate cap
    assert (ic.expected_of(ic.tiles_by_candidate_cap)[1] >= 0).all() and case.k == 4096


def _crossings(case):
    g = ic.geometry(case)
    assert len(g.tiles) == 1
    items = g.items[0]
    ranges = ic.walk_ranges(items, g.grids[0])
    assert sum(hi - lo for lo, hi, _, _ in ranges) == items.sum()
    return g, items, ranges


def test_item_walk_many_lists():
    case = ic.item_walk_many_lists()
    g, items, ranges = _crossings(case)
    lens = ic.list_lengths(case)
    assert case.nlist == 1100 and (lens == 0).sum() >= 220 and lens.max() <= 200 and (lens > ic.ROW_BLOCK).any()
    assert (g.pairs[0] > 0).all() and (items > 0).sum() > ic.SCAN_GRID == g.grids[0] and g.item_totals[0] > ic.SCAN_GRID
    assert any(b > a for _, _, a, b in ranges)                                           # a workgroup crosses into another list
    assert any(b > a + 1 and (items[a + 1:b] == 0).all() for _, _, a, b in ranges)       # ... over lists without items
    assert any(b > a + 20 for _, _, a, b in ranges)                                      # ... over a run of twenty
    want = ic.expected_of(ic.item_walk_many_lists)
    empty_probe = lens[case.probe[:, 0]] == 0
    assert empty_probe.sum() > 200 and ((want[1] == -1).all(1) == empty_probe).all()
    assert ((want[1] == -1).any(1) & ~empty_probe).any()                                 # lists shorter than k pad too


def test_item_walk_long_lists():
    case = ic.item_walk_long_lists()
    g, items, ranges = _crossings(case)
    lens = ic.list_lengths(case)
    assert case.nlist == 40 and lens.min() >= 1409 and lens.max() <= 1536 and (-(-lens // ic.ROW_BLOCK) == 12).all()
    assert {65, 128, 130} <= set(g.pairs[0].tolist()) and g.pairs[0].min() >= 65 and g.pairs[0].max() <= 130
    assert g.item_totals[0] > 900 and g.grids[0] == ic.SCAN_GRID
    assert any(hi - lo >= 2 and a == b for lo, hi, a, b in ranges) and any(b > a for _, _, a, b in ranges)
    # the lists are the index's own assignment given the centroids, by a wide margin
    cent = ic.item_walk_centroids()
    best = odense.ip_topk_exact(case.d, cent, 2)[0]
    assert (best[:, 0] - best[:, 1] > 1e-4).all()
    # the coarse call of the index: one list of 40 centroids that every query probes = many pair tiles of one list
    coarse = ic.plan_geometry(np.zeros((len(case.q), 1), np.int32), [40], 1, 40, len(case.q), 1)
    assert coarse.item_totals[0] == -(-len(case.q) // ic.PAIR_TILE) > 50


@pytest.mark.parametrize("nlist", [1024, 1025, 2049])
def test_plan_carry(nlist):
    case = ic.plan_carry(nlist)
    g = ic.geometry(case)
    assert len(g.tiles) == 1 and case.nlist == nlist
    pairs, items = g.pairs[0], g.items[0]
    assert pairs[1023] > 1 and items[1023] > 0 and pairs[:1020].sum() > 0
    assert (case.probe >= nlist).any() == (nlist < 2049)                 # lists past the end are named where they do not exist
    for seam in (1024, 2048):
        if nlist > seam:
            assert pairs[seam - 1] > 0 and pairs[seam] > 0 and items[seam - 1] > 0 and items[seam] > 0
            both = ((case.probe == seam - 1).any(1) & (case.probe == seam).any(1))
            assert both.any()                                            # one query on both sides of the boundary
    if nlist == 1024:                                                    # the totals at [nlist] are the carry alone
        assert len(pairs) % ic.PLAN_CHUNK == 0
    want = ic.expected_of(ic.plan_carry, nlist)
    assert (want[1][:, 0] >= 0).sum() > 150


def test_pair_and_row_edges():
    dims = set()
    for c in ic.EDGE_PAIR_COUNTS:
        case = ic.pair_and_row_edges(c)
        g = ic.geometry(case)
        assert ic.list_lengths(case).tolist() == list(ic.EDGE_LENS) and len(case.q) == c and case.k == 50
        assert (g.pairs[0] == c).all() and len(g.tiles) == 1
        assert all(sorted(row) == list(range(16)) for row in case.probe.tolist())
        dims.add(case.q.shape[1])
    assert dims == {4, 28, 36}
    assert ic.EDGE_PAIR_COUNTS == (31, 32, 33, 63, 64, 65, 127, 128, 129)
    assert ic.EDGE_LENS == (0, 1, 2, 3, 4, 5, 31, 32, 33, 127, 128, 129, 255, 256, 257, 600)


def test_select_k_around_the_total():
    assert ic.SELECT_KS == (1, 2, 3, 5, 3999, 4000, 4001)
    for k in ic.SELECT_KS:
        case = ic.select_k(k)
        lens = ic.list_lengths(case)
        assert len(case.d) == 5000 and all(lens[row].sum() == ic.SELECT_TOTAL for row in case.probe)
        want = ic.expected_of(ic.select_k, k)
        assert ((want[1] == -1).sum(1) == max(0, k - ic.SELECT_TOTAL)).all()      # padding exactly when k exceeds the total


def test_select_overflow_and_crowded_top():
    for k in (100, 2600):
        case = ic.select_overflow(k)
        want = ic.expected_of(ic.select_overflow, k)
        for query in range(2):
            scores = ic.probed_scores(case, query)
            width, bins = ic.linear_bins(scores)
            assert len(scores) == 5000 and np.isinf(width) and width.dtype == np.float32 and (bins == 0).all()
            assert np.isfinite(scores).all() and scores.max() > 2.9e38 and scores.min() < -2.9e38
            assert (want[0][query, -1] > 0) == (k == 100) and want[0][query, -1] != 0
    case = ic.select_crowded_top()
    scores = ic.probed_scores(case, 0)
    width, bins = ic.linear_bins(scores)
    assert 0 < width < odense.FLT_MAX and (bins == bins.max()).sum() > 10 * case.k and (bins >= bins.max() - 1).sum() == 3000
    top = scores[bins >= bins.max() - 1]
    assert len(np.unique(top)) == 4 and (1.0 - top.min()) <= 3 * 2.0 ** -24 and (scores == scores.max()).sum() > case.k
    want = ic.expected_of(ic.select_crowded_top)
    assert (want[0] == np.float32(1.0)).all() and (np.diff(want[1][0]) > 0).all()


@pytest.mark.parametrize("given_ids", [True, False])
def test_ties_are_cut_where_intended(given_ids):
    above, run_rows = ic.tie_layout(given_ids)
    first = ic.ties("first", given_ids)
    ids_of = np.arange(len(first.d)) if first.row_ids is None else first.row_ids
    run_ids = np.sort(ids_of[run_rows])
    assert len(run_ids) == ic.TIE_RUN and above >= 5
    if given_ids:
        for must in (0, (1 << 21) - 1, (1 << 21) + 1, 1 << 31, (1 << 32) - 1):
            assert must in run_ids
        low21, low10 = run_ids & ((1 << 21) - 1), run_ids & 1023
        assert (np.bincount(low21)[0x155555] >= 59)                              # differ only above bit 21
        mid = run_ids[(run_ids >> 21 == 0x5A5) & (low10 == 0x2AA)]
        assert len(mid) >= 59 and len(np.unique(mid >> 10)) == len(mid)          # differ only in bits 10..20
        assert (ids_of > 1 << 31).sum() > 500
    else:
        assert (np.diff(first.list_of) >= 0).all()                               # list-major already: the id is the row
    assert len(np.unique(first.list_of[run_rows])) == 3                          # the run lies in all three lists
    for place, need in zip(ic.TIE_PLACES, (ic.TIE_RUN, ic.TIE_RUN - 1, 1)):
        case = ic.ties(place, given_ids)
        s, i = ic.expected_of(ic.ties, place, given_ids)
        tie = s[0] == s[0, -1]
        assert case.k == above + need and tie.sum() == need and not tie[:above].any() and len(case.d) > case.k
        assert np.array_equal(i[0][tie], run_ids[:need])                         # the lowest ids of the run, ascending
        assert (need < ic.TIE_RUN) == (place != "last")                          # cut, except when the run is taken whole


def test_nothing_to_scan():
    for kind in ("no probes", "empty lists"):
        case = ic.nothing_to_scan(kind)
        g = ic.geometry(case)
        assert g.item_totals.tolist() == [0] and g.grids[0] > 0
        assert (g.pairs.sum() == 0) == (kind == "no probes")
        want = ic.expected_of(ic.nothing_to_scan, kind)
        assert (want[1] == -1).all() and (want[0] == -odense.FLT_MAX).all()
    assert (ic.list_lengths(ic.nothing_to_scan("empty lists"))[[0, 2, 4]] == 0).all()
    normal = ic.expected_of(ic.nothing_to_scan, "normal")
    assert (normal[1][:, 0] >= 0).sum() > 40 and (normal[1] == -1).any()
    for a in ("no probes", "empty lists"):
        assert np.array_equal(ic.nothing_to_scan(a).d, ic.nothing_to_scan("normal").d)
