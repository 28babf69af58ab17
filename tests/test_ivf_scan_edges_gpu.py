"""mevi_ivf_scan_topk_f32 at its edges: several query tiles (by query count and by the candidate cap, nprobe 256), workgroups that
walk many items across lists and over lists without items, more than 1024 lists in the plan kernel, every pair-tile and
row-block boundary, and the select kernel's corners (k around the total, an overflowing score range, a crowded top bin, cut and
uncut runs of equals under ids from all of [0, 2^32)).  The inputs are tests/ivf_cases.py; tests/test_ivf_cases_cpu.py proves
that each reaches its path.  Bar, as in tests/test_ivf_scan_gpu.py: ids identical, scores identical as uint32 bits."""
import numpy as np
import pytest
import torch

import ivf_cases as ic
from mevi_amd import dense, ivf

pytestmark = pytest.mark.gpu


def _to(cuda, a):
    return torch.from_numpy(np.array(a)).to(cuda)          # a copy: the cases' arrays are read-only


def _device(cuda, case, ids="given"):
    docs, off, row_ids = ic.list_major(case)
    return (_to(cuda, case.q), _to(cuda, docs), _to(cuda, off), None if ids is None else _to(cuda, row_ids), case.max_list_len,
            _to(cuda, case.probe), case.k)


def _same(got, want, rows=slice(None)):
    s, i = got
    torch.cuda.synchronize()
    np.testing.assert_array_equal(i.cpu().numpy()[rows], want[1][rows])
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32)[rows], want[0].view(np.uint32)[rows])


def _scan_equals_the_oracle(cuda, builder, *args, **kw):
    got = dense.ivf_scan_topk(*_device(cuda, builder(*args)), **kw)
    _same(got, ic.expected_of(builder, *args))
    return got


def _bytes(pair):
    return pair[0].cpu().numpy().tobytes(), pair[1].cpu().numpy().tobytes()


def test_two_tiles_by_query_count(cuda):
    """4096 + 65 queries: the second tile's pointer offsets and its narrower bitmap; the rows around the seam first."""
    case = ic.tiles_by_query_count()
    nq, dim = case.q.shape
    assert dense.ivf_scan_query_tile(nq, 2, case.k, dim, case.nlist, case.max_list_len) == 4096
    args, want = _device(cuda, case), ic.expected_of(ic.tiles_by_query_count)
    a = dense.ivf_scan_topk(*args)
    _same(a, want, slice(4090, 4161))
    _same(a, want)
    out = (torch.full((nq, case.k), 7.0, dtype=torch.float32, device=cuda), torch.full((nq, case.k), -7, dtype=torch.int64, device=cuda))
    ws = torch.full((dense.ivf_scan_workspace_bytes(nq, 2, case.k, dim, case.nlist, case.max_list_len),), 0xA5, dtype=torch.uint8, device=cuda)
    b = dense.ivf_scan_topk(*args, out=out, workspace=ws)
    torch.cuda.synchronize()
    assert b[0] is out[0] and b[1] is out[1] and _bytes(a) == _bytes(b)


def test_three_tiles_by_candidate_cap_at_nprobe_256(cuda):
    """max_list_len = nd = 262144 at nprobe 256: 8 queries a tile, tiles of 8, 8, 4 in the whole 2 GiB of candidates (allocated,
    not initialised); k = 4096 over some 220 000 probed rows a query."""
    case = ic.tiles_by_candidate_cap()
    nq, dim = case.q.shape
    assert dense.ivf_scan_query_tile(nq, 256, case.k, dim, case.nlist, case.max_list_len) == 8
    try:
        ws = torch.empty(dense.ivf_scan_workspace_bytes(nq, 256, case.k, dim, case.nlist, case.max_list_len), dtype=torch.uint8, device=cuda)
    except torch.OutOfMemoryError as e:
        pytest.skip(f"the device cannot give the {ic.CAND_CAP >> 20} MiB candidate workspace: {e}")
    _scan_equals_the_oracle(cuda, ic.tiles_by_candidate_cap, workspace=ws)


def test_workgroups_walk_across_lists_and_over_empty_ones(cuda):
    _scan_equals_the_oracle(cuda, ic.item_walk_many_lists)


def test_workgroups_walk_many_items_of_long_lists(cuda):
    """Directly, and through the index given the centroids (coarse call: one list, 61 pair tiles)."""
    case = ic.item_walk_long_lists()
    want = ic.expected_of(ic.item_walk_long_lists)
    _scan_equals_the_oracle(cuda, ic.item_walk_long_lists)
    index = ivf.IVFFlatIndex(_to(cuda, case.d), case.nlist, centroids=_to(cuda, ic.item_walk_centroids()))
    assert np.array_equal(index.list_of.cpu().numpy(), case.list_of) and index.scan_wanted(len(case.q), case.k, 1)
    _same(index.search_scan(_to(cuda, case.q), case.k, 1), want)


@pytest.mark.parametrize("nlist", [1024, 1025, 2049])
def test_plan_kernel_carries_over_1024_lists(cuda, nlist):
    _scan_equals_the_oracle(cuda, ic.plan_carry, nlist)


@pytest.mark.parametrize("c", ic.EDGE_PAIR_COUNTS)
def test_pair_tile_and_row_block_edges(cuda, c):
    _scan_equals_the_oracle(cuda, ic.pair_and_row_edges, c)


@pytest.mark.parametrize("k", ic.SELECT_KS)
def test_select_k_small_and_around_the_total(cuda, k):
    _scan_equals_the_oracle(cuda, ic.select_k, k)


@pytest.mark.parametrize("k", [100, 2600])
def test_select_when_the_score_range_overflows(cuda, k):
    _scan_equals_the_oracle(cuda, ic.select_overflow, k)


def test_select_with_a_crowded_top_bin(cuda):
    _scan_equals_the_oracle(cuda, ic.select_crowded_top)


@pytest.mark.parametrize("place", ic.TIE_PLACES)
def test_ties_under_ids_from_the_whole_32_bit_range(cuda, place):
    _scan_equals_the_oracle(cuda, ic.ties, place, True)


@pytest.mark.parametrize("place", ic.TIE_PLACES)
def test_ties_with_the_row_as_the_id(cuda, place):
    """row_ids = None; the case's rows are list-major already, so the id is the caller's row."""
    case = ic.ties(place, False)
    assert np.array_equal(ic.list_major(case)[2], np.arange(len(case.d)))
    _same(dense.ivf_scan_topk(*_device(cuda, case, ids=None)), ic.expected_of(ic.ties, place, False))


def test_nothing_to_scan_returns_padding_and_leaves_nothing_behind(cuda):
    """A table of -1 and a table of empty lists on a workspace a normal call has just used: all padding; the normal call that
    follows each is unchanged."""
    normal = ic.nothing_to_scan("normal")
    nq, dim = normal.q.shape
    ws = torch.full((dense.ivf_scan_workspace_bytes(nq, 3, normal.k, dim, normal.nlist, normal.max_list_len),), 0xA5, dtype=torch.uint8,
                    device=cuda)
    _scan_equals_the_oracle(cuda, ic.nothing_to_scan, "normal", workspace=ws)
    for kind in ("no probes", "empty lists"):
        s, i = _scan_equals_the_oracle(cuda, ic.nothing_to_scan, kind, workspace=ws)
        assert bool((i == -1).all()) and bool((s == -torch.finfo(torch.float32).max).all())
        _scan_equals_the_oracle(cuda, ic.nothing_to_scan, "normal", workspace=ws)
