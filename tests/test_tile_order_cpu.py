"""The ticketed tile walk of the persistent f16 filter (csrc/mfma_pp.h: walk_range, sweep_order), checked through the library's
own host entry point mevi_ip_filter_tile_walk -- the same functions the kernel calls.

Label g = blockIdx & 7 owns a contiguous, item-balanced piece of one order of all (pair, query tile) items and hands it out in
ticket order.  Checked here: the eight pieces cover every item exactly once and differ in length by at most one item, and any
32 consecutive tickets -- the tiles in flight on one XCD -- touch few distinct operand slabs (pair + query tiles).
"""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def walk(L, n_a, n_b, g):
    n = L.mevi_ip_filter_tile_walk(n_a, n_b, g, None, None)
    assert n >= 0
    a = np.empty(max(n, 1), dtype=np.int32)
    b = np.empty(max(n, 1), dtype=np.int32)
    assert L.mevi_ip_filter_tile_walk(n_a, n_b, g, a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)) == n
    return a[:n].astype(np.int64), b[:n].astype(np.int64)


SHAPES = [(n_a, n_b) for n_a in (1, 2, 3, 7, 8, 9, 27, 48, 135, 378, 1061, 21637) for n_b in (1, 2, 3, 5, 7, 8, 9, 16, 27, 28, 31, 33)]


@pytest.mark.parametrize("n_a,n_b", SHAPES)
def test_labels_cover_every_item_once_and_balanced(L, n_a, n_b):
    seen = np.zeros((n_a, n_b), dtype=np.int64)
    lens = []
    for g in range(8):
        a, b = walk(L, n_a, n_b, g)
        lens.append(len(a))
        if len(a):
            assert a.min() >= 0 and a.max() < n_a and b.min() >= 0 and b.max() < n_b
            np.add.at(seen, (a, b), 1)
    assert (seen == 1).all()
    assert max(lens) - min(lens) <= 1


def test_bad_arguments_are_refused(L):
    assert L.mevi_ip_filter_tile_walk(0, 28, 0, None, None) == -1
    assert L.mevi_ip_filter_tile_walk(10, 28, 8, None, None) == -1
    assert L.mevi_ip_filter_tile_walk(1 << 20, 1 << 12, 0, None, None) == -1


def _window_slabs(a, b, win=32):
    """Distinct pair + query tiles of every window of `win` consecutive tickets."""
    return np.array([len(set(a[s:s + win].tolist())) + len(set(b[s:s + win].tolist())) for s in range(max(len(a) - win, 0) + 1)])


@pytest.mark.parametrize("n_a,n_b", [(21637, 28), (8648, 28), (4320, 27), (3200, 32), (2664, 9), (776, 4), (8000, 1)])
def test_windows_of_32_tickets_share_their_slabs(L, n_a, n_b):
    nc = (n_b + 7) >> 3
    widths = [n_b // nc + (c < n_b % nc) for c in range(nc)]
    ends = np.cumsum(widths) * n_a                       # first item (of the whole order) past each column
    for g in (0, 3, 7):
        a, b = walk(L, n_a, n_b, g)
        base = sum(L.mevi_ip_filter_tile_walk(n_a, n_b, h, None, None) for h in range(g))   # the label's first item
        slabs = _window_slabs(a, b)
        first = base + np.arange(len(slabs))
        col_first = np.searchsorted(ends, first, side="right")
        col_last = np.searchsorted(ends, first + 31, side="right")
        for c, w in enumerate(widths):                   # inside a column: its w query tiles + the pair tiles 32 tickets span
            inside = slabs[(col_first == c) & (col_last == c)]
            assert (inside <= w + -(-32 // w) + 1).all()
        # a window across a column's turn re-uses the pair tiles just fetched (serpentine): two columns' query tiles at most
        assert (slabs <= 2 * max(widths) + -(-32 // min(widths)) + 1).all()
        if min(widths) >= 7:   # e.g. the C2 search (28 query tiles: 4 columns of 7): 12-13 of the 64 slab requests of 32 tiles
            assert slabs.mean() <= 13.0
            assert (slabs <= 13).mean() >= 0.99
