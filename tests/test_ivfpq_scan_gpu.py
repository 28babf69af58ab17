"""The ADC list scan (mevi_ivfpq_scan_topk_f32 through dense.ivfpq_scan_topk) against tests/ivfpq_cases.py: adc_expected, which is
built from oracle calls only.  Bar: ids identical, scores identical as uint32 bits.  Shapes are the smallest that reach each path:
both code-load widths (m % 16), K = 256 and K known at run time, the 96 KiB table, several row blocks, several query tiles."""
import functools

import numpy as np
import pytest
import torch

import ivfpq_cases as pc
from mevi_amd import dense

pytestmark = pytest.mark.gpu

RB = dense.IVFPQ_ROW_BLOCK
FLT_MAX = np.finfo(np.float32).max


def _dev(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a)).to(cuda)          # a copy: shared cases are read-only


def _run(cuda, q, book, codes, off, ids, probe, bias, k, max_list_len=None, **kw):
    longest = int(np.diff(off).max()) if max_list_len is None else max_list_len
    return dense.ivfpq_scan_topk(_dev(cuda, q), _dev(cuda, book), _dev(cuda, codes), _dev(cuda, off), _dev(cuda, ids), longest,
                                 _dev(cuda, probe), _dev(cuda, bias), k, **kw)


def _same(got, want):
    s, i = got
    torch.cuda.synchronize()
    np.testing.assert_array_equal(i.cpu().numpy(), want[1])
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), want[0].view(np.uint32))


def _check(cuda, args, k, max_list_len=None, **kw):
    want = pc.adc_expected(*args, k, max_list_len=max_list_len)
    got = _run(cuda, *args, k, max_list_len=max_list_len, **kw)
    _same(got, want)
    return got, want


@pytest.mark.parametrize("dim,m,K,nq,nd,nlist,nprobe,k", [
    (16, 4, 16, 1, 300, 4, 1, 10),
    (16, 4, 1, 3, 100, 2, 2, 5),            # one centroid: every code is 0
    (48, 12, 200, 33, 3000, 8, 3, 1000),    # m % 16 != 0 (dword code loads), K no power of two
    (80, 20, 256, 65, 5000, 8, 8, 4096),    # eight draws of eight lists: repeats, some 3300 probed rows a query: padding
    (768, 64, 256, 257, 3000, 10, 1, 10),   # the C2 index shape: 16-byte code loads, a 64 KiB table
    (768, 96, 256, 5, 2000, 10, 3, 100),    # the 96 KiB table (dynamic LDS above 64 KiB)
    (64, 16, 100, 33, 1500, 6, 2, 50),      # 16-byte code loads with K != 256: codes clamped to K - 1 at run time
])
def test_scan_equals_adc_expected_over_shapes(cuda, dim, m, K, nq, nd, nlist, nprobe, k):
    args = pc.random_index(dim * 3 + m + nq, dim, m, K, nq, nd, nlist, nprobe, repeats=k == 4096)
    _, want = _check(cuda, args, k)
    if k == 4096:
        assert (want[1][:, -1] == -1).sum() > 30 and (want[1][:, 0] >= 0).all()     # the case does pad


def test_padding_when_k_exceeds_the_probed_rows(cuda):
    """(80, 20, 256) again with fewer rows than k = 4096: every query's tail is -FLT_MAX / -1."""
    args = pc.random_index(7, 80, 20, 256, 65, 3000, 8, 8)
    _, want = _check(cuda, args, 4096)
    assert (want[1][:, 3000:] == -1).all() and (want[1][:, :3000] >= 0).all() and (want[0][:, 3000:] == -FLT_MAX).all()


@pytest.mark.parametrize("m,K", [(16, 256), (8, 32)])
def test_flat_pq_one_list_no_bias_no_row_ids(cuda, m, K):
    """IndexPQ: one list, probe_score NULL (bias +0), row_ids NULL (the id is the row); 2 * RB + 77 rows = three row blocks."""
    q, book, codes, off, _, _, _ = pc.random_index(11, 4 * m, m, K, 9, 0, 1, 1, lens=[2 * RB + 77])
    probe = np.zeros((9, 1), np.int32)
    _check(cuda, (q, book, codes, off, None, probe, None), 100)


def test_probe_edges_then_a_normal_call_on_the_same_workspace(cuda):
    """-1 entries, entries >= nlist, a list named twice whose slots carry DIFFERENT biases (the first wins), empty lists, a table of
    -1 (all padding), each followed by a normal call on the same workspace."""
    lens = [0, 50, 0, 700, RB + 5, 30]
    q, book, codes, off, ids, _, _ = pc.random_index(13, 32, 8, 64, 40, 0, len(lens), 4, lens=lens)
    rng = np.random.default_rng(14)
    nq, nlist, k = len(q), len(lens), 60
    normal = np.stack([rng.permutation(nlist)[:4] for _ in range(nq)]).astype(np.int32)
    bias = rng.standard_normal((nq, 4)).astype(np.float32)
    edges = normal.copy()
    edges[::3, 1] = -1
    edges[1::5, 2] = nlist                            # past the last list
    edges[2::7, 0] = np.iinfo(np.int32).min
    edges[::4, 3] = edges[::4, 0]                     # the same list twice, under another bias
    assert (bias[::4, 3] != bias[::4, 0]).all()
    edges[7] = -1                                     # a query that probes nothing
    edges[8] = 3                                      # one list in all four slots
    edges[9] = [0, 2, 0, 2]                           # only empty lists
    ws = torch.full((dense.ivfpq_scan_workspace_bytes(nq, 4, k, 32, 8, 64, nlist, max(lens)),), 0xA5, dtype=torch.uint8, device=cuda)
    first, want_normal = _check(cuda, (q, book, codes, off, ids, normal, bias), k, workspace=ws)
    _, want = _check(cuda, (q, book, codes, off, ids, edges, bias), k, workspace=ws)
    assert (want[1][7] == -1).all() and (want[1][9] == -1).all() and (want[1][8] >= 0).all()
    # the repeated list counted once and with the first slot's bias: the second slot's bias would have given other scores
    swapped = bias.copy()
    swapped[::4, 0], swapped[::4, 3] = bias[::4, 3], bias[::4, 0]
    other = pc.adc_expected(q, book, codes, off, ids, edges, swapped, k)
    assert not np.array_equal(other[0][::4], want[0][::4])
    _check(cuda, (q, book, codes, off, ids, normal, bias), k, workspace=ws)
    nothing = np.full((nq, 4), -1, np.int32)
    (s, i), _ = _check(cuda, (q, book, codes, off, ids, nothing, bias), k, workspace=ws)
    assert bool((i == -1).all()) and bool((s == -FLT_MAX).all())
    again, _ = _check(cuda, (q, book, codes, off, ids, normal, bias), k, workspace=ws)
    assert again[0].cpu().numpy().tobytes() == want_normal[0].tobytes() and again[1].cpu().numpy().tobytes() == want_normal[1].tobytes()


def test_row_block_edges_under_a_larger_bound(cuda):
    """Lists of 0, 1, RB - 1, RB, RB + 1 and 2 RB + 1 rows, every query probing all of them in its own slot order, with
    max_list_len above the longest list; then a bound BELOW the longest lists: they are clamped, never overrun."""
    lens = [0, 1, RB - 1, RB, RB + 1, 2 * RB + 1]
    q, book, codes, off, ids, probe, bias = pc.random_index(15, 16, 4, 256, 7, 0, len(lens), len(lens), lens=lens)
    for k in (10, 3000):
        _check(cuda, (q, book, codes, off, ids, probe, bias), k, max_list_len=2 * RB + 600)
    _, want = _check(cuda, (q, book, codes, off, ids, probe, bias), 4096, max_list_len=RB - 1)
    assert ((want[1] >= 0).sum(1) == 1 + 4 * (RB - 1)).all() and 1 + 4 * (RB - 1) < 4096
    # m % 16 == 0 (16-byte code loads) at the same edges, the last list ending exactly at nd
    q, book, codes, off, ids, probe, bias = pc.random_index(16, 64, 16, 256, 5, 0, len(lens), len(lens), lens=lens)
    _check(cuda, (q, book, codes, off, ids, probe, bias), 500, max_list_len=sum(lens))


@functools.lru_cache(maxsize=None)
def _tie_case(place):
    """128 rows with identical codes spread over three lists with equal biases, five rows above them; row_ids from all of
    [0, 2^32): corner values, ids >= 2^31 and ids that differ only in high bits (tests/ivf_cases.py: _tie_ids)."""
    import ivf_cases as ic

    rng = np.random.default_rng(21)
    nd, m, K, run = 2000, 8, 256, ic.TIE_RUN
    q = rng.standard_normal((1, 32)).astype(np.float32)
    book = rng.standard_normal((m, K, 4)).astype(np.float32)
    table = pc.luts(q, book)[0]
    codes = rng.integers(0, K, size=(nd, m)).astype(np.uint8)
    copies = rng.choice(nd, size=run + 5, replace=False)
    tied = np.array([7, 200, 31, 0, 255, 128, 64, 9], np.uint8)
    codes[copies[:run]] = tied
    codes[copies[run:]] = table.argmax(1).astype(np.uint8)             # the best row there is: strictly above the run
    lens = np.bincount(rng.integers(0, 3, size=nd), minlength=3)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    in_list = np.bincount(np.searchsorted(off, copies[:run], "right") - 1, minlength=3)
    assert in_list.min() > 20                                          # the run is spread over the three lists
    ids_run, ids_rest = ic._tie_ids(rng, run, nd)
    ids = np.empty(nd, np.int64)
    ids[copies[:run]] = ids_run
    ids[np.setdiff1d(np.arange(nd), copies[:run])] = ids_rest
    assert (ids >= 1 << 31).any()
    bias = np.full((1, 3), 0.25, np.float32)
    scores = pc.adc_scores(table, codes, np.float32(0.25))
    tie = pc.adc_scores(table, tied[None, :], np.float32(0.25))[0]
    assert (scores == tie).sum() == run
    above = int((scores > tie).sum())
    assert above >= 5
    need = {"last": run, "one before last": run - 1, "first": 1}[place]
    return (q, book, codes, off, ids, np.array([[2, 0, 1]], np.int32), bias), above + need


@pytest.mark.parametrize("place", ["last", "one before last", "first"])
def test_ties_across_lists_under_ids_from_the_whole_32_bit_range(cuda, place):
    args, k = _tie_case(place)
    _, want = _check(cuda, args, k)
    assert (want[1] >= 0).all()


def test_three_query_tiles_by_the_candidate_cap_at_nprobe_256(cuda):
    """max_list_len = nd = 262144 as the bound at nprobe 256 and m = 4: 256 MiB of candidates a query, 8 queries a tile, 20 queries
    in tiles of 8, 8, 4 over the whole 2 GiB of candidates (allocated, not initialised).  300 lists of 300..1500 rows, k 4096."""
    import ivf_cases as ic

    case = ic.tiles_by_candidate_cap()
    nq, nd, nlist, k = len(case.q), len(case.d), case.nlist, case.k
    assert dense.ivfpq_scan_query_tile(nq, 256, k, 16, 4, 16, nlist, nd) == 8
    rng = np.random.default_rng(31)
    q = rng.standard_normal((nq, 16)).astype(np.float32)
    book = rng.standard_normal((4, 16, 4)).astype(np.float32)
    codes = rng.integers(0, 16, size=(nd, 4)).astype(np.uint8)
    _, off, ids = ic.list_major(case)
    bias = rng.standard_normal((nq, 256)).astype(np.float32)
    ws = torch.empty(dense.ivfpq_scan_workspace_bytes(nq, 256, k, 16, 4, 16, nlist, nd), dtype=torch.uint8, device=cuda)
    _check(cuda, (q, book, codes, off, ids, case.probe, bias), k, max_list_len=nd, workspace=ws)


def test_two_runs_give_the_same_bytes_and_outputs_are_written_in_place(cuda):
    args = pc.random_index(41, 64, 16, 256, 70, 4000, 6, 3)
    a = _run(cuda, *args, 50)
    out = (torch.full((70, 50), 7.0, dtype=torch.float32, device=cuda), torch.full((70, 50), -7, dtype=torch.int64, device=cuda))
    b = _run(cuda, *args, 50, out=out)
    torch.cuda.synchronize()
    assert b[0] is out[0] and b[1] is out[1]
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()
