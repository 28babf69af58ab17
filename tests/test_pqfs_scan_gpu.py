"""The packed 4-bit ADC scan and the packer (mevi_pqfs_scan_topk_f32, mevi_pq4_pack through mevi_amd.dense) against
tests/ivfpq_cases.py: adc_expected with K = 16 over the UNPACKED codes, and against the byte scan (dense.ivfpq_scan_topk) on the
same unpacked codes.  Bar: ids identical, scores identical as uint32 bits.  Shapes are the smallest that reach each path: dword
and 16-byte row loads (m % 32), one dword per row, the 128 KiB table of 32 copies, the tables of 16 copies (m > 64), several row
blocks, several query tiles."""
import functools

import numpy as np
import pytest
import torch

import ivfpq_cases as pc
import pqfs_cases as fc
from mevi_amd import dense

pytestmark = pytest.mark.gpu

RB = dense.PQFS_ROW_BLOCK
FLT_MAX = np.finfo(np.float32).max


def _dev(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a)).to(cuda)          # a copy: shared cases are read-only


def _run(cuda, q, book, codes, off, ids, probe, bias, k, max_list_len=None, **kw):
    """`codes` are the unpacked u8 [nd, m]; the device packs them."""
    longest = int(np.diff(off).max()) if max_list_len is None else max_list_len
    packed = dense.pq4_pack(_dev(cuda, codes))
    return dense.pqfs_scan_topk(_dev(cuda, q), _dev(cuda, book), packed, _dev(cuda, off), _dev(cuda, ids), longest, _dev(cuda, probe),
                                _dev(cuda, bias), k, **kw)


def _bytes_run(cuda, q, book, codes, off, ids, probe, bias, k, max_list_len=None):
    longest = int(np.diff(off).max()) if max_list_len is None else max_list_len
    return dense.ivfpq_scan_topk(_dev(cuda, q), _dev(cuda, book), _dev(cuda, codes), _dev(cuda, off), _dev(cuda, ids), longest,
                                 _dev(cuda, probe), _dev(cuda, bias), k)


def _same(got, want):
    s, i = got
    torch.cuda.synchronize()
    np.testing.assert_array_equal(i.cpu().numpy(), want[1])
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), want[0].view(np.uint32))


def _check(cuda, args, k, max_list_len=None, byte_scan=True, **kw):
    want = pc.adc_expected(*args, k, max_list_len=max_list_len)
    got = _run(cuda, *args, k, max_list_len=max_list_len, **kw)
    _same(got, want)
    if byte_scan:                                      # the existing scan at K = 16 over the unpacked codes: the same bits
        _same(_bytes_run(cuda, *args, k, max_list_len=max_list_len), want)
    return got, want


@pytest.mark.parametrize("dim,m,nq,nd,nlist,nprobe,k", [
    (32, 8, 1, 300, 4, 1, 1),               # one dword per row
    (96, 24, 33, 3000, 8, 3, 1000),         # 12-byte rows, dword loads
    (128, 32, 33, 5000, 8, 8, 4096),        # the first 16-byte load; eight draws of eight lists: repeats and padding
    (256, 64, 33, 3000, 8, 2, 10),          # the largest table of 32 copies: 128 KiB
    (768, 96, 5, 2500, 10, 3, 100),         # 16 copies, 96 KiB, 16-byte loads
    (288, 72, 5, 2500, 10, 3, 10),          # 16 copies, 36-byte rows: dword loads
    (768, 64, 257, 3000, 10, 1, 10),        # the C2 index shape
])
def test_scan_equals_adc_expected_over_shapes(cuda, dim, m, nq, nd, nlist, nprobe, k):
    args = pc.random_index(dim * 3 + m + nq, dim, m, 16, nq, nd, nlist, nprobe, repeats=k == 4096)
    _, want = _check(cuda, args, k)
    if k == 4096:
        assert (want[1][:, -1] == -1).sum() > 10 and (want[1][:, 0] >= 0).all()     # the case does pad


def test_nibble_order(cuda):
    """Every byte 0xF0: the even codes are 0, the odd ones 15, over a codebook with distinct entries.  Reading the nibbles the
    other way round gives another expected list, so the equality below does pin the order."""
    q, book, codes, off, ids, probe, bias = pc.random_index(51, 32, 8, 16, 4, 600, 3, 2)
    codes = codes.copy()
    marked = np.arange(0, 600, 3)
    codes[marked, 0::2] = 0
    codes[marked, 1::2] = 15
    packed = fc.pack(codes)
    assert (packed[marked] == 0xF0).all() and len({tuple(e) for j in range(8) for e in book[j].tolist()}) == 8 * 16
    args = (q, book, codes, off, ids, probe, bias)
    _, want = _check(cuda, args, 50)
    wrong = pc.adc_expected(q, book, fc.unpack_swapped(packed), off, ids, probe, bias, 50)
    assert not np.array_equal(wrong[1], want[1]) and not np.array_equal(wrong[0], want[0])


@pytest.mark.parametrize("n,m", [(0, 8), (1, 8), (1, 96), (1027, 24), (4096, 64)])
def test_pack_kernel_equals_numpy_and_masks_high_bits(cuda, n, m):
    rng = np.random.default_rng(n + m)
    codes = rng.integers(0, 256, size=(n, m)).astype(np.uint8)         # bytes >= 16: only their low 4 bits count
    got = dense.pq4_pack(_dev(cuda, codes))
    torch.cuda.synchronize()
    assert got.shape == (n, m // 2) and got.dtype == torch.uint8
    np.testing.assert_array_equal(got.cpu().numpy(), fc.pack(codes))
    np.testing.assert_array_equal(got.cpu().numpy(), fc.pack(codes & 15))
    out = torch.full((n + 2, m // 2), 0xA5, dtype=torch.uint8, device=cuda)
    assert dense.pq4_pack(_dev(cuda, codes), out=out[1:n + 1]).data_ptr() == out[1:n + 1].data_ptr()
    torch.cuda.synchronize()
    assert bool((out[0] == 0xA5).all()) and bool((out[n + 1] == 0xA5).all())       # nothing written around the rows
    np.testing.assert_array_equal(out[1:n + 1].cpu().numpy(), fc.pack(codes))


def test_row_alignment_and_row_block_edges_at_m_8(cuda):
    """m = 8: a packed row is one dword, so rows are only 4-byte aligned.  Lists of 0, 1 and 2 rows in between move the starts of
    the long lists (RB - 1, RB, RB + 1 and 2 RB + 1 rows) to every residue mod 4.  Every query probes all lists in
    its own slot order, under a bound above the longest list and under one below it (clamped, never overrun)."""
    lens = [1, RB - 1, 0, RB, 2, RB + 1, 0, 2 * RB + 1]
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    assert {int(s) % 4 for s, n in zip(starts, lens) if n >= RB - 1} == {0, 1, 2, 3}
    q, book, codes, off, ids, probe, bias = pc.random_index(15, 32, 8, 16, 6, 0, len(lens), len(lens), lens=lens)
    for k in (10, 3000):
        _check(cuda, (q, book, codes, off, ids, probe, bias), k, max_list_len=2 * RB + 600)
    _, want = _check(cuda, (q, book, codes, off, ids, probe, bias), 4096, max_list_len=RB - 1)
    probed = sum(min(n, RB - 1) for n in lens)
    assert ((want[1] >= 0).sum(1) == min(probed, 4096)).all()
    # 16-byte loads at the same edges, the last list ending exactly at nd
    lens = [0, 1, RB - 1, RB, RB + 1, 2 * RB + 1]
    q, book, codes, off, ids, probe, bias = pc.random_index(16, 128, 32, 16, 5, 0, len(lens), len(lens), lens=lens)
    _check(cuda, (q, book, codes, off, ids, probe, bias), 500, max_list_len=sum(lens))


@pytest.mark.parametrize("m", [8, 32])
def test_flat_pq_one_list_no_bias_no_row_ids(cuda, m):
    """IndexPQFastScan: one list, probe_score NULL (bias +0), row_ids NULL (the id is the row); 2 * RB + 77 rows = three row blocks."""
    q, book, codes, off, _, _, _ = pc.random_index(11, 4 * m, m, 16, 9, 0, 1, 1, lens=[2 * RB + 77])
    probe = np.zeros((9, 1), np.int32)
    _check(cuda, (q, book, codes, off, None, probe, None), 100)


def test_probe_edges_then_a_normal_call_on_the_same_workspace(cuda):
    """-1 entries, entries >= nlist, a list named twice whose slots carry DIFFERENT biases (the first wins), empty lists, a table of
    -1 (all padding), each followed by a normal call on the same workspace."""
    lens = [0, 50, 0, 700, RB + 5, 30]
    q, book, codes, off, ids, _, _ = pc.random_index(13, 32, 8, 16, 40, 0, len(lens), 4, lens=lens)
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
    ws = torch.full((dense.pqfs_scan_workspace_bytes(nq, 4, k, 32, 8, nlist, max(lens)),), 0xA5, dtype=torch.uint8, device=cuda)
    first, want_normal = _check(cuda, (q, book, codes, off, ids, normal, bias), k, workspace=ws)
    _, want = _check(cuda, (q, book, codes, off, ids, edges, bias), k, workspace=ws)
    assert (want[1][7] == -1).all() and (want[1][9] == -1).all() and (want[1][8] >= 0).all()
    # the repeated list counted once and with the first slot's bias: the second slot's bias would have given other scores
    swapped = bias.copy()
    swapped[::4, 0], swapped[::4, 3] = bias[::4, 3], bias[::4, 0]
    other = pc.adc_expected(q, book, codes, off, ids, edges, swapped, k)
    assert not np.array_equal(other[0][::4], want[0][::4])
    nothing = np.full((nq, 4), -1, np.int32)
    (s, i), _ = _check(cuda, (q, book, codes, off, ids, nothing, bias), k, byte_scan=False, workspace=ws)
    assert bool((i == -1).all()) and bool((s == -FLT_MAX).all())
    again, _ = _check(cuda, (q, book, codes, off, ids, normal, bias), k, byte_scan=False, workspace=ws)
    assert again[0].cpu().numpy().tobytes() == want_normal[0].tobytes() and again[1].cpu().numpy().tobytes() == want_normal[1].tobytes()


@functools.lru_cache(maxsize=None)
def _tie_case(place):
    """128 rows with identical codes spread over three lists with equal biases, five rows above them; row_ids from all of
    [0, 2^32): corner values, ids >= 2^31 and ids that differ only in high bits (tests/ivf_cases.py: _tie_ids)."""
    import ivf_cases as ic

    rng = np.random.default_rng(21)
    nd, m, run = 2000, 8, ic.TIE_RUN
    q = rng.standard_normal((1, 32)).astype(np.float32)
    book = rng.standard_normal((m, 16, 4)).astype(np.float32)
    table = pc.luts(q, book)[0]
    codes = rng.integers(0, 16, size=(nd, m)).astype(np.uint8)
    copies = rng.choice(nd, size=run + 5, replace=False)
    tied = np.array([7, 2, 15, 0, 9, 12, 4, 1], np.uint8)
    assert not np.array_equal(tied, table.argmax(1))
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
    assert (scores == tie).sum() >= run
    above = int((scores > tie).sum())
    assert above >= 5
    need = {"last": int((scores == tie).sum()), "one before last": int((scores == tie).sum()) - 1, "first": 1}[place]
    return (q, book, codes, off, ids, np.array([[2, 0, 1]], np.int32), bias), above + need


@pytest.mark.parametrize("place", ["last", "one before last", "first"])
def test_ties_across_lists_under_ids_from_the_whole_32_bit_range(cuda, place):
    args, k = _tie_case(place)
    _, want = _check(cuda, args, k)
    assert (want[1] >= 0).all()


def test_padding_when_k_exceeds_the_probed_rows(cuda):
    args = pc.random_index(7, 96, 24, 16, 17, 3000, 8, 8)
    _, want = _check(cuda, args, 4096)
    assert (want[1][:, 3000:] == -1).all() and (want[1][:, :3000] >= 0).all() and (want[0][:, 3000:] == -FLT_MAX).all()


def test_three_query_tiles_by_the_candidate_cap_at_nprobe_256(cuda):
    """max_list_len = nd = 262144 as the bound at nprobe 256: 256 MiB of candidates a query, so the tile derived from
    mevi_pqfs_scan_query_tile walks the 20 queries in at least three tiles, the last one ragged, over the whole 2 GiB of
    candidates (allocated, not initialised).  300 lists of 300..1500 rows, k 4096."""
    import ivf_cases as ic

    case = ic.tiles_by_candidate_cap()
    nq, nd, nlist, k = len(case.q), len(case.d), case.nlist, case.k
    tile = dense.pqfs_scan_query_tile(nq, 256, k, 32, 8, nlist, nd)
    assert tile >= 1 and -(-nq // tile) >= 3 and nq % tile != 0
    rng = np.random.default_rng(31)
    q = rng.standard_normal((nq, 32)).astype(np.float32)
    book = rng.standard_normal((8, 16, 4)).astype(np.float32)
    codes = rng.integers(0, 16, size=(nd, 8)).astype(np.uint8)
    _, off, ids = ic.list_major(case)
    bias = rng.standard_normal((nq, 256)).astype(np.float32)
    ws = torch.empty(dense.pqfs_scan_workspace_bytes(nq, 256, k, 32, 8, nlist, nd), dtype=torch.uint8, device=cuda)
    _check(cuda, (q, book, codes, off, ids, case.probe, bias), k, max_list_len=nd, byte_scan=False, workspace=ws)


def test_rows_beyond_nd_are_never_read(cuda):
    """The buffer holds 64 more rows behind nd whose codes are every subspace's best entry for every query (the queries are
    positive and one entry is the only large positive one); the last list ends at nd, in the middle of a row block.  A scan that
    read on -- the reference over a list reaching behind nd shows it -- would return nothing but them."""
    rng = np.random.default_rng(61)
    nq, m, dim, nd, extra = 7, 8, 32, 1500, 64
    q = np.abs(rng.standard_normal((nq, dim))).astype(np.float32)      # all positive: entry 5, the only large positive one, is best
    book = (rng.standard_normal((m, 16, 4)) * 0.1).astype(np.float32)
    book[:, 5] = 3.0
    codes = rng.integers(0, 16, size=(nd + extra, m)).astype(np.uint8)
    codes[:nd][codes[:nd] == 5] = 6
    codes[nd:] = 5
    lens = [400, 600, 500]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.arange(nd + extra, dtype=np.int64)[::-1].copy()
    probe = np.tile(np.array([[2, 0, 1]], np.int32), (nq, 1))
    bias = rng.standard_normal((nq, 3)).astype(np.float32)
    over = off.copy()
    over[-1] = nd + extra                              # what reading on behind nd would see
    k = 20
    would = pc.adc_expected(q, book, codes, over, ids, probe, bias, k)
    assert (would[1] < extra).all()                    # ... and they would fill the whole result
    want = pc.adc_expected(q, book, codes[:nd], off, ids[:nd], probe, bias, k)
    packed_all = dense.pq4_pack(_dev(cuda, codes))
    ids_all = _dev(cuda, ids)
    got = dense.pqfs_scan_topk(_dev(cuda, q), _dev(cuda, book), packed_all[:nd], _dev(cuda, off), ids_all[:nd], nd, _dev(cuda, probe),
                               _dev(cuda, bias), k)
    _same(got, want)
    assert bool((got[1] >= extra).all())


def test_graph_replay_equals_eager_and_two_runs_give_the_same_bytes(cuda):
    args = pc.random_index(41, 128, 32, 16, 70, 4000, 6, 3)
    q, book, codes, off, ids, probe, bias = args
    k = 50
    want = pc.adc_expected(*args, k)
    t = [_dev(cuda, a) for a in (q, book, off, ids, probe, bias)]
    packed = dense.pq4_pack(_dev(cuda, codes))
    longest = int(np.diff(off).max())
    ws = torch.empty(dense.pqfs_scan_workspace_bytes(70, 3, k, 128, 32, 6, longest), dtype=torch.uint8, device=cuda)
    out = (torch.full((70, k), 7.0, dtype=torch.float32, device=cuda), torch.full((70, k), -7, dtype=torch.int64, device=cuda))

    def call():
        return dense.pqfs_scan_topk(t[0], t[1], packed, t[2], t[3], longest, t[4], t[5], k, out=out, workspace=ws)

    eager = call()
    assert eager[0] is out[0] and eager[1] is out[1]
    _same(eager, want)
    first = (out[0].clone(), out[1].clone())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    out[0].fill_(7.0)
    out[1].fill_(-7)
    graph.replay()
    _same(out, want)
    assert torch.equal(out[0].view(torch.int32), first[0].view(torch.int32)) and torch.equal(out[1], first[1])
    for i in (0, 4, 5):                                # the queries in reverse order in the same buffers: the replay follows them
        t[i].copy_(torch.flip(t[i], [0]))
    graph.replay()
    _same(out, (want[0][::-1], want[1][::-1]))
