"""The scalar-quantised list scan (mevi_sq_scan_topk_f32 through dense.sq_scan_topk) against tests/sq_cases.py: sq_expected, which
is numpy f32 and oracle calls only.  Bar: ids identical, scores identical as uint32 bits.  Shapes are the smallest that reach each
path: dim 16 (tail loop only), 20 (8-bit rows of 20 bytes: dword code loads), 48 (one chunk of 32 and a tail; 24-byte rows at 4
bits), 768 (16-byte code loads at both widths); one and two accumulators, one and two pair tiles, several row blocks, several
query tiles.  The same calls are held against the EXISTING kernels over the decoded rows: the IVF-Flat scan and the exact search."""
import numpy as np
import pytest
import torch

import sq_cases as sc
from mevi_amd import dense

pytestmark = pytest.mark.gpu

RB = dense.IVF_ROW_BLOCK
FLT_MAX = np.finfo(np.float32).max
SHAPES = [(16, 8), (16, 4), (20, 8), (48, 8), (48, 4), (768, 8), (768, 4)]          # every legal (dim, bits) of the dims above


def _dev(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a)).to(cuda)          # a copy: shared cases are read-only


def _run(cuda, q, codes, vmin, vdiff, bits, off, ids, probe, bias, k, max_list_len=None, **kw):
    longest = int(np.diff(off).max()) if max_list_len is None else max_list_len
    return dense.sq_scan_topk(_dev(cuda, q), _dev(cuda, codes), _dev(cuda, vmin), _dev(cuda, vdiff), bits, _dev(cuda, off),
                              _dev(cuda, ids), longest, _dev(cuda, probe), _dev(cuda, bias), k, **kw)


def _same(got, want):
    s, i = got
    torch.cuda.synchronize()
    np.testing.assert_array_equal(i.cpu().numpy(), want[1])
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), want[0].view(np.uint32))


def _check(cuda, args, k, max_list_len=None, **kw):
    want = sc.sq_expected(*args, k, max_list_len=max_list_len)
    got = _run(cuda, *args, k, max_list_len=max_list_len, **kw)
    _same(got, want)
    return got, want


def _flat_scan_over_decoded(cuda, args, k, max_list_len=None):
    """dense.ivf_scan_topk over the rows decoded on the device (mevi_amd.sq.decode, itself held against the numpy decode)."""
    from mevi_amd import sq

    q, codes, vmin, vdiff, bits, off, ids, probe, _ = args
    rows = sq.decode(_dev(cuda, codes), _dev(cuda, vmin), _dev(cuda, vdiff), bits)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rows.cpu().numpy().view(np.uint32), sc.decode(codes, vmin, vdiff, bits).view(np.uint32))
    longest = int(np.diff(off).max()) if max_list_len is None else max_list_len
    return dense.ivf_scan_topk(_dev(cuda, q), rows.contiguous(), _dev(cuda, off), _dev(cuda, ids), longest, _dev(cuda, probe), k)


@pytest.mark.parametrize("dim,bits", SHAPES)
def test_scan_equals_expected_and_the_ivf_flat_scan_over_decoded_rows(cuda, dim, bits):
    """33 queries x 3 of 6 lists (repeats allowed) over 900 rows; then the same call without a bias against the existing IVF-Flat
    scan over the decoded rows, bit for bit."""
    args = sc.random_index(dim * 3 + bits, dim, bits, 33, 900, 6, 3, repeats=True)
    _check(cuda, args, 100)
    unbiased = args[:8] + (None,)
    got, want = _check(cuda, unbiased, 100)
    _same(_flat_scan_over_decoded(cuda, unbiased, 100), want)
    assert not np.array_equal(want[0], sc.sq_expected(*args, 100)[0])                 # the bias does count


@pytest.mark.parametrize("bits", [8, 4])
def test_row_block_edges_under_a_larger_and_a_smaller_bound(cuda, bits):
    """Lists of 0, 1, 127, 128, 129 and 2 * 128 + 1 rows, every query probing all of them in its own slot order, with max_list_len
    above the longest list; then a bound BELOW the longest lists: they are clamped, never overrun."""
    lens = [0, 1, RB - 1, RB, RB + 1, 2 * RB + 1]
    args = sc.random_index(15 + bits, 48, bits, 7, 0, len(lens), len(lens), lens=lens)
    for k in (10, 700):
        _check(cuda, args, k, max_list_len=2 * RB + 300)
    _, want = _check(cuda, args, 4096, max_list_len=RB - 1)
    assert ((want[1] >= 0).sum(1) == 1 + 4 * (RB - 1)).all() and 1 + 4 * (RB - 1) < 4096
    _check(cuda, args, 50, max_list_len=sum(lens))                                    # the last list ends exactly at nd


@pytest.mark.parametrize("pairs", [1, 32, 33, 64, 65])
@pytest.mark.parametrize("dim,bits", [(20, 8), (16, 4), (48, 8)])
def test_pair_counts_on_one_list(cuda, pairs, dim, bits):
    """1, 32, 33, 64 and 65 (query, slot) pairs on ONE list of 200 rows: one accumulator, both, and the second pair tile."""
    q, codes, vmin, vdiff, _, off, ids, _, bias = sc.random_index(pairs + dim, dim, bits, pairs, 0, 2, 1, lens=[37, 200])
    probe = np.ones((pairs, 1), np.int32)
    _check(cuda, (q, codes, vmin, vdiff, bits, off, ids, probe, bias), 60)


@pytest.mark.parametrize("bits", [8, 4])
def test_probe_edges_then_a_normal_call_on_the_same_workspace(cuda, bits):
    """-1 entries, entries >= nlist, INT32_MIN, a list named twice whose slots carry DIFFERENT biases (the first wins), empty lists,
    a query that probes nothing, a table of -1 (all padding), each followed by a normal call on the same 0xA5-filled workspace."""
    lens = [0, 50, 0, 300, RB + 5, 30]
    q, codes, vmin, vdiff, _, off, ids, _, _ = sc.random_index(13 + bits, 32, bits, 40, 0, len(lens), 4, lens=lens)
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
    fixed = (q, codes, vmin, vdiff, bits, off, ids)
    ws = torch.full((dense.sq_scan_workspace_bytes(nq, 4, k, 32, bits, nlist, max(lens)),), 0xA5, dtype=torch.uint8, device=cuda)
    first, want_normal = _check(cuda, fixed + (normal, bias), k, workspace=ws)
    _, want = _check(cuda, fixed + (edges, bias), k, workspace=ws)
    assert (want[1][7] == -1).all() and (want[1][9] == -1).all() and (want[1][8] >= 0).all()
    # the repeated list counted once and with the first slot's bias: the second slot's bias would have given other scores
    swapped = bias.copy()
    swapped[::4, 0], swapped[::4, 3] = bias[::4, 3], bias[::4, 0]
    other, _ = _check(cuda, fixed + (edges, swapped), k, workspace=ws)
    assert not np.array_equal(other[0].cpu().numpy()[::4], want[0][::4])
    _check(cuda, fixed + (normal, bias), k, workspace=ws)
    nothing = np.full((nq, 4), -1, np.int32)
    (s, i), _ = _check(cuda, fixed + (nothing, bias), k, workspace=ws)
    assert bool((i == -1).all()) and bool((s == -FLT_MAX).all())
    again, _ = _check(cuda, fixed + (normal, bias), k, workspace=ws)
    assert again[0].cpu().numpy().tobytes() == want_normal[0].tobytes() and again[1].cpu().numpy().tobytes() == want_normal[1].tobytes()


def test_padding_when_k_exceeds_the_probed_rows(cuda):
    """k = 4096 over eight draws of eight lists of 3000 rows in all: every query's tail is -FLT_MAX / -1."""
    args = sc.random_index(7, 20, 8, 65, 3000, 8, 8, repeats=True)
    _, want = _check(cuda, args, 4096)
    assert (want[1][:, 3000:] == -1).all() and (want[1][:, 0] >= 0).all() and (want[0][:, 3000:] == -FLT_MAX).all()
    assert (want[1][:, -1] == -1).all()


@pytest.mark.parametrize("dim,bits", [(48, 8), (48, 4), (768, 8)])
def test_flat_index_one_list_no_bias_no_row_ids(cuda, dim, bits):
    """IndexScalarQuantizer: one list, probe_score NULL, row_ids NULL (the id is the row); 2 * 128 + 77 rows = three row blocks.
    The same answer comes from the existing kernels over the decoded rows: the IVF-Flat scan and the exact search."""
    q, codes, vmin, vdiff, _, off, _, _, _ = sc.random_index(11 + dim + bits, dim, bits, 9, 0, 1, 1, lens=[2 * RB + 77])
    probe = np.zeros((9, 1), np.int32)
    args = (q, codes, vmin, vdiff, bits, off, None, probe, None)
    _, want = _check(cuda, args, 100)
    _same(_flat_scan_over_decoded(cuda, args, 100), want)
    rows = _dev(cuda, sc.decode(codes, vmin, vdiff, bits))
    _same(dense.DenseIndex(rows).search(_dev(cuda, q), 100), want)


@pytest.mark.parametrize("bits", [8, 4])
def test_end_levels_zero_ranges_and_negative_minima(cuda, bits):
    """Codes that are all 0 and all L, dimensions with vdiff == 0 (they decode to vmin whatever the code) and vmin < 0 throughout."""
    q, codes, vmin, vdiff, _, off, ids, probe, bias = sc.random_index(23 + bits, 48, bits, 12, 700, 4, 2)
    vmin = -np.abs(vmin) - np.float32(0.5)
    vdiff[::5] = 0.0
    codes[:100] = 0
    codes[100:200] = 255                              # level L in every byte, or in both nibbles
    codes[200:230, ::2] = 0
    args = (q, codes, vmin, vdiff, bits, off, ids, probe, bias)
    decoded = sc.decode(codes, vmin, vdiff, bits)
    assert (decoded[:, ::5] == vmin[::5]).all() and (decoded[:100] == (vmin + vdiff * sc.levels(bits)[0])).all()
    assert (sc.unpack(codes[100:200], bits) == (1 << bits) - 1).all()
    _check(cuda, args, 300)
    _same(_flat_scan_over_decoded(cuda, args[:8] + (None,), 300), sc.sq_expected(*args[:8], None, 300))


def test_an_id_above_two_to_the_31_and_ties_by_unsigned_id(cuda):
    """Rows with identical codes in one list tie; their ids, one of them above 2^31, order them as unsigned 32-bit values."""
    q, codes, vmin, vdiff, bits, off, ids, probe, bias = sc.random_index(29, 16, 8, 3, 0, 2, 2, lens=[40, 60])
    codes[45:50] = codes[44]
    ids = ids.copy()
    ids[46] = (1 << 31) + 5
    ids[48] = (1 << 32) - 1
    _, want = _check(cuda, (q, codes, vmin, vdiff, bits, off, ids, probe, bias), 100)
    assert ((want[1] == (1 << 31) + 5).sum(1) == 1).all() and ((want[1] == (1 << 32) - 1).sum(1) == 1).all()
    where = [np.flatnonzero(np.isin(row, ids[44:50])) for row in want[1]]
    assert all(len(w) == 6 and (np.diff(w) == 1).all() and (np.diff(row[w]) > 0).all() for w, row in zip(where, want[1]))


def test_three_query_tiles_by_the_candidate_cap_at_nprobe_256(cuda):
    """max_list_len = nd = 262144 as the bound at nprobe 256: 256 MiB of candidates a query, 8 queries a tile, 20 queries in tiles
    of 8, 8, 4 over the whole 2 GiB of candidates (allocated, not initialised).  300 lists of 300..1500 rows, k 4096."""
    import ivf_cases as ic

    case = ic.tiles_by_candidate_cap()
    nq, nd, nlist, k = len(case.q), len(case.d), case.nlist, case.k
    assert dense.sq_scan_query_tile(nq, 256, k, 16, 8, nlist, nd) == 8
    rng = np.random.default_rng(31)
    q = rng.standard_normal((nq, 16)).astype(np.float32)
    codes = rng.integers(0, 256, size=(nd, 16)).astype(np.uint8)
    vmin = (rng.standard_normal(16) - 0.3).astype(np.float32)
    vdiff = (rng.random(16) + 0.01).astype(np.float32)
    _, off, ids = ic.list_major(case)
    bias = rng.standard_normal((nq, 256)).astype(np.float32)
    ws = torch.empty(dense.sq_scan_workspace_bytes(nq, 256, k, 16, 8, nlist, nd), dtype=torch.uint8, device=cuda)
    _check(cuda, (q, codes, vmin, vdiff, 8, off, ids, case.probe, bias), k, max_list_len=nd, workspace=ws)


def test_two_runs_give_the_same_bytes_and_outputs_are_written_in_place(cuda):
    args = sc.random_index(41, 64, 4, 70, 4000, 6, 3)
    a = _run(cuda, *args, 50)
    out = (torch.full((70, 50), 7.0, dtype=torch.float32, device=cuda), torch.full((70, 50), -7, dtype=torch.int64, device=cuda))
    b = _run(cuda, *args, 50, out=out)
    torch.cuda.synchronize()
    assert b[0] is out[0] and b[1] is out[1]
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()
