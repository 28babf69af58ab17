"""The additive quantiser's ADC list scan (mevi_aq_scan_topk_f32 through dense.aq_scan_topk) against tests/aq_cases.py: aq_expected,
which is built from oracle calls only.  Bar: ids identical, scores identical as uint32 bits.  Shapes are the smallest that reach each
path: both code-load widths (M % 16), K = 256 and K known at run time, the 96 KiB table, both table kernels (fewer than 64 queries in
a tile, and more), dim below, across and many times their k slabs, several row blocks, two query tiles."""
import numpy as np
import pytest
import torch

import aq_cases as ac
import ivfpq_cases as pc
from mevi_amd import dense

pytestmark = pytest.mark.gpu

RB = dense.IVFPQ_ROW_BLOCK
FLT_MAX = np.finfo(np.float32).max


def _dev(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a)).to(cuda)          # a copy: shared cases are read-only


def _run(cuda, q, book, codes, off, ids, probe, bias, k, max_list_len=None, fn=dense.aq_scan_topk, **kw):
    longest = int(np.diff(off).max()) if max_list_len is None else max_list_len
    return fn(_dev(cuda, q), _dev(cuda, book), _dev(cuda, codes), _dev(cuda, off), _dev(cuda, ids), longest, _dev(cuda, probe),
              _dev(cuda, bias), k, **kw)


def _same(got, want):
    s, i = got
    torch.cuda.synchronize()
    np.testing.assert_array_equal(i.cpu().numpy(), want[1])
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), want[0].view(np.uint32))


def _check(cuda, args, k, max_list_len=None, **kw):
    want = ac.aq_expected(*args, k, max_list_len=max_list_len)
    got = _run(cuda, *args, k, max_list_len=max_list_len, **kw)
    _same(got, want)
    return got, want


@pytest.mark.parametrize("dim,M,K,nq,nd,nlist,nprobe,k", [
    (4, 4, 16, 1, 300, 4, 1, 10),             # the smallest of everything
    (4, 4, 1, 3, 100, 2, 2, 1),               # one centroid a level: every code is 0; k 1
    (36, 12, 200, 33, 3000, 8, 3, 1000),      # M % 16 != 0 (dword code loads), K no power of two, dim across a 32-column slab
    (36, 20, 256, 65, 5000, 8, 8, 4096),      # eight draws of eight lists: repeats, some 3300 probed rows a query: padding; matrix cores
    (768, 64, 256, 70, 3000, 10, 1, 10),      # the C2 index shape: 16-byte code loads, a 64 KiB table, matrix-core tables
    (768, 64, 256, 5, 3000, 10, 16, 10),      # ... and the few-query table kernel; nprobe above nlist: repeats
    (768, 96, 256, 5, 2000, 10, 3, 100),      # the 96 KiB table (dynamic LDS above 64 KiB)
    (36, 96, 16, 17, 2000, 5, 2, 10),         # 96 levels of 16
    (100, 64, 16, 33, 1500, 6, 2, 50),        # 16-byte code loads with K != 256: codes clamped to K - 1 at run time
    (36, 4, 256, 300, 2500, 7, 2, 10),        # 300 queries
])
def test_scan_equals_aq_expected_over_shapes(cuda, dim, M, K, nq, nd, nlist, nprobe, k):
    args = ac.random_index(dim * 3 + M + nq, dim, M, K, nq, nd, nlist, nprobe, repeats=k == 4096 or nprobe > nlist)
    _, want = _check(cuda, args, k)
    if k == 4096:
        assert (want[1][:, -1] == -1).sum() > 30 and (want[1][:, 0] >= 0).all()     # the case does pad


def test_padding_when_k_exceeds_the_probed_rows(cuda):
    """Fewer rows than k = 4096: every query's tail is -FLT_MAX / -1."""
    args = ac.random_index(7, 36, 20, 256, 65, 3000, 8, 8)
    _, want = _check(cuda, args, 4096)
    assert (want[1][:, 3000:] == -1).all() and (want[1][:, :3000] >= 0).all() and (want[0][:, 3000:] == -FLT_MAX).all()


@pytest.mark.parametrize("M,K,dim", [(16, 256, 36), (8, 32, 4)])
def test_flat_form_one_list_no_bias_no_row_ids(cuda, M, K, dim):
    """IndexResidualQuantizer: one list, probe_score NULL (bias +0), row_ids NULL (the id is the row); 2 * RB + 77 rows = three row blocks."""
    q, book, codes, off, _, _, _ = ac.random_index(11, dim, M, K, 9, 0, 1, 1, lens=[2 * RB + 77])
    probe = np.zeros((9, 1), np.int32)
    _check(cuda, (q, book, codes, off, None, probe, None), 100)


@pytest.mark.parametrize("nprobe", [1, 16, 256])
def test_probe_counts_with_repeats_and_entries_out_of_range(cuda, nprobe):
    """nprobe 1, 16 and 256 over 40 lists (some empty): independent draws (repeats), -1, nlist and INT_MIN entries, a list named twice
    under DIFFERENT biases (the first wins), a query that probes nothing, one that probes only empty lists."""
    lens = [0, 50, 0, 70] + [int(x) for x in np.random.default_rng(3).integers(0, 90, size=36)]
    nlist, nq, k = len(lens), 24, 60
    q, book, codes, off, ids, probe, bias = ac.random_index(13 + nprobe, 36, 8, 64, nq, 0, nlist, nprobe, lens=lens, repeats=True)
    probe[::3, 0] = -1
    probe[1::5, -1] = nlist                          # past the last list
    probe[2::7, 0] = np.iinfo(np.int32).min
    if nprobe > 1:
        probe[::4, -1] = probe[::4, 0]               # the same list twice, under another bias
        probe[9] = [0, 2] * (nprobe // 2)            # only empty lists
    probe[7] = -1                                    # a query that probes nothing
    _, want = _check(cuda, (q, book, codes, off, ids, probe, bias), k)
    assert (want[1][7] == -1).all() and (want[0][7] == -FLT_MAX).all()
    if nprobe > 1:
        assert (want[1][9] == -1).all()
        swapped = bias.copy()
        swapped[::4, 0], swapped[::4, -1] = bias[::4, -1], bias[::4, 0]
        other = ac.aq_expected(q, book, codes, off, ids, probe, swapped, k)
        assert not np.array_equal(other[0][::4], want[0][::4])


def test_empty_lists_long_lists_and_a_bound_below_the_longest(cuda):
    """Lists of 0, 1, RB - 1, RB, RB + 1 and 2 RB + 1 rows, every query probing all of them in its own slot order, with max_list_len
    above the longest list; then a bound BELOW the longest lists: they are clamped, never overrun; then 16-byte code loads at the same
    edges, the last list ending exactly at nd."""
    lens = [0, 1, RB - 1, RB, RB + 1, 2 * RB + 1]
    q, book, codes, off, ids, probe, bias = ac.random_index(15, 36, 4, 256, 7, 0, len(lens), len(lens), lens=lens)
    for k in (10, 3000):
        _check(cuda, (q, book, codes, off, ids, probe, bias), k, max_list_len=2 * RB + 600)
    _, want = _check(cuda, (q, book, codes, off, ids, probe, bias), 4096, max_list_len=RB - 1)
    assert ((want[1] >= 0).sum(1) == 1 + 4 * (RB - 1)).all() and 1 + 4 * (RB - 1) < 4096
    q, book, codes, off, ids, probe, bias = ac.random_index(16, 4, 16, 256, 5, 0, len(lens), len(lens), lens=lens)
    _check(cuda, (q, book, codes, off, ids, probe, bias), 500, max_list_len=sum(lens))
    _check(cuda, (q, book, codes, off, None, probe, bias), 500, max_list_len=sum(lens))        # row_ids NULL behind lists


def test_two_query_tiles_by_the_table_cap(cuda):
    """96 levels of 256 centroids: 96 KiB of tables a query, 1365 queries in the 128 MiB of a tile; 1370 queries are tiles of 1365
    (matrix-core tables) and 5 (the few-query kernel), at dim 4: one short k slab."""
    nq, M, K, dim, nlist = 1370, 96, 256, 4, 3
    assert dense.aq_scan_query_tile(nq, 2, 10, dim, M, K, nlist, 300) == 1365
    args = ac.random_index(31, dim, M, K, nq, 600, nlist, 2)
    assert int(np.diff(args[3]).max()) <= 300
    _check(cuda, args, 10, max_list_len=300)


@pytest.mark.parametrize("m,dsub,K,nq", [(8, 4, 256, 5), (16, 48, 256, 70), (12, 12, 100, 33)])
def test_a_block_diagonal_codebook_gives_the_product_quantisers_scan(cuda, m, dsub, K, nq):
    """Level j of the codebook = subspace j of a product codebook in columns j * dsub ..., zero elsewhere: the same tables (a chain
    over zeros changes nothing), the same codes, so mevi_aq_scan_topk_f32 returns the bits of mevi_ivfpq_scan_topk_f32."""
    q, pq_book, codes, off, ids, probe, bias = pc.random_index(50 + m, m * dsub, m, K, nq, 3000, 6, 3)
    book = ac.pq_as_aq(pq_book)
    want = _run(cuda, q, pq_book, codes, off, ids, probe, bias, 100, fn=dense.ivfpq_scan_topk)
    got = _run(cuda, q, book, codes, off, ids, probe, bias, 100)
    torch.cuda.synchronize()
    assert got[0].cpu().numpy().tobytes() == want[0].cpu().numpy().tobytes() and got[1].cpu().numpy().tobytes() == want[1].cpu().numpy().tobytes()
    _same(got, pc.adc_expected(q, pq_book, codes, off, ids, probe, bias, 100))


@pytest.mark.parametrize("nq", [1, 32])
def test_graph_replay_equals_the_eager_call(cuda, nq):
    """The call captured with preallocated outputs and workspace, replayed on new queries: the eager call's bytes."""
    q, book, codes, off, ids, probe, bias = ac.random_index(60 + nq, 36, 16, 256, 2 * nq, 4000, 6, 3)
    k, longest = 20, int(np.diff(off).max())
    d = [_dev(cuda, a) for a in (book, codes, off, ids)]
    sq, sp, sb = _dev(cuda, q[:nq]), _dev(cuda, probe[:nq]), _dev(cuda, bias[:nq])
    out = (torch.empty((nq, k), dtype=torch.float32, device=cuda), torch.empty((nq, k), dtype=torch.int64, device=cuda))
    ws = torch.empty(dense.aq_scan_workspace_bytes(nq, 3, k, 36, 16, 256, 6, longest), dtype=torch.uint8, device=cuda)

    def call():
        return dense.aq_scan_topk(sq, d[0], d[1], d[2], d[3], longest, sp, sb, k, out=out, workspace=ws)

    call()                                           # loads the kernels, opts in to the dynamic LDS
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for part in (slice(0, nq), slice(nq, 2 * nq)):
        sq.copy_(_dev(cuda, q[part])), sp.copy_(_dev(cuda, probe[part])), sb.copy_(_dev(cuda, bias[part]))
        out[0].fill_(7.0), out[1].fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        eager = _run(cuda, q[part], book, codes, off, ids, probe[part], bias[part], k)
        _same(out, ac.aq_expected(q[part], book, codes, off, ids, probe[part], bias[part], k))
        assert eager[1].cpu().numpy().tobytes() == out[1].cpu().numpy().tobytes()


def test_two_runs_give_the_same_bytes_and_outputs_are_written_in_place(cuda):
    args = ac.random_index(41, 36, 16, 256, 70, 4000, 6, 3)
    a = _run(cuda, *args, 50)
    out = (torch.full((70, 50), 7.0, dtype=torch.float32, device=cuda), torch.full((70, 50), -7, dtype=torch.int64, device=cuda))
    b = _run(cuda, *args, 50, out=out)
    torch.cuda.synchronize()
    assert b[0] is out[0] and b[1] is out[1]
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()
