"""The additive quantiser's lookup tables (mevi_aq_lut_f32 through dense.aq_lut) against tests/aq_cases.py: luts, which is built
from oracle calls only.  Bar: every entry identical as uint32 bits.  A table row does not depend on the other queries of the call, so
one reference of 257 queries per (M x K, dim) serves every query count: the first nq rows of it.  Query counts: 1, and one below, at
and one above every tile edge of the two kernels -- the 4 queries of a wave and the 16 of a workgroup of the few-query kernel, the 64
from which the matrix-core kernel is taken, its 128-query wave groups and its 256-query workgroups."""
import functools

import numpy as np
import pytest
import torch

import aq_cases as ac
from mevi_amd import dense, hip

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
NQ_MAX = dense.AQ_LUT_QUERY_TILE + 1
COUNTS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def _case(M, K, dim):
    rng = np.random.default_rng(1000 * M + 10 * K + dim)
    q = rng.standard_normal((NQ_MAX, dim)).astype(np.float32)
    book = rng.standard_normal((M, K, dim)).astype(np.float32)
    want = ac.luts(q, book)
    for a in (q, book, want):
        a.setflags(write=False)
    return q, book, want


def _same(got, want):
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("M,K", [(4, 1), (4, 3), (8, 16), (4, 256), (96, 256)])
@pytest.mark.parametrize("dim", [4, 36, 100, 768])
def test_tables_equal_the_oracle_chain_at_every_tile_edge(cuda, M, K, dim):
    """M x K: 4, 12 (a tile of codebook rows unfilled, odd), 128 (one matrix-core tile), 1024, 24576 (the 96 KiB table); dim below,
    across and many times the k slabs (32 columns on the matrix cores, 128 in the few-query kernel)."""
    assert COUNTS[-1] == NQ_MAX and {dense.AQ_LUT_FEW_QUERIES, dense.AQ_LUT_QUERY_TILE} <= set(COUNTS)
    q, book, want = _case(M, K, dim)
    dq, dbook = torch.from_numpy(np.array(q)).to(cuda), torch.from_numpy(np.array(book)).to(cuda)     # copies: the case is read-only
    counts = COUNTS if M * K * dim <= 1024 * 768 else (1, 17, 63, 64, 257)       # the largest tables: one count per path and edge
    for nq in counts:
        _same(dense.aq_lut(dq[:nq].contiguous(), dbook), want[:nq])


def test_a_row_does_not_depend_on_the_batch_or_the_kernel(cuda):
    """Query 0 alone (few-query kernel), among 64 and among 257 (matrix cores): the same bits; into a preallocated `out`."""
    q, book, want = _case(8, 16, 100)
    dq, dbook = torch.from_numpy(np.array(q)).to(cuda), torch.from_numpy(np.array(book)).to(cuda)     # copies: the case is read-only
    out = torch.full((64, 8, 16), 7.0, dtype=torch.float32, device=cuda)
    got = dense.aq_lut(dq[:64].contiguous(), dbook, out=out)
    assert got is out
    alone, all_ = dense.aq_lut(dq[:1].contiguous(), dbook), dense.aq_lut(dq, dbook)
    torch.cuda.synchronize()
    assert alone[0].cpu().numpy().tobytes() == out[0].cpu().numpy().tobytes() == all_[0].cpu().numpy().tobytes() == want[0].tobytes()
    assert dense.aq_lut(dq[:0].contiguous(), dbook).shape == (0, 8, 16)


@pytest.mark.parametrize("nq", [3, 70])
def test_signed_zeros_and_denormals_in_the_query(cuda, nq):
    """Queries of -0, +0, denormals of both signs and normal values against a codebook with zero rows, denormal entries and values
    that take a denormal product back into the normal range: no flush to zero on either kernel (3 queries: the few-query kernel; 70:
    the matrix cores), and the one sign the header gives up: a chain that ends in -0 is stored as +0."""
    rng = np.random.default_rng(5)
    dim, M, K = 36, 4, 8
    tiny = np.float32(1e-41)
    assert tiny != 0 and tiny < np.finfo(np.float32).tiny
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    q[0] = -0.0
    q[1] = np.where(np.arange(dim) % 2 == 0, tiny * 3, -tiny)
    q[2, ::3] = -0.0
    q[2, 1::3] = tiny * 3
    book = rng.standard_normal((M, K, dim)).astype(np.float32)
    book[0, 0] = 0.0
    book[0, 1] = -0.0
    book[1, 0] = tiny
    book[1, 1] = np.float32(2.0 ** 20)                  # denormal query x 2^20: normal again
    book[2, 0, 1:] = 0.0
    book[2, 0, 0] = np.float32(-1.0)                    # a single term: the chain is the product, then adds of signed zeros
    want = ac.luts(q, book)
    chains = ac.luts_by_pair_dot(q, book)             # a chain whose products all underflow ends in -0; the header stores it as +0,
    assert np.signbit(chains[chains == 0]).any() and not np.signbit(want[want == 0]).any() and (want == 0).sum() > 16    # as the oracle call does
    assert np.array_equal((chains + np.float32(0)).view(np.uint32), want.view(np.uint32))
    assert (np.abs(want[1, 1, 1]) > 0) and np.abs(want[1, 1, 1]) < np.finfo(np.float32).tiny * 2.0 ** 21       # denormals did count
    _same(dense.aq_lut(torch.from_numpy(q).to(cuda), torch.from_numpy(book).to(cuda)), want)


@pytest.mark.parametrize("nq", [2, 64])
@pytest.mark.parametrize("dim", [36, 768])
def test_a_codebook_row_of_flt_max_over_dim_neither_overflows_nor_reorders(cuda, nq, dim):
    """Rows of +-FLT_MAX / dim against queries of +-1: every partial sum of the chain stays finite, and a chain taken in another
    order (pairwise, or from the far end) rounds differently from the sequential one on the mixed-sign rows."""
    rng = np.random.default_rng(6)
    M, K = 4, 4
    big = np.float32(FLT_MAX / dim * (1 - 2.0 ** -12))   # below FLT_MAX / dim by more than the dim roundings of 2^-24 can add
    q = np.where(rng.random((nq, dim)) < 0.5, -1.0, 1.0).astype(np.float32)
    q[0] = 1.0
    book = (rng.random((M, K, dim)).astype(np.float32) * big).astype(np.float32)
    book[0, 0] = big                                     # all of one sign under q[0]: the sum climbs to ~FLT_MAX
    book[0, 1] = -big * np.float32(0.75)                # not down to -FLT_MAX itself: that value is the padding of the oracle call
    book[1] *= np.where(rng.random((K, dim)) < 0.5, -1.0, 1.0).astype(np.float32)
    want = ac.luts(q, book)
    assert np.isfinite(want).all() and abs(float(want[0, 0, 0])) > FLT_MAX * 0.99
    backwards = ac.luts(q[:, ::-1], book[:, :, ::-1])
    assert not np.array_equal(want, backwards)           # the order of the chain is visible in this data
    _same(dense.aq_lut(torch.from_numpy(q).to(cuda), torch.from_numpy(book).to(cuda)), want)


def test_refusals_on_the_device_leave_the_output_alone(cuda):
    """dim % 4, misaligned and null pointers: refused with the documented status, the output untouched."""
    L = hip.lib()
    q = torch.zeros((4, 40), dtype=torch.float32, device=cuda)
    book = torch.zeros((4, 8, 40), dtype=torch.float32, device=cuda)
    out = torch.full((4, 4, 8), 7.0, dtype=torch.float32, device=cuda)

    def call(qp, dim, bp, op, nq=4):
        return L.mevi_aq_lut_f32(qp, nq, dim, bp, 4, 8, op, hip.stream_ptr()), L.mevi_last_error().decode()

    for args, code, word in (((hip.ptr(q), 38, hip.ptr(book), hip.ptr(out)), -2, "dim=38"),
                             ((hip.ptr(q) + 4, 36, hip.ptr(book), hip.ptr(out)), -1, "align"),
                             ((hip.ptr(q), 36, hip.ptr(book) + 8, hip.ptr(out)), -1, "align"),
                             ((hip.ptr(q), 36, hip.ptr(book), hip.ptr(out) + 2), -1, "align"),
                             ((None, 40, hip.ptr(book), hip.ptr(out)), -1, "null"),
                             ((hip.ptr(q), 40, None, hip.ptr(out)), -1, "null"),
                             ((hip.ptr(q), 40, hip.ptr(book), None), -1, "null")):
        st, msg = call(*args)
        assert st == code and word in msg and msg.startswith("aq_lut:"), (args, st, msg)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(None, 40, None, None, nq=0)[0] == 0
