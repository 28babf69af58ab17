"""The residual a greedy encoder hands from one group of levels to the next (mevi_rq_residual_f32 through dense.rq_residual) against
the numpy chain of tests/aq_cases.py: residual_expected, and the encoder `rqindex.encode` chains out of it against
oracle.rq.rq_encode over ALL levels.  Bar: residuals identical as uint32 bits, codes equal."""
import numpy as np
import pytest
import torch

import aq_cases as ac
from mevi_amd import dense, rq, rqindex
from oracle import rq as orq

pytestmark = pytest.mark.gpu


def _case(seed, n, dim, G, K, stride=None):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    book = rng.standard_normal((G, K, dim)).astype(np.float32)
    codes = rng.integers(0, K, size=(n, G if stride is None else stride)).astype(np.int32)
    return x, book, codes


def _same(got, want):
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("G", [1, 3, 8])
@pytest.mark.parametrize("K", [1, 256])
@pytest.mark.parametrize("dim", [4, 36, 768])
def test_residual_equals_the_numpy_chain_in_and_out_of_place(cuda, G, K, dim):
    for n in (0, 1, 1000):
        x, book, codes = _case(G * 1000 + K + dim + n, n, dim, G, K)
        want = ac.residual_expected(x, book, codes)
        dx, dbook, dcodes = (torch.from_numpy(a).to(cuda) for a in (x, book, codes))
        out = dense.rq_residual(dx, dbook, dcodes)
        assert out.data_ptr() != dx.data_ptr() or n == 0
        _same(out, want)
        _same(dx, x)                                 # out of place: the input is left alone
        back = dense.rq_residual(dx, dbook, dcodes, out=dx)
        assert back is dx
        _same(dx, want)                              # in place


def test_a_code_stride_above_the_levels_and_a_column_slice(cuda):
    """codes as columns 8..11 of a wider array (stride 16), and as the first 3 columns of rows of 5: only the G levels are read."""
    x, book, wide = _case(5, 700, 36, 4, 16, stride=16)
    dx, dbook, dwide = (torch.from_numpy(a).to(cuda) for a in (x, book, wide))
    _same(dense.rq_residual(dx, dbook, dwide[:, 8:12]), ac.residual_expected(x, book, wide[:, 8:12]))
    x, book, rows5 = _case(6, 700, 36, 3, 16, stride=5)
    rows5[:, 3:] = 1 << 30                           # what lies behind the levels is never an index
    dx, dbook, d5 = (torch.from_numpy(a).to(cuda) for a in (x, book, rows5))
    _same(dense.rq_residual(dx, dbook, d5), ac.residual_expected(x, book, rows5[:, :3]))


def test_codes_out_of_range_subtract_the_first_or_the_last_centroid(cuda):
    """include/mevi_hip_aq.h: a code < 0 subtracts codebook[g][0], a code >= K subtracts codebook[g][K - 1]."""
    x, book, codes = _case(7, 300, 36, 3, 10)
    codes[::5, 0] = -1
    codes[1::5, 1] = 10
    codes[2::5, 2] = np.iinfo(np.int32).max
    codes[3::5, 0] = np.iinfo(np.int32).min
    clamped = np.clip(codes, 0, 9)
    assert (clamped != codes).sum() >= 200
    want = ac.residual_expected(x, book, codes)
    assert np.array_equal(want, ac.residual_expected(x, book, clamped))
    dx, dbook, dcodes = (torch.from_numpy(a).to(cuda) for a in (x, book, codes))
    _same(dense.rq_residual(dx, dbook, dcodes), want)


@pytest.mark.parametrize("dim", [128, 36])
@pytest.mark.parametrize("M", [4, 12, 16])
def test_chained_device_encode_equals_the_oracle_over_all_levels(cuda, M, dim):
    """`rqindex.encode` (groups of 8 levels through rq.rq_encode, the residual between them in place) against oracle.rq.rq_encode of
    the whole codebook: dim 128 takes the matrix-core encoder, dim 36 the exact kernel; duplicate centroids: the lowest index wins."""
    rng = np.random.default_rng(M * 10 + dim)
    n, K = 1500, 256 if dim == 128 else 40
    x = rng.standard_normal((n, dim)).astype(np.float32)
    book = (rng.standard_normal((M, K, dim)) * (0.75 ** np.arange(M))[:, None, None]).astype(np.float32)
    book[:, K - 1] = book[:, 0]
    book[M - 1, K // 2] = book[M - 1, 1]
    want = orq.rq_encode(x, book)
    assert (want != K - 1).all() and np.array_equal(want, ac.chained_encode(x, book, 8))
    dx, dbook = torch.from_numpy(x).to(cuda), torch.from_numpy(book).to(cuda)
    rq.rq_encode(dx[:64].contiguous(), dbook[:min(M, 8)].contiguous())
    assert rq._LAST_ENCODE["path"] == ("fast" if dim == 128 else "exact")
    got = rqindex.encode(dx, None, None, None, dbook, chunk=600)        # three chunks, the last one short
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and got.shape == (n, M)
    np.testing.assert_array_equal(got.cpu().numpy().astype(np.int32), want)
    _same(dx, x)                                     # the corpus rows are never written
    # ... and as residuals to list centroids, rows in list order
    cent = rng.standard_normal((5, dim)).astype(np.float32)
    list_of = rng.integers(0, 5, size=n).astype(np.int32)
    order = np.argsort(list_of, kind="stable")
    got = rqindex.encode(dx, torch.from_numpy(order).to(cuda), torch.from_numpy(list_of).to(cuda), torch.from_numpy(cent).to(cuda), dbook,
                         chunk=600)
    np.testing.assert_array_equal(got.cpu().numpy().astype(np.int32), orq.rq_encode(x[order] - cent[list_of[order]], book))
