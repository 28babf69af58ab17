"""GPU: mevi_opq_encode_f32 (csrc/opq_encode.hip) bit for bit against the on-device composition it replaces --
mevi_opq_rotate_rows_f32 (plain form) then mevi_pq_encode_f32 -- and, at the small cases, against the CPU restatement from the
oracle's chains (tests/opq_clusters_ref.py).  R is `opq.random_rotation`: not exactly representable, so a wrong summation order
of the rotation shows in the codes' distances."""
import numpy as np
import pytest
import torch

import opq_clusters_ref as oref

pytestmark = pytest.mark.gpu
UNSUPPORTED = -2


def _case(dim, M, K, n, seed=None):
    from mevi_amd import opq

    rng = np.random.default_rng(seed if seed is not None else dim * 31 + M * 7 + K + n)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    R = opq.random_rotation(dim, 5 + dim).astype(np.float32)
    cb = rng.standard_normal((M, K, dim // M)).astype(np.float32)
    return x, R, cb


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _composition(x, R, cb):
    from mevi_amd import dense, rq

    return rq.pq_encode(dense.opq_rotate_rows(x, None, None, None, R, mode="fused"), cb)


def _fused(x, R, cb, codes=None):
    from mevi_amd import hip

    n, dim = x.shape
    M, K, dsub = cb.shape
    if codes is None:
        codes = torch.full((n, M), -1, dtype=torch.int32, device=x.device)
    st = hip.lib().mevi_opq_encode_f32(hip.ptr(x), n, dim, hip.ptr(R), hip.ptr(cb), M, K, dsub, hip.ptr(codes), hip.stream_ptr())
    hip.check(st, "mevi_opq_encode_f32")
    return codes


CASES = [
    # dim, M, K, n, also against the CPU restatement
    (64, 4, 32, 1, True), (64, 4, 32, 127, True), (64, 4, 32, 128, True), (64, 4, 32, 129, True),      # row tails
    (64, 4, 32, 257, True), (64, 4, 32, 300, True),                                                     # ... a second workgroup
    (768, 4, 32, 300, True),        # the production shape: a 192-wide subspace across three column tiles
    (768, 32, 256, 130, True),      # many narrow subspaces, four passes of eight
    (44, 11, 16, 257, True),        # dim no multiple of the 32-wide k slab, dsub 4
    (64, 4, 20, 200, False),        # centroid-chunk tail
    (64, 4, 1, 200, False),         # a single centroid
    (128, 8, 64, 260, False),       # the 128-column main loop
    (96, 3, 40, 140, False),        # two chunks, the second a tail; one k slab of 32
    (1024, 8, 16, 100, False),      # the widest fused dim: eight passes of one 128-wide subspace
    (320, 4, 32, 70, False),        # dsub 80: two subspaces per 192-column pass, three k slabs with a tail
]


@pytest.mark.parametrize("dim,M,K,n,cpu", CASES)
def test_fused_codes_equal_the_composition_bit_for_bit(cuda, dim, M, K, n, cpu):
    from mevi_amd import hip

    assert hip.lib().mevi_opq_encode_fused(dim, M, K, dim // M) == 1
    xh, Rh, ch = _case(dim, M, K, n)
    x, R, cb = _dev(cuda, xh, Rh, ch)
    got = _fused(x, R, cb).cpu().numpy()
    want = _composition(x, R, cb).cpu().numpy()
    assert got.min() >= 0 and got.max() < K
    assert np.array_equal(got, want)
    if cpu:
        assert np.array_equal(got, oref.encode(xh, Rh, ch))


def test_widest_dim_takes_the_composition_through_encode(cuda):
    from mevi_amd import hip, rq

    dim, M, bits, n = 4096, 32, 5, 130
    assert hip.lib().mevi_opq_encode_fused(dim, M, 1 << bits, dim // M) == 0
    xh, Rh, ch = _case(dim, M, 1 << bits, n)
    x, R, cb = _dev(cuda, xh, Rh, ch)
    pq = rq.ProductQuantization("opq", M, bits, "l2", dim, device=cuda)
    pq.load_codebook(ch)
    pq.load_rotation(Rh)
    assert torch.equal(pq._encode(x), _composition(x, R, cb))


def test_outside_the_fused_envelope(cuda):
    from mevi_amd import hip, rq

    dim, M, bits, n = 1024, 2, 5, 70
    xh, Rh, ch = _case(dim, M, 1 << bits, n)
    x, R, cb = _dev(cuda, xh, Rh, ch)
    codes = torch.full((n, M), -1, dtype=torch.int32, device=cuda)
    st = hip.lib().mevi_opq_encode_f32(hip.ptr(x), n, dim, hip.ptr(R), hip.ptr(cb), M, 1 << bits, dim // M, hip.ptr(codes),
                                       hip.stream_ptr())
    assert st == UNSUPPORTED and "dsub=512" in hip.lib().mevi_last_error().decode()
    torch.cuda.synchronize()
    assert (codes == -1).all()
    pq = rq.ProductQuantization("opq", M, bits, "l2", dim, device=cuda)
    pq.load_codebook(ch)
    pq.load_rotation(Rh)
    assert torch.equal(pq._encode(x), _composition(x, R, cb))


def test_duplicate_centroids_and_nan_rows(cuda):
    dim, M, K, n = 64, 4, 32, 200
    xh, Rh, ch = _case(dim, M, K, n, seed=3)
    ch[:, 7] = ch[:, 3]                 # exact distance ties: the lowest index wins
    ch[:, 30] = ch[:, 11]
    ch[2, 20:] = ch[2, 19]
    xh[12, 5] = np.nan                  # one NaN reaches every rotated column: all-zero codes
    xh[13] = np.nan
    x, R, cb = _dev(cuda, xh, Rh, ch)
    got = _fused(x, R, cb).cpu().numpy()
    assert np.array_equal(got, _composition(x, R, cb).cpu().numpy())
    assert not np.isin(got, [7, 30]).any() and not (got[:, 2] > 19).any()
    assert (got[12] == 0).all() and (got[13] == 0).all()
    keep = np.ones(n, bool)
    keep[[12, 13]] = False
    assert np.array_equal(got[keep], oref.encode(xh[keep], Rh, ch))


def test_rows_of_codes_past_n_are_untouched(cuda):
    dim, M, K, n, pad = 64, 4, 32, 130, 300
    xh, Rh, ch = _case(dim, M, K, pad)
    x, R, cb = _dev(cuda, xh, Rh, ch)
    codes = torch.full((pad, M), -7, dtype=torch.int32, device=cuda)
    _fused(x[:n], R, cb, codes=codes)
    assert (codes[n:] == -7).all()
    assert torch.equal(codes[:n], _composition(x[:n].contiguous(), R, cb))


def test_side_stream_and_captured_graph(cuda):
    dim, M, K, n = 768, 4, 32, 300
    xh, Rh, ch = _case(dim, M, K, n)
    x, R, cb = _dev(cuda, xh, Rh, ch)
    want = _composition(x, R, cb)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        got = _fused(x, R, cb)
    side.synchronize()
    assert torch.equal(got, want)
    codes = torch.full((n, M), -1, dtype=torch.int32, device=cuda)
    _fused(x, R, cb, codes=codes)        # the first call sets the kernel's attribute outside the capture
    torch.cuda.synchronize()
    codes.fill_(-1)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _fused(x, R, cb, codes=codes)
    for _ in range(2):
        codes.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(codes, want)
    x.copy_(x.flip(0))                   # the graph reads the buffers, not a snapshot
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(codes, want.flip(0))
