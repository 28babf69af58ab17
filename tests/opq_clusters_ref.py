"""ProductQuantization('opq') restated in numpy from the oracle's pieces (test helper, no tests here): a product quantiser behind a
rotation (MEVI/pq.py:259-279, 629-630, 775-783).

* `rotate`       -- y = chain(x, R): `opq_cases.rotate_expected`, the oracle's sequential fmaf chain per output (x @ R.T)
* `encode`       -- `pq_ref.pq_encode` of the rotated rows: the arithmetic of mevi_opq_encode_f32
* `beam_search`  -- `pq_ref.beam_search` of the rotated rows
* `reconstruct`  -- the concatenated centroids, then `@ R` as the same chain over the rows of R.T (back in the input space)
* `hadamard_rotation` / `exact_case` -- the fixtures of tools/capture_goldens_opq.py: a rotation and rows for which every product
  is exact in f32 under any summation order, so that a BLAS matmul and the chain give the same bits
"""
import numpy as np

import opq_cases
import pq_ref


def rotate(x, R):
    return opq_cases.rotate_expected(np.ascontiguousarray(x, np.float32), np.ascontiguousarray(R, np.float32))


def encode(x, R, codebook):
    return pq_ref.pq_encode(rotate(x, R), codebook)


def beam_search(x, R, codebook, nbeam):
    return pq_ref.beam_search(rotate(x, R), codebook, nbeam)


def reconstruct(codes, R, codebook):
    vectors = pq_ref.reconstruct(codes, codebook)
    flat = rotate(vectors.reshape(-1, vectors.shape[-1]), np.ascontiguousarray(np.asarray(R, np.float32).T))
    return flat.reshape(vectors.shape)


def hadamard_rotation(dim, block, rng):
    """f32 [dim, dim] orthonormal: block-diagonal normalised Hadamard blocks of size `block` = 4^p (entries +-2^-p), rows and
    columns permuted and rows signed.  Every entry is a power of two: products with dyadic rows are exact."""
    p = int(round(np.log(block) / np.log(4)))
    assert 4 ** p == block and dim % block == 0
    H = np.ones((1, 1))
    while len(H) < block:
        H = np.block([[H, H], [H, -H]])
    H = H * 2.0 ** -p
    R = np.zeros((dim, dim))
    for b in range(0, dim, block):
        R[b:b + block, b:b + block] = H
    R = R[rng.permutation(dim)][:, rng.permutation(dim)] * rng.choice([-1.0, 1.0], size=(dim, 1))
    assert np.array_equal(R @ R.T, np.eye(dim))
    return R.astype(np.float32)


def exact_case(M, bits, dim, n, block, seed, pool=40, scale=0.25, noise=0.06):
    """(X, R, C): centroids on multiples of 2^-8, rotated rows Y on multiples of 2^-6 near the centroids of `pool` code paths (so
    clusters have several members; scale 0.25: distances of a few units, one f32 ulp moves a beam probability by ~1e-7),
    X = Y R -- exact, and X R^T = Y exactly under any summation order."""
    rng = np.random.default_rng(seed)
    K, dsub = 1 << bits, dim // M
    C = (np.round(scale * rng.standard_normal((M, K, dsub)) * 256) / 256).astype(np.float32)
    R = hadamard_rotation(dim, block, rng)
    paths = rng.integers(0, K, size=(pool, M))
    Y = pq_ref.reconstruct(paths[rng.integers(0, pool, size=n)], C) + noise * rng.standard_normal((n, dim))
    Y = (np.round(Y * 64) / 64).astype(np.float32)
    X = (Y.astype(np.float64) @ R.astype(np.float64)).astype(np.float32)
    assert np.array_equal(X.astype(np.float64) @ R.astype(np.float64).T, Y.astype(np.float64))
    return X, R, C
