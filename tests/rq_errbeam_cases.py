"""Expected values of the residual quantiser's beam-search encoder (include/mevi_hip_rq_errbeam.h, mevi_amd/rqindex.py:encode_walk)
from existing oracle calls only, and the inputs its tests share.  No number here is a tolerance: the bar of the GPU tests is bit
equality.

`step_expected`   one level: err = -oracle.rq.rq_encode(rows, cent[None], return_neg_dist=True)[1] (the fmaf chain of the squared
                  differences, k ascending from +0), the Lo = min(L, B * K) smallest (err, b * K + c) by np.lexsort -- always sorted --
                  and the next rows by one np.float32 array subtraction.
`walk_expected`   M steps from B = 1, then the path of slot 0 (`codes_expected`).
`codes_expected`  the backtrack over (parent, code) traces.
`walk_float64`    a float64 restatement of the walk, for checking the reference where nothing is near a tie.
`aniso_corpus`    the seeded corpus of the quality condition: rows z * A with a decaying spectrum, and a greedy-trained codebook
                  (numpy Lloyd iterations from seeded rows, level by level on the greedy residual)."""
import numpy as np

from oracle import rq as orq


def step_expected(res_in, cent, L):
    """(parent u8 [n, Lo], code u8 [n, Lo], err f32 [n, Lo], res_out f32 [n, Lo, dim]) of one step."""
    res_in = np.ascontiguousarray(res_in, np.float32)
    cent = np.ascontiguousarray(cent, np.float32)
    n, B, dim = res_in.shape
    K = len(cent)
    Lo = min(int(L), B * K)
    if n == 0:
        return (np.zeros((0, Lo), np.uint8), np.zeros((0, Lo), np.uint8), np.zeros((0, Lo), np.float32), np.zeros((0, Lo, dim), np.float32))
    err = -orq.rq_encode(res_in.reshape(n * B, dim), cent[None], return_neg_dist=True)[1]
    err = err.reshape(n, B * K)
    assert err.dtype == np.float32 and not np.signbit(err).any()
    flat = np.broadcast_to(np.arange(B * K), err.shape)
    order = np.lexsort((flat, err), axis=-1)[:, :Lo]                  # err ascending, the lower b * K + c on ties
    parent, code = order // K, order % K
    res_out = np.take_along_axis(res_in, parent[:, :, None], axis=1) - cent[code]
    assert res_out.dtype == np.float32
    return parent.astype(np.uint8), code.astype(np.uint8), np.take_along_axis(err, order, axis=1), res_out


def codes_expected(parent, code, row_stride=None):
    """u8 [n, M] from per-level lists parent[j] / code[j] u8 [n, Lo_j] (or arrays [M, n, S]): p = 0; for j = M-1 .. 0: take
    code_j[i][p], then p = parent_j[i][p]."""
    M, n = len(parent), len(parent[0])
    out = np.zeros((n, M), np.uint8)
    p = np.zeros(n, np.int64)
    rows = np.arange(n)
    for j in range(M - 1, -1, -1):
        out[:, j] = np.asarray(code[j])[rows, p]
        p = np.asarray(parent[j])[rows, p].astype(np.int64)
    return out


def walk_expected(x, codebook, L, return_trace=False):
    """u8 [n, M]: the codes of the rows x f32 [n, dim] (already residuals to a coarse centroid where there is one) under a beam of L;
    with return_trace also (parents, codes, errs per level)."""
    cb = np.asarray(codebook, np.float32)
    cur = np.ascontiguousarray(x, np.float32)[:, None, :]
    parents, codes, errs = [], [], []
    for j in range(cb.shape[0]):
        p, c, e, cur = step_expected(cur, cb[j], L)
        parents.append(p)
        codes.append(c)
        errs.append(e)
    out = codes_expected(parents, codes)
    return (out, parents, codes, errs) if return_trace else out


def walk_float64(x, codebook, L):
    """(codes [n, M], smallest gap between a kept and the next candidate error relative to the error) in float64."""
    cb = np.asarray(codebook, np.float64)
    cur = np.asarray(x, np.float64)[:, None, :]
    n, (M, K, _) = len(x), cb.shape
    parents, codes, gap = [], [], np.inf
    for j in range(M):
        B = cur.shape[1]
        err = ((cur[:, :, None, :] - cb[j][None, None]) ** 2).sum(-1).reshape(n, B * K)
        order = np.argsort(err, axis=1, kind="stable")
        Lo = min(L, B * K)
        s = np.take_along_axis(err, order[:, :min(Lo + 1, B * K)], axis=1)
        if s.shape[1] > 1:
            gap = min(gap, float((np.diff(s, axis=1) / np.maximum(s[:, 1:], 1e-300)).min()))
        order = order[:, :Lo]
        parents.append(order // K)
        codes.append(order % K)
        cur = np.take_along_axis(cur, (order // K)[:, :, None], axis=1) - cb[j][order % K]
    return codes_expected(parents, codes), gap


def recon_error64(x, codebook, codes):
    """float64 [n]: ||x - sum_j codebook[j][code_j]||^2."""
    cb = np.asarray(codebook, np.float64)
    left = np.asarray(x, np.float64).copy()
    for j in range(cb.shape[0]):
        left -= cb[j][np.asarray(codes)[:, j]]
    return (left ** 2).sum(1)


def random_step(seed, n, B, dim, K, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, B, dim)) * scale).astype(np.float32), rng.standard_normal((K, dim)).astype(np.float32)


def random_trace(seed, M, n, Lo, S):
    """(parent, code) u8 [M, n, S] with parents < Lo in the first Lo slots and 255 (never to be reached) past them."""
    rng = np.random.default_rng(seed)
    parent = np.full((M, n, S), 255, np.uint8)
    code = rng.integers(0, 256, (M, n, S)).astype(np.uint8)
    parent[:, :, :Lo] = rng.integers(0, Lo, (M, n, Lo))
    return parent, code


def greedy_codebook(x, M, K, seed, iters=8):
    """f32 [M, K, dim]: level j = a few numpy Lloyd iterations from K seeded rows on the greedy residual of levels < j."""
    rng = np.random.default_rng(seed)
    res = np.array(x, np.float32, copy=True)
    book = []
    for _ in range(M):
        cent = res[rng.choice(len(res), K, replace=False)].copy()
        for _ in range(iters):
            lab = orq.rq_encode(res, cent[None])[:, 0]
            for c in range(K):
                if (lab == c).any():
                    cent[c] = res[lab == c].mean(0)
        lab = orq.rq_encode(res, cent[None])[:, 0]
        book.append(cent)
        res = res - cent[lab]
    return np.stack(book).astype(np.float32)


QUALITY = dict(seed=5, n=700, dim=36, M=12, K=16, decay=0.85)


def aniso_corpus(seed=QUALITY["seed"], n=QUALITY["n"], dim=QUALITY["dim"], M=QUALITY["M"], K=QUALITY["K"], decay=QUALITY["decay"]):
    """(x f32 [n, dim], codebook f32 [M, K, dim]): rows z * A, A = a random rotation of a spectrum decay^k, and a codebook trained
    greedily on them."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    A = (decay ** np.arange(dim))[:, None] * q
    x = (rng.standard_normal((n, dim)) @ A).astype(np.float32)
    return x, greedy_codebook(x, M, K, seed + 1)
