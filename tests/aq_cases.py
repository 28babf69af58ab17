"""Expected values of the additive-quantiser calls (include/mevi_hip_aq.h) from existing oracle calls only, and the small generators
their tests share.  No number here is a tolerance: the bar of the GPU tests is bit equality (scores as uint32, ids equal).

`aq_expected` restates the header:
  lut[j]  = the K chains <q, codebook[j][c]> over ALL dim columns: oracle.dense.ip_topk_exact(q, codebook[j], K) put back by
            centroid (`luts`; tests/test_rqindex_cpu.py holds it equal to oracle.dense.pair_dot, entry by entry, on a small case)
  score, probes, the clamp of a list, the result: those of the product quantiser's scan, so they are not written again:
            tests/ivfpq_cases.py:adc_expected is handed the query M times side by side and the codebook as M "subspaces" of dim
            columns -- its table of subspace j is then the chain <q, codebook[j][c]> (held equal to `luts` in the CPU test), and
            `adc_scores`, `clean_slots` and the lexsort are its own.
`residual_expected` is the numpy chain of mevi_rq_residual_f32, `chained_encode` the rule by which levels are encoded in groups."""
import numpy as np

from oracle import dense as odense
from oracle import rq as orq

import ivfpq_cases as pc
from ivfpq_cases import adc_scores, clean_slots  # noqa: F401  (the tests of this family use them under this module's name)


def luts(q, codebook):
    """f32 [nq, M, K]: one oracle call per level, every one of the K chains of all queries, sorted; put back by centroid."""
    q = np.ascontiguousarray(q, np.float32)
    cb = np.ascontiguousarray(codebook, np.float32)
    M, K, dim = cb.shape
    assert q.shape[1] == dim
    out = np.empty((len(q), M, K), np.float32)
    for j in range(M):
        s, c = odense.ip_topk_exact(q, cb[j], K)
        assert (np.sort(c, axis=1) == np.arange(K)).all()
        np.put_along_axis(out[:, j, :], c, s, axis=1)
    return out


def luts_by_pair_dot(q, codebook):
    """The same tables entry by entry: lut[i, j] = oracle.dense.pair_dot(q_i, codebook[j]).  For small cases."""
    q = np.ascontiguousarray(q, np.float32)
    cb = np.ascontiguousarray(codebook, np.float32)
    return np.stack([np.stack([odense.pair_dot(q[i], cb[j]) for j in range(cb.shape[0])]) for i in range(len(q))])


def as_product(q, codebook):
    """(q', codebook) with q' = the query M times side by side: the product-quantiser problem whose tables are this one's."""
    return np.ascontiguousarray(np.tile(np.asarray(q, np.float32), (1, np.asarray(codebook).shape[0]))), codebook


def aq_expected(q, codebook, codes, offsets, row_ids, probe, probe_score, k, max_list_len=None):
    """(scores f32 [nq, k], ids i64 [nq, k]) of mevi_aq_scan_topk_f32.  codebook f32 [M, K, dim]; the rest as adc_expected."""
    qq, cb = as_product(q, codebook)
    return pc.adc_expected(qq, cb, codes, offsets, row_ids, probe, probe_score, k, max_list_len)


def aq_float64(q, codebook, codes, bias):
    """Float64 scores of one query over rows `codes`: bias + <q, sum_j codebook[j][code_j]>, for checking the reference."""
    cb = np.asarray(codebook, np.float64)
    recon = sum(cb[j][codes[:, j]] for j in range(cb.shape[0]))
    return np.float64(bias) + recon @ np.asarray(q, np.float64)


def random_index(seed, dim, M, K, nq, nd, nlist, nprobe, lens=None, repeats=False):
    """tests/ivfpq_cases.py:random_index with a full-width codebook f32 [M, K, dim]: (q, codebook, codes list-major, offsets,
    row_ids = a permutation, probe, probe_score)."""
    # asked for M "subspaces" of dim columns, that generator draws a codebook of this shape; the query keeps its first dim columns
    q, codebook, codes, offsets, row_ids, probe, probe_score = pc.random_index(seed, dim * M, M, K, nq, nd, nlist, nprobe, lens, repeats)
    assert codebook.shape == (M, K, dim)
    return np.ascontiguousarray(q[:, :dim]), codebook, codes, offsets, row_ids, probe, probe_score


def residual_expected(x, codebook, codes):
    """((x - cb[0][code_0]) - cb[1][code_1]) - ...: np.float32 array subtractions in ascending level, codes clamped to [0, K)."""
    cb = np.asarray(codebook, np.float32)
    out = np.array(x, np.float32, copy=True)
    for g in range(cb.shape[0]):
        out = out - cb[g][np.clip(np.asarray(codes)[:, g], 0, cb.shape[1] - 1)]
        assert out.dtype == np.float32
    return out


def chained_encode(x, codebook, group=8):
    """i32 [n, M]: oracle.rq.rq_encode of `group` levels at a time, the residual of a group handed on by `residual_expected`."""
    cb = np.asarray(codebook, np.float32)
    x = np.array(x, np.float32, copy=True)
    parts = []
    for g in range(0, cb.shape[0], group):
        part = orq.rq_encode(x, cb[g:g + group])
        parts.append(part)
        x = residual_expected(x, cb[g:g + group], part)
    return np.concatenate(parts, axis=1)


def pq_as_aq(pq_codebook):
    """The additive codebook f32 [m, K, m * dsub] whose level j is the product codebook's subspace j in columns j * dsub ..., zero
    elsewhere: its tables are the product quantiser's (a chain over zeros adds +0 to +0 before and keeps the sum after)."""
    pq = np.asarray(pq_codebook, np.float32)
    m, K, dsub = pq.shape
    out = np.zeros((m, K, m * dsub), np.float32)
    for j in range(m):
        out[j, :, j * dsub:(j + 1) * dsub] = pq[j]
    return out
