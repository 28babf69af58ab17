"""Reference of the refine call (include/mevi_hip_refine.h: mevi_refine_topk_f32) -- numpy and the oracle only."""
import numpy as np

from oracle import dense as odense

FLT_MAX = np.finfo(np.float32).max


def refine_expected(q, docs, cand, k):
    """(scores f32 [nq, k], ids i64 [nq, k], nvalid i32 [nq]) the call must return, bit for bit.

    Per query: the candidates with an id inside [0, len(docs)) sorted by ascending id, repeats kept, scored by
    `oracle.dense.ip_topk_exact(q[b:b+1], docs[valid], n_valid)` -- the pinned sequential chain, ties by ascending position, which
    after the sort is ascending id --, the positions mapped back to ids, truncated to k, padded with -FLT_MAX / -1."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    docs = np.ascontiguousarray(docs, dtype=np.float32)
    cand = np.asarray(cand, dtype=np.int64)
    nq = q.shape[0]
    out_s = np.full((nq, k), -FLT_MAX, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    nvalid = np.zeros(nq, np.int32)
    for b in range(nq):
        valid = np.sort(cand[b][(cand[b] >= 0) & (cand[b] < docs.shape[0])])
        nvalid[b] = len(valid)
        if len(valid) == 0:
            continue
        s, pos = odense.ip_topk_exact(q[b:b + 1], docs[valid], len(valid))
        n = min(k, len(valid))
        out_s[b, :n] = s[0, :n]
        out_i[b, :n] = valid[pos[0, :n]]
    return out_s, out_i, nvalid
