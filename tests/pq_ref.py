"""Product quantisation restated from the oracle's pieces (test helper, no tests here).

* `pq_encode`      -- oracle.rq.rq_encode on each column slice with a one-level codebook: the arithmetic of
                      mevi_pq_encode_f32 (sequential fmaf chain, lowest index on ties)
* `reconstruct`    -- pq.get_reconstruct_vector for 'pq' (MEVI/pq.py:768-784): concatenation of the chosen centroids
* `beam_search`    -- pq.beam_search, 'pq' branch (MEVI/pq.py:614-713): per level softmax(-dist(x_j, C[j])), the same
                      row for every beam, times the beam score, top-R over beams x K (all kept below R, (beam, code) order)
* `near_tie_sets`  -- per (row, subspace) the codes whose float64 distance lies within a relative `tol` of the minimum
"""
import numpy as np

from oracle import rq as orq


def pq_encode(x, codebook, return_neg_dist=False):
    x = np.asarray(x, dtype=np.float32)
    cb = np.asarray(codebook, dtype=np.float32)
    M, K, dsub = cb.shape
    codes = np.empty((x.shape[0], M), np.int32)
    nd = np.empty((x.shape[0], M, K), np.float32)
    for j in range(M):
        c, d = orq.rq_encode(x[:, j * dsub:(j + 1) * dsub], cb[j:j + 1], return_neg_dist=True)
        codes[:, j] = c[:, 0]
        nd[:, j] = d[:, 0]
    return (codes, nd) if return_neg_dist else codes


def reconstruct(codes, codebook):
    cb = np.asarray(codebook, dtype=np.float32)
    codes = np.asarray(codes)
    return np.concatenate([cb[j][codes[..., j]] for j in range(cb.shape[0])], axis=-1)


def beam_search(x, codebook, R):
    """(labels i32[n, R, M], scores f32[n, R]) with the score rows of `pq_encode(..., return_neg_dist=True)`."""
    x = np.asarray(x, dtype=np.float32)
    cb = np.asarray(codebook, dtype=np.float32)
    M, K, _ = cb.shape
    n = x.shape[0]
    _, nd = pq_encode(x, cb, return_neg_dist=True)
    scores = np.ones((n, 1), np.float32)
    labels = np.zeros((n, 1, 0), np.int32)
    for j in range(M):
        z = nd[:, j] - nd[:, j].max(-1, keepdims=True)
        p = np.exp(z)
        p = (p / p.sum(-1, keepdims=True)).astype(np.float32)
        flat = (scores[:, :, None] * p[:, None, :]).reshape(n, -1)
        nb = scores.shape[1]
        if R < nb * K:
            order = np.argsort(-flat, axis=1, kind="stable")[:, :R]
            prev, code = order // K, order % K
            scores = np.take_along_axis(flat, order, 1)
            labels = np.concatenate([np.take_along_axis(labels, prev[:, :, None], 1), code[:, :, None].astype(np.int32)], -1)
        else:
            scores = flat
            code = np.tile(np.arange(K), nb)
            labels = np.concatenate([np.repeat(labels, K, axis=1),
                                     np.broadcast_to(code[None, :, None], (n, nb * K, 1)).astype(np.int32)], -1)
    return labels, scores


def near_tie_sets(x, codebook, tol=1e-6):
    """bool [n, M, K]: code c of subspace j is within tol * (1 + min) of row i's smallest float64 distance."""
    x = np.asarray(x, dtype=np.float64)
    cb = np.asarray(codebook, dtype=np.float64)
    M, K, dsub = cb.shape
    out = np.empty((x.shape[0], M, K), bool)
    for j in range(M):
        d = ((x[:, None, j * dsub:(j + 1) * dsub] - cb[j][None]) ** 2).sum(-1)
        m = d.min(-1, keepdims=True)
        out[:, j] = d <= m + tol * (1.0 + m)
    return out


def codes_agree(got, want, ties):
    """Codes equal wherever a (row, subspace) has one nearest centroid; both inside the near-tie set elsewhere."""
    got, want = np.asarray(got), np.asarray(want)
    single = ties.sum(-1) == 1
    inset = np.take_along_axis(ties, got[..., None].astype(np.int64), -1)[..., 0]
    return bool(np.array_equal(got[single], want[single]) and inset.all())


def beams_agree(labels, scores, want_labels, want_scores, score_tol=1e-6, gap=1e-6):
    """Beam lists equal position by position wherever the reference's score is apart (> gap) from its neighbours;
    scores within score_tol everywhere (sorted lists, so a near-tie swap does not move a score)."""
    labels, want_labels = np.asarray(labels), np.asarray(want_labels)
    scores, want_scores = np.asarray(scores), np.asarray(want_scores)
    if labels.shape != want_labels.shape or np.abs(scores - want_scores).max() > score_tol:
        return False
    g = np.abs(np.diff(want_scores, axis=1)) > gap
    firm = np.concatenate([np.ones((len(g), 1), bool), g], 1) & np.concatenate([g, np.ones((len(g), 1), bool)], 1)
    return bool((labels == want_labels).all(-1)[firm].all())
