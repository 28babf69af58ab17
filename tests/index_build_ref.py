"""References for the offline index build (test helper, no tests here): numpy, float64 and the C oracle only.

* `cluster_means64`      -- per-cluster float64 sums / count, rounded once to f32 (what mevi_cluster_means_f32 approximates)
* `cluster_means_blocks` -- the (workgroups, rows per workgroup) split include/mevi_hip.h documents for that kernel
* `cluster_means_bound`  -- elementwise error bound of the documented reduction order (derivation below)
* `sum_sq_rtol`          -- relative bound of the f64 sum of squares (its summation depth)
* `rq_beam_search_chain` / `pq_beam_search_chain` -- pq.beam_search with the per-level scores taken from the oracle's
                            sequential fmaf chain (the arithmetic mevi_rq_neg_dist_f32 promises), softmax and product in float64
* `beams_agree_rel`      -- relative-gap comparison of two beam lists, returns the share of decidable ("firm") positions
* `clustered_inputs`     -- rows that are sums (rq) / concatenations (pq) of codebook entries plus noise, for which the
                            reference leaves most beam positions decidable

Constants of the beam comparison.  The device computes each level's softmax in f32 (expf, a 64-lane tree sum, a divide)
where the reference below works in float64 and rounds once per level.  How far f32 softmax arithmetic moves a beam score
was measured on the CPU: the same restatement with every softmax step in np.float32 (exp, sum, divide, product) against
the float64 one, over every (shape, R) of BEAM_CASES and PQ_BEAM_CASES --

    largest relative score difference, 'rq' cases: 7.08e-7      'pq' cases: 1.23e-6      (MEASURED_F32_SOFTMAX_RDIFF = 1.23e-6)

(tests/test_index_build_ref_cpu.py recomputes it and holds it to the recorded value.)  SCORE_RTOL = 4 x that maximum,
= 4.92e-6, GAP_RTOL = 4 x SCORE_RTOL = 1.97e-5; the margin covers the few ulp per level by which the device's expf / logf and summation order
differ from numpy's.
"""
import numpy as np

from oracle import rq as orq

U32 = 2.0 ** -24          # unit roundoff of f32
U64 = 2.0 ** -53

MEASURED_F32_SOFTMAX_RDIFF = 1.23e-6
SCORE_RTOL = 4 * MEASURED_F32_SOFTMAX_RDIFF      # 4.92e-6
GAP_RTOL = 4 * SCORE_RTOL                        # 1.97e-5
FIRM_SHARE_MIN = 0.85
MAX_CUT_EXCLUDED = 0.03       # largest share of rows beams_agree_rel may leave out for an undecidable top-R cut

# (n, dim, M, K) -> the beam widths the GPU tests run.  R comes from {1, 3, 10, K-1, K, K+4, 40, 260}, kept wherever
# R <= K**M and every top-R step stays inside the beam step's nb*K <= 16384.
BEAM_CASES = {
    (301, 64, 3, 16): (1, 3, 10, 15, 16, 20, 40, 260),      # 260: keep-all at levels 0 and 1 (16, 256), top-R at level 2
    (130, 768, 4, 32): (1, 3, 10, 31, 32, 36, 40, 260),     # 32, 36, 40, 260: keep-all at level 0, then top-R
    (67, 96, 2, 256): (1, 3, 10, 40),                       # R * 256 <= 16384
    (50, 32, 1, 8): (1, 3, 7, 8),                           # M = 1; R = 8 keeps everything
    (200, 100, 8, 4): (1, 3, 4, 8, 10, 40, 260),            # 40: keep-all at levels 0 and 1; 260: at levels 0..3
}
# spread ratio between consecutive levels of clustered_inputs.  With ratio 2 and GAP_RTOL these two shapes leave the
# reference alone below the 85 % firm share (60 % at (130, 768, 4, 32) R = 260, 42-64 % at (200, 100, 8, 4) R >= 3: flat
# softmax rows at the deep levels, many score pairs within 2e-5); the input changed, not the cap.
BEAM_RATIO = {(130, 768, 4, 32): 1.3, (200, 100, 8, 4): 1.3}
PQ_BEAM_CASES = {
    (301, 64, 4, 16): (1, 3, 10, 15, 16, 20, 40, 260),
    (67, 96, 2, 256): (1, 3, 10, 40),
}


# (n, dim, K) of the bit-for-bit cluster-means runs (integer-valued rows in [-8, 8]): every n edge at one K, the production
# LDS splits (K = 256 at dim 768: 64-column chunks, 12 passes; K = 4096: 4-column chunks; K = 100 and 1000: chunks that
# divide neither 16384 nor dim), dims below / at / above one chunk, 2 M rows (1954 rows per workgroup) at dim 32.
INT_MEANS_CASES = (
    (0, 100, 7), (1, 100, 7), (63, 100, 7), (64, 100, 7), (65, 100, 7), (4097, 100, 7), (65536, 100, 7), (65537, 100, 7),
    (2_000_000, 32, 7), (2_000_000, 32, 256), (2_000_000, 32, 1),
    (65537, 768, 256), (4097, 260, 4096), (65537, 768, 100),
    (1, 1, 1), (4097, 1, 1), (65, 3, 7), (4097, 4, 100), (64, 4, 1000), (65536, 3, 100), (65536, 256, 256),
    (65536, 260, 256), (4097, 1028, 1000), (65537, 260, 1000), (63, 1028, 4096), (65537, 1, 4096), (65, 768, 256),
    (4097, 100, 1), (65537, 1028, 7),
)


# ---- cluster means ---------------------------------------------------------------------------------------------------------

def cluster_means_blocks(n):
    """(nb, P): mevi_cluster_means_f32 splits the rows over nb = min(1024, ceil(n / 64)) workgroups (at least one), each
    owning P = ceil(n / nb) consecutive rows (the last ones fewer, possibly none)."""
    nb = min(1024, max(1, -(-n // 64)))
    return nb, -(-n // nb)


def _by_cluster(labels, K):
    labels = np.asarray(labels).reshape(-1)
    order = np.argsort(labels, kind="stable")
    counts = np.bincount(labels, minlength=K).astype(np.int64)
    assert len(counts) == K, "label out of range"
    return order, counts, np.concatenate([[0], np.cumsum(counts)])


def _cluster_sums64(x, labels, K, fn, rows=32768):
    """float64 [K, dim]: sum over the rows of every cluster of fn(x) (x converted to float64 first), a slab at a time."""
    order, counts, start = _by_cluster(labels, K)
    out = np.zeros((K, x.shape[1]), np.float64)
    for k in np.nonzero(counts)[0]:
        idx = order[start[k]:start[k + 1]]
        for a in range(0, len(idx), rows):
            out[k] += fn(x[idx[a:a + rows]].astype(np.float64)).sum(0)
    return out, counts


def cluster_means64(x, labels, K, old=None, return_f64=False):
    """(means f32 [K, dim], counts int64 [K], sum ||x||^2 as a float64): float64 sums per cluster, divided by the count,
    rounded once to f32; an empty cluster takes old[k] (0 without `old`).  `return_f64` appends the unrounded means."""
    x = np.asarray(x, dtype=np.float32)
    s, counts = _cluster_sums64(x, labels, K, lambda v: v)
    m64 = np.zeros_like(s) if old is None else np.asarray(old, dtype=np.float32).astype(np.float64).copy()
    full = counts > 0
    m64[full] = s[full] / counts[full, None].astype(np.float64)
    sumsq = 0.0
    for a in range(0, len(x), 32768):
        sumsq += float((x[a:a + 32768].astype(np.float64) ** 2).sum())
    out = (m64.astype(np.float32), counts, np.float64(sumsq))
    return out + (m64,) if return_f64 else out


def cluster_means_bound(x, labels, K, n):
    """float64 [K, dim]: bound on |kernel mean - exact mean| for real-valued data,

        ((P - 1) * 2^-24 * sum_{i in k} |x[i, c]|) / cnt_k  +  2^-24 * |mean[k, c]|,     P = cluster_means_blocks(n)[1].

    Derivation, from the reduction order the header documents.  Stage 1: a workgroup adds its rows of cluster k to an f32
    accumulator that starts at 0, one after the other, in row order.  With m_b such rows the first addition is exact and the
    other m_b - 1 round, so (Higham, Accuracy and Stability, 4.2, to first order in u = 2^-24) the block sum is off by at
    most (m_b - 1) u sum_{i in block, k} |x[i, c]| <= (P - 1) u sum_{i in block, k} |x[i, c]|.  Stage 2 adds the block sums
    in float64: its own error, nb * 2^-53 of the same magnitude, is 2^-29 u per block and is left out.  Summed over the
    blocks and divided by the count this is the first term.  The second term is the one rounding of the quotient to f32;
    the comparison is therefore made with the UNROUNDED float64 mean (`cluster_means64(..., return_f64=True)`).  Empty
    clusters copy `old`: bound 0."""
    x = np.asarray(x, dtype=np.float32)
    assert x.shape[0] == n
    P = cluster_means_blocks(n)[1]
    sabs, counts = _cluster_sums64(x, labels, K, np.abs)
    ssum, _ = _cluster_sums64(x, labels, K, lambda v: v)
    cnt = np.maximum(counts, 1)[:, None].astype(np.float64)
    bound = (max(P - 1, 0) * U32 * sabs) / cnt + U32 * np.abs(ssum / cnt)
    bound[counts == 0] = 0.0
    return bound


def cluster_means_chunk(K):
    """Columns per LDS table of the kernel: min(256, 16384 // K)."""
    return min(256, 16384 // K)


def sum_sq_rtol(n, dim, K):
    """Relative bound of the kernel's sum of squares.  Every term is positive and every operation is float64: a thread adds
    at most P * ceil(dim / chunk) squares one by one, a 256-leaf tree (8 levels) joins the threads, the finish kernel adds
    the nb block sums in order -- a summation of depth P * ceil(dim / chunk) + 8 + nb, each step within 2^-53 relative."""
    nb, P = cluster_means_blocks(n)
    return (P * -(-dim // cluster_means_chunk(K)) + 8 + nb) * U64


# ---- beam search -----------------------------------------------------------------------------------------------------------

def _neg_dist(rows, level_book):
    return orq.rq_encode(rows, level_book[None], return_neg_dist=True)[1][:, 0]


def _beam_chain(x, cb, R, pq, dt):
    x = np.ascontiguousarray(x, dtype=np.float32)
    cb = np.ascontiguousarray(cb, dtype=np.float32)
    M, K, d = cb.shape
    n = x.shape[0]
    scores = np.ones((n, 1), np.float32)
    labels = np.zeros((n, 1, 0), np.int32)
    resid = x[:, None, :]                                       # 'rq': [n, nb, dim]
    cut = np.full(n, np.inf)
    for j in range(M):
        nb = scores.shape[1]
        if pq:
            nd = np.broadcast_to(_neg_dist(x[:, j * d:(j + 1) * d], cb[j])[:, None, :], (n, nb, K))
        else:
            nd = _neg_dist(resid.reshape(n * nb, d), cb[j]).reshape(n, nb, K)
        z = nd.astype(dt) - nd.max(-1, keepdims=True).astype(dt)
        e = np.exp(z)
        p = e / e.sum(-1, keepdims=True, dtype=dt)
        flat = (scores.astype(dt)[:, :, None] * p).astype(np.float32).reshape(n, nb * K)
        if R < nb * K:
            order = np.argsort(-flat, axis=1, kind="stable")            # ties: lower beam * K + code first
            kept, nxt = np.take_along_axis(flat, order[:, R - 1:R], 1)[:, 0], np.take_along_axis(flat, order[:, R:R + 1], 1)[:, 0]
            with np.errstate(divide="ignore", invalid="ignore"):
                cut = np.minimum(cut, np.where(kept > 0, (kept.astype(np.float64) - nxt) / kept, 0.0))
            order = order[:, :R]
            parent, code = order // K, order % K
            scores = np.take_along_axis(flat, order, 1)
        else:
            parent = np.broadcast_to(np.repeat(np.arange(nb), K)[None], (n, nb * K))
            code = np.broadcast_to(np.tile(np.arange(K), nb)[None], (n, nb * K))
            scores = flat
        labels = np.concatenate([np.take_along_axis(labels, parent[:, :, None], 1), code[:, :, None].astype(np.int32)], -1)
        if j != M - 1 and not pq:
            resid = np.take_along_axis(resid, parent[:, :, None], 1) - cb[j][code]      # f32
    return labels, scores, cut


def rq_beam_search_chain(x, cb, R, softmax_dtype=np.float64, return_cut_gap=False):
    """oracle.rq.rq_beam_search with the score rows of oracle.rq.rq_encode(resid, cb[j:j+1], return_neg_dist=True) -- the
    sequential fmaf chain -- the softmax and the product with the beam score in `softmax_dtype` (float64), rounded to f32
    per level, ordering stable on beam * K + code, residual hand-down resid[parent] - cb[j][code] in f32.
    Returns (labels i32 [n, R', M], scores f32 [n, R']); `return_cut_gap` appends, per row, the smallest relative gap
    between the last kept and the first dropped candidate over the top-R steps (inf when nothing was ever dropped): a row
    whose gap is below the comparison's `gap_rtol` has a beam SET the arithmetic does not decide."""
    lab, sc, cut = _beam_chain(x, cb, R, False, softmax_dtype)
    return (lab, sc, cut) if return_cut_gap else (lab, sc)


def pq_beam_search_chain(x, cb, R, softmax_dtype=np.float64, return_cut_gap=False):
    """The 'pq' twin: level j scores column slice j of the row against cb[j] (f32 [M, K, dsub]), the same score row for
    every beam, no residual."""
    lab, sc, cut = _beam_chain(x, cb, R, True, softmax_dtype)
    return (lab, sc, cut) if return_cut_gap else (lab, sc)


def beams_agree_rel(labels, scores, want_labels, want_scores, score_rtol, gap_rtol, cut_gap=None):
    """(agree, firm share).  agree: equal shapes, |score - want| <= score_rtol * want everywhere, and labels equal at
    every firm position -- one whose reference score differs from both neighbours in the (descending) list by more than
    gap_rtol * score.  In kept-everything lists ((beam, code) order) the neighbours are those of the sorted scores.
    `cut_gap` (per row, from `*_beam_search_chain(..., return_cut_gap=True)`): a row where some top-R step dropped a
    candidate within gap_rtol of the last one it kept has no decidable beam SET -- a swap there changes which residuals the
    deeper levels score, so neither its labels nor its scores are comparable; such rows are left out of both checks and
    every position of theirs counts as not firm (the firm share the callers hold to FIRM_SHARE_MIN pays for them), and
    more than MAX_CUT_EXCLUDED of the rows left out is an error of the inputs (AssertionError), not a pass."""
    labels, want_labels = np.asarray(labels), np.asarray(want_labels)
    scores, want = np.asarray(scores, dtype=np.float64), np.asarray(want_scores, dtype=np.float64)
    if labels.shape != want_labels.shape or scores.shape != want.shape:
        return False, 0.0
    order = np.argsort(-want, axis=1, kind="stable")
    w = np.take_along_axis(want, order, 1)
    g = np.abs(np.diff(w, axis=1))
    one = np.ones((len(w), 1), bool)
    firm_sorted = np.concatenate([one, g > gap_rtol * w[:, 1:]], 1) & np.concatenate([g > gap_rtol * w[:, :-1], one], 1)
    firm = np.empty_like(firm_sorted)
    np.put_along_axis(firm, order, firm_sorted, 1)
    rows = np.ones(len(w), bool) if cut_gap is None else np.asarray(cut_gap) > gap_rtol
    assert (~rows).mean() <= MAX_CUT_EXCLUDED, f"{int((~rows).sum())} of {len(rows)} rows have an undecidable top-R cut"
    firm &= rows[:, None]
    share = float(firm.mean()) if firm.size else 1.0
    ok_scores = bool((np.abs(scores - want) <= score_rtol * np.abs(want))[rows].all())
    ok_labels = bool((labels == want_labels).all(-1)[firm].all())
    return ok_scores and ok_labels, share


def clustered_inputs(n, dim, M, K, seed, pq=False, ratio=2.0):
    """(x f32 [n, dim], codebook f32 [M, K, dim]) with s = dim ** -0.5, cb[j] = N(0, 1) * 2 s / ratio ** j and
    x = sum_j cb[j][pick[:, j]] + 0.5 * s * ratio ** -(M - 1) * N(0, 1): every level has one clearly nearest centroid, the
    runners-up are spread out and no product probability underflows.  (ratio 2 halves the spread per level: by level 7
    the K score columns differ by 5e-4 and the softmax is flat -- deep trees take a smaller ratio, see BEAM_RATIO.)
    pq: codebook f32 [M, K, dim // M], every subspace like level 0 of the above (s = dsub ** -0.5, noise 0.5 s)."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, K, size=(n, M))
    if pq:
        dsub = dim // M
        s = dsub ** -0.5
        cb = (rng.standard_normal((M, K, dsub)) * 2 * s).astype(np.float32)
        x = np.concatenate([cb[j][pick[:, j]] for j in range(M)], 1) + 0.5 * s * rng.standard_normal((n, M * dsub))
        return x.astype(np.float32), cb
    s = dim ** -0.5
    cb = np.stack([rng.standard_normal((K, dim)) * 2 * s / ratio ** j for j in range(M)]).astype(np.float32)
    x = sum(cb[j][pick[:, j]] for j in range(M)) + 0.5 * s * ratio ** -(M - 1) * rng.standard_normal((n, dim))
    return x.astype(np.float32), cb


def beam_case_inputs(shape, pq=False):
    """The (x, codebook) every test runs for a case of BEAM_CASES / PQ_BEAM_CASES."""
    n, dim, M, K = shape
    return clustered_inputs(n, dim, M, K, 1000 + sum(shape), pq=pq, ratio=1.0 if pq else BEAM_RATIO.get(shape, 2.0))
