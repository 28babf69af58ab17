"""The kernels that turn beams into ranked documents, at their limits: the segmented sorts (csrc/rerank.hip, incl. the
> 64 KiB LDS opt-in of segments above 8192 entries), the row softmax and the beam step in all its modes and its
tree form (csrc/beam.hip), pair_dot at awkward dims and strides, and FineStage.rerank on both its kernel path and
its > MAX_SEGMENT device-sort fallbacks.

Bars: bit-exact wherever the kernel's arithmetic can be restated exactly (sorts, aggregation, fmaf chains);
otherwise a bound derived, in the test's docstring, from the f32 operations the kernel performs, against float64.
Constants of every derived bound: U = 2^-24 (unit roundoff of one f32 operation); EF = 2^-22 for the device
libm's expf / logf (documented at 1 ulp; 2 ulp = 2^-22 relative is used); TINY = 2^-126 per result that may
underflow (covers flush-to-zero as well as gradual underflow)."""
import ctypes

import numpy as np
import pytest
import torch

from mevi_amd import fine, hip, ops
from oracle import dense as odense

from rankcheck import same_ranking

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EF = 2.0 ** -22
TINY = 2.0 ** -126

# segment lengths: empty, one, around one wave / the 64-key minimum, mid, and the LDS opt-in (P = 16384, 128 KiB)
SEG_LENS = [0, 1, 63, 64, 65, 1000, 8192, 8193, 16384]


def _oracle_dot():
    L = odense.lib()
    L.oracle_dot_f32.restype = ctypes.c_float
    L.oracle_dot_f32.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    return lambda a, b: L.oracle_dot_f32(a.ctypes.data, b.ctypes.data, a.shape[0])


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ----------------------------------------------------------------------------------------------------------------------
# 1. segmented aggregate sort


def _ref_aggregate(sc, ids, mode):
    """main_models.py:4001-4011 restated: uscores from f32 0 (add) or -inf (max), every entry folded in candidate
    order with ONE scalar f32 operation, then sorted by (score desc, id asc)."""
    udocs, uidx = np.unique(ids, return_inverse=True)
    acc = [np.float32(0.0) if mode == "add" else np.float32(-np.inf)] * len(udocs)
    for ui, s in zip(uidx.tolist(), sc.tolist()):
        s = np.float32(s)
        acc[ui] = acc[ui] + s if mode == "add" else max(acc[ui], s)
    acc = np.array(acc, np.float32).reshape(-1)
    order = np.lexsort((udocs, -acc))
    return acc[order], udocs[order]


def _aggregate_segment(rng, n):
    """n candidate entries: ids repeated 1..50 times with a DIFFERENT score per occurrence (sign random, magnitude
    log-uniform in 1e-30..1e30), single-occurrence ids mixed in, and groups of ids whose occurrences carry the same
    small dyadic values (every sum and max exact) -- exactly tied aggregates that only the id order separates."""
    ids, sc = [], []
    id_pool = rng.choice(2 ** 31 - 1, size=n + 8, replace=False)
    k = 0
    while len(ids) < n:
        left = n - len(ids)
        kind = rng.random()
        if kind < 0.15:                                            # a tie group: 2..4 ids, same value multiset
            m = int(min(rng.integers(1, 8), max(left // 2, 1)))
            vals = (rng.integers(1, 400, size=m) / 4.0).astype(np.float32)
            g = int(min(rng.integers(2, 5), max(left // m, 1)))
            for _ in range(g):
                ids += [int(id_pool[k])] * m
                sc += list(rng.permutation(vals))
                k += 1
            continue
        m = 1 if kind < 0.5 else int(rng.integers(1, 51))
        m = min(m, left)
        ids += [int(id_pool[k])] * m
        sc += list((rng.choice([-1.0, 1.0], size=m) * 10.0 ** rng.uniform(-30, 30, size=m)).astype(np.float32))
        k += 1
    ids, sc = np.array(ids[:n], np.int64), np.array(sc[:n], np.float32)
    p = rng.permutation(n)                                         # occurrences interleaved in candidate order
    return sc[p], ids[p]


def _check_aggregate(cuda, segs, mode):
    lens = [len(s[0]) for s in segs]
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    sc = np.concatenate([s[0] for s in segs]).astype(np.float32)
    ids = np.concatenate([s[1] for s in segs]).astype(np.int64)
    os_, oi_, cnt = ops.segment_aggregate_sort(_dev(sc, cuda), _dev(ids, cuda), _dev(seg, cuda), max(lens), mode)
    os_, oi_, cnt = os_.cpu().numpy(), oi_.cpu().numpy(), cnt.cpu().numpy()
    for j, (a, b) in enumerate(zip(seg[:-1], seg[1:])):
        rs, ri = _ref_aggregate(sc[a:b], ids[a:b], mode)
        assert cnt[j] == len(ri), (j, cnt[j], len(ri))
        assert np.array_equal(oi_[a:a + cnt[j]], ri), f"segment {j} (len {b - a}): ids differ"
        assert np.array_equal(os_[a:a + cnt[j]].view(np.uint32), rs.view(np.uint32)), f"segment {j}: score bits differ"


@pytest.mark.parametrize("mode", ["add", "max"])
@pytest.mark.parametrize("n", SEG_LENS)
def test_segment_aggregate_sort_equals_the_reference_loop(cuda, n, mode):
    """Bit-exact (scores, ids, counts) against the reference's scalar loop: the kernel folds each id's entries in
    candidate order from 0 / -inf with one f32 add / fmaxf each, exactly the loop's arithmetic."""
    rng = np.random.default_rng(1000 + n)
    _check_aggregate(cuda, [_aggregate_segment(rng, n)], mode)


@pytest.mark.parametrize("mode", ["add", "max"])
def test_segment_aggregate_sort_mixed_segments_in_one_launch(cuda, mode):
    """Bit-exact, several segments of mixed lengths (empty ones and the 16384-entry opt-in size among them) sharing
    one launch: every workgroup sizes its own sort inside the launch's LDS."""
    rng = np.random.default_rng(7)
    lens = [65, 0, 16384, 1, 8193, 63, 0, 1000, 64, 8192]
    _check_aggregate(cuda, [_aggregate_segment(rng, n) for n in lens], mode)


# ----------------------------------------------------------------------------------------------------------------------
# 2. segmented sort


def _check_sort(cuda, segs):
    lens = [len(s[0]) for s in segs]
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    sc = np.concatenate([s[0] for s in segs]).astype(np.float32)
    ids = np.concatenate([s[1] for s in segs]).astype(np.int64)
    os_, oi_ = ops.segment_sort_desc(_dev(sc, cuda), _dev(ids, cuda), _dev(seg, cuda), max(lens))
    os_, oi_ = os_.cpu().numpy(), oi_.cpu().numpy()
    for j, (a, b) in enumerate(zip(seg[:-1], seg[1:])):
        order = np.lexsort((ids[a:b], -sc[a:b]))
        assert np.array_equal(oi_[a:b], ids[a:b][order]), f"segment {j} (len {b - a}): ids differ"
        assert np.array_equal(os_[a:b].view(np.uint32), sc[a:b][order].view(np.uint32)), f"segment {j}: score bits differ"


def _sort_segment(rng, n):
    """Scores with many exact ties (a few dozen quarter-integers), some distinct values, +-inf and extreme
    magnitudes; ids drawn from a small range (repeats) and the full 31-bit range."""
    sc = (rng.integers(-40, 40, size=n) / 4.0).astype(np.float32)
    wide = rng.random(n) < 0.3
    sc[wide] = (rng.choice([-1.0, 1.0], size=int(wide.sum())) * 10.0 ** rng.uniform(-30, 30, size=int(wide.sum()))).astype(np.float32)
    sc[rng.random(n) < 0.01] = np.inf
    sc[rng.random(n) < 0.01] = -np.inf
    ids = np.where(rng.random(n) < 0.5, rng.integers(0, 64, size=n), rng.integers(0, 2 ** 31 - 1, size=n)).astype(np.int64)
    return sc, ids


@pytest.mark.parametrize("n", SEG_LENS)
def test_segment_sort_desc_at_its_limits(cuda, n):
    """Bit-exact against np.lexsort((ids, -scores)), the order nci.generate relies on: integer keys, no arithmetic."""
    _check_sort(cuda, [_sort_segment(np.random.default_rng(2000 + n), n)])


def test_segment_sort_desc_mixed_segments_in_one_launch(cuda):
    """Bit-exact, segments of mixed lengths incl. empty ones and the opt-in sizes in one launch."""
    rng = np.random.default_rng(8)
    _check_sort(cuda, [_sort_segment(rng, n) for n in [8193, 0, 1, 16384, 63, 0, 65, 1000, 64, 8192]])


def test_segment_aggregate_sort_of_an_all_empty_batch(cuda):
    """Every segment empty and no entries at all: counts 0, nothing else touched."""
    e = torch.zeros(0, dtype=torch.float32, device=cuda)
    _, _, cnt = ops.segment_aggregate_sort(e, e.long(), _dev(np.zeros(4, np.int64), cuda), 0, "add")
    assert cnt.cpu().tolist() == [0, 0, 0]


# ----------------------------------------------------------------------------------------------------------------------
# 3. row softmax


def _lse_model(x):
    """float64 model of the kernel's log-sum-exp of every row of x f32 [rows, cols] (max; per lane a sequential sum
    of expf(x - max) over columns lane, lane + 64, ...; a 6-level shuffle tree; logf).  Returns (t = x - max exact,
    e = exp(t), s = sum e, rho [rows, cols] = relative error bound of each computed expf, lam [rows] = bound on
    |logf(s_computed) - log(s)|).

    max: fmaxf is exact.  t_c: one f32 subtraction, t_c (1 + d), |d| <= U, so exp(t_c) is off by a factor e^(t_c d)
    and expf adds EF: rho_c = expm1(|t_c| U) (1 + EF) + EF (+ TINY absolute when the result underflows).  Sum: a term passes at most d = ceil(cols/64) - 1 lane additions (the first,
    0 + e, is exact) and 6 tree levels, so s_k = sum e_c (1 + rho_c)(1 + g_c), |g_c| <= gamma_d = dU / (1 - dU);
    all terms are positive, hence eta = |s_k / s - 1| <= (sum e_c rho_c) / s + gamma_d (1 + max rho) + cols TINY / s.
    logf(s_k) = (log s + log(1 + eta')) (1 + EF'):  lam = eta / (1 - eta) + (log s + eta / (1 - eta)) EF."""
    x = x.astype(np.float64)
    cols = x.shape[1]
    m = x.max(1, keepdims=True)
    t = x - m
    e = np.exp(t)
    s = e.sum(1)
    rho = np.expm1(np.abs(t) * U) * (1 + EF) + EF
    d = -(-cols // 64) - 1 + 6
    gam = d * U / (1 - d * U)
    eta = (e * rho).sum(1) / s + gam * (1 + rho.max(1)) + cols * TINY / s
    lam = eta / (1 - eta) + (np.log(s) + eta / (1 - eta)) * EF
    return t, e, s, rho, lam


def _log_bound(t, lam, ref):
    """|kernel - float64| of (t_k - logf(s_k)) (+ beam score): t rounded (|t| U), the logf error lam, and one
    rounding of the result (|ref| + |t| U + lam) U."""
    return np.abs(t) * U + lam[:, None] + (np.abs(ref) + np.abs(t) * U + lam[:, None]) * U


def _prob_bound(rho, lam, ref, w, s):
    """|kernel - float64| of w * (expf(t) / expf(logf(s_k))): numerator (1 + rho), denominator expf(l) with
    |l - log s| <= lam, so within a factor (1 +- mu), mu = (e^lam - 1) + EF e^lam; one division and one multiply
    (U each): rel = (1 + rho)(1 + U)^2 / (1 - mu) - 1.  Underflow: the numerator, the quotient and the product may
    each lose TINY (the first two then scaled by |w| / den and |w|), den >= s (1 - mu)."""
    mu = np.expm1(lam) + EF * np.exp(lam)
    rel = (1 + rho) * (1 + U) ** 2 / (1 - mu[:, None]) - 1
    aw = np.abs(np.asarray(w, np.float64)).reshape(-1, 1)
    return rel * np.abs(ref) + TINY * (aw / (s[:, None] * (1 - mu[:, None])) * (1 + rel) + aw + 1), rel


def _softmax_inputs(rng, rows, cols):
    x = rng.uniform(-80, 80, size=(rows, cols)).astype(np.float32)    # expf(x - max) underflows for most columns
    x[1] = 3.25                                                       # all columns equal
    x[2] = -80.0
    x[3] = rng.standard_normal(cols).astype(np.float32)               # a peaked-free, well-conditioned row
    return x


@pytest.mark.parametrize("cols", [1, 5, 63, 64, 65, 257, 5000])
def test_row_softmax_log_mode_vs_float64(cuda, cols):
    """mode 0 (out = (x - max) - logf(sum expf(x - max))) within _log_bound of float64 (see _lse_model for the
    derivation).  At cols <= 257 with |x| <= 80 the bound is below 5e-5 (|t| <= 160: 160 U + 160 U for the two
    roundings, sum e_c |t_c| U / s <= cols U / e, gamma_10, log(257) EF: about 2.7e-5), so a kernel that dropped
    one column holding 1e-4 of the normaliser -- every output of its row off by -log(1 - 1e-4) ~ 1e-4 -- fails."""
    rng = np.random.default_rng(cols)
    rows = 7 if cols > 1000 else 13
    x = _softmax_inputs(rng, rows, cols)
    got = ops.row_softmax(_dev(x, cuda), log=True).cpu().numpy().astype(np.float64)
    t, e, s, rho, lam = _lse_model(x)
    ref = t - np.log(s)[:, None]
    bound = _log_bound(t, lam, ref)
    if cols <= 257:
        assert bound.max() < 5e-5, bound.max()
    assert np.all(np.abs(got - ref) <= bound), float((np.abs(got - ref) / bound).max())


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("cols", [1, 5, 63, 64, 65, 257, 5000])
def test_row_softmax_prob_mode_vs_float64(cuda, cols, with_scale):
    """mode 1 (out = w * (expf(x - max) / expf(logf(sum)))) within _prob_bound of float64, w = scale[row] or 1.
    At cols <= 257 the relative part is below 5e-5 (rho <= 160 U + EF, mu ~ lam + EF ~ 7e-6), so dropping a column
    holding 1e-4 of the normaliser -- every output of its row 1e-4 too large -- fails."""
    rng = np.random.default_rng(50 + cols)
    rows = 7 if cols > 1000 else 13
    x = _softmax_inputs(rng, rows, cols)
    w = (rng.random(rows) * 4 - 1).astype(np.float32) if with_scale else np.ones(rows, np.float32)
    got = ops.row_softmax(_dev(x, cuda), log=False, scale=_dev(w, cuda) if with_scale else None).cpu().numpy()
    t, e, s, rho, lam = _lse_model(x)
    ref = w.astype(np.float64)[:, None] * e / s[:, None]
    bound, rel = _prob_bound(rho, lam, ref, w, s)
    if cols <= 257:
        assert rel.max() < 5e-5, rel.max()
    assert np.all(np.abs(got.astype(np.float64) - ref) <= bound), float((np.abs(got - ref) / bound).max())


# ----------------------------------------------------------------------------------------------------------------------
# 4. beam step


def _beam_step_raw(logits, bs, K, R, mode):
    """mevi_beam_step_f32 in any mode (mode 2 is what pq.beam_search calls)."""
    nq, nb = bs.shape
    dev = logits.device
    sc = torch.empty((nq, R), dtype=torch.float32, device=dev)
    parent = torch.empty((nq, R), dtype=torch.int32, device=dev)
    code = torch.empty((nq, R), dtype=torch.int32, device=dev)
    hip.check(hip.lib().mevi_beam_step_f32(hip.ptr(logits), hip.ptr(bs), nq, nb, K, R, mode, hip.ptr(sc), hip.ptr(parent),
                                           hip.ptr(code), hip.stream_ptr()), "mevi_beam_step_f32")
    return sc.cpu().numpy(), parent.cpu().numpy().astype(np.int64), code.cpu().numpy().astype(np.int64)


def _beam_ref(x, bs, K, mode):
    """float64 candidate scores [nq, nb*K] and their bounds (see _log_bound / _prob_bound): mode 0 bs + lsm[1 + c]
    over the K + 1 columns, mode 2 bs * softmax over the K columns."""
    nq, nb = bs.shape
    t, e, s, rho, lam = _lse_model(x)
    b64 = bs.astype(np.float64).reshape(-1, 1)
    if mode == 0:
        lsm = t[:, 1:] - np.log(s)[:, None]
        ref = b64 + lsm
        e1 = _log_bound(t[:, 1:], lam, lsm)             # (t - logf) as in _log_bound, then one rounding of bs + that
        err = e1 + (np.abs(ref) + e1) * U
    else:
        ref = b64 * e / s[:, None]
        err, _ = _prob_bound(rho, lam, ref, bs.reshape(-1), s)
    return ref.reshape(nq, nb * K), err.reshape(nq, nb * K)


def _beam_inputs(rng, nq, nb, K, mode):
    ncol = K + 1 if mode == 0 else K
    x = (rng.standard_normal((nq * nb, ncol)) * 3).astype(np.float32)
    if mode == 0:
        bs = (-rng.random((nq, nb)) * 5).astype(np.float32)
        x[0, :] = rng.uniform(-80, 80, ncol).astype(np.float32)         # large-magnitude logits
    else:
        bs = rng.random((nq, nb)).astype(np.float32)
        x[0, :] = rng.uniform(-80, 80, ncol).astype(np.float32)         # probabilities underflow to 0
        if nb > 1:
            x[1, :] = -1e4 * rng.random(ncol).astype(np.float32)        # all but the max underflow
    return x, bs


def _check_selection(sc, parent, code, ref, err, K, R):
    """Returned scores within tol = max(err + |ref| U) of float64 (the extra |ref| U: same_ranking compares against
    ref rounded to f32); the chosen (parent, code) set equals the float64 top-R except inside runs closer than
    2 tol; (parent, code) names a candidate whose float64 score is within tol of the returned score."""
    nq = ref.shape[0]
    for q in range(nq):
        flat = parent[q] * K + code[q]
        assert np.all((code[q] >= 0) & (code[q] < K)) and len(np.unique(flat)) == R
        tol = float((err[q] + np.abs(ref[q]) * U).max())
        order = np.lexsort((np.arange(ref.shape[1]), -ref[q]))[:R]
        same_ranking(sc[q], flat, ref[q][order], order, tol=tol, full_scores=ref[q])
        assert np.all(np.abs(sc[q].astype(np.float64) - ref[q][flat]) <= tol)


BEAM_SHAPES = [(K, nb, R) for K, nb in [(1, 7), (5, 9), (32, 10), (33, 6), (256, 3)] for R in (1, nb * K)] + [
    (256, 64, 64), (256, 64, 16384), (32, 512, 100), (32, 512, 16384)]   # nb*K = 16384: P = 16384, 128 KiB of keys


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("K,nb,R", BEAM_SHAPES)
def test_beam_step_selects_the_float64_top_r(cuda, K, nb, R, mode):
    """Selection against float64 (_check_selection) with the bound of _beam_ref; and the returned bits equal the
    kernel's own all-candidates run (R = nb*K) at the same (parent, code): the score of a candidate does not depend
    on which of them are kept.  Mode 0: NCI step; mode 2: pq.beam_search step, incl. rows whose probabilities
    underflow to 0 (exact ties there, broken by r*K + c)."""
    rng = np.random.default_rng(K * 1000 + nb + mode)
    nq = 2 if nb * K >= 8192 else 3
    x, bs = _beam_inputs(rng, nq, nb, K, mode)
    xd, bd = _dev(x, cuda), _dev(bs, cuda)
    sc, parent, code = _beam_step_raw(xd, bd, K, R, mode)
    ref, err = _beam_ref(x, bs, K, mode)
    _check_selection(sc, parent, code, ref, err, K, R)
    full, fp, fc = _beam_step_raw(xd, bd, K, nb * K, mode) if R < nb * K else (sc, parent, code)
    for q in range(nq):
        by_flat = np.empty(nb * K, np.float32)
        by_flat[fp[q] * K + fc[q]] = full[q]
        assert np.array_equal(sc[q].view(np.uint32), by_flat[parent[q] * K + code[q]].view(np.uint32))
        if R == nb * K:
            assert np.array_equal(np.sort(fp[q] * K + fc[q]), np.arange(nb * K))


@pytest.mark.parametrize("K,nb", [(1, 7), (5, 9), (33, 6), (256, 3)])
def test_beam_step_final_mode_vs_float64(cuda, K, nb):
    """mode 1 (bs + log_softmax[eos]) within the mode-0 bound of the eos column."""
    rng = np.random.default_rng(300 + K)
    x, bs = _beam_inputs(rng, 3, nb, K, 0)
    got = ops.beam_step(_dev(x, cuda), _dev(bs, cuda), K, 1, final_step=True).cpu().numpy().astype(np.float64)
    t, e, s, rho, lam = _lse_model(x)
    lsm = t[:, :1] - np.log(s)[:, None]
    ref = bs.astype(np.float64).reshape(-1, 1) + lsm
    e1 = _log_bound(t[:, :1], lam, lsm)
    err = e1 + (np.abs(ref) + e1) * U
    assert np.all(np.abs(got.reshape(-1, 1) - ref) <= err)


@pytest.mark.parametrize("mode", [0, 2])
def test_beam_step_exact_ties_come_out_by_flat_index(cuda, mode):
    """Identical rows and beam scores give bit-identical candidates (same arithmetic on the same inputs); the order
    must then be score descending, equal scores by ascending r*K + c -- exactly.  Logits are multiples of 0.5 with
    repeats inside the row, so different logits are far apart and equal logits tie within the row as well."""
    rng = np.random.default_rng(9)
    nq, nb, K = 2, 8, 33
    ncol = K + 1 if mode == 0 else K
    row = (rng.integers(-6, 6, size=ncol) / 2.0).astype(np.float32)
    x = np.tile(row, (nq * nb, 1))
    bs = np.full((nq, nb), -1.5 if mode == 0 else 0.75, np.float32)
    sc, parent, code = _beam_step_raw(_dev(x, cuda), _dev(bs, cuda), K, nb * K, mode)
    cl = row[1:] if mode == 0 else row
    expect = np.lexsort((np.arange(nb * K), -np.tile(cl, nb).astype(np.float64)))
    for q in range(nq):
        assert np.array_equal(parent[q] * K + code[q], expect)
        for v in np.unique(cl):                                       # one bit pattern per logit value
            assert len(np.unique(sc[q][np.tile(cl, nb)[expect] == v].view(np.uint32))) == 1


@pytest.mark.parametrize("nb,K", [(9, 7), (64, 256)])
def test_pq_step_agrees_with_row_softmax_keep_all_branch(cuda, nb, K):
    """pq.beam_search sends R < nb*K through beam-step mode 2 and keeps everything through row_softmax mode 1 with
    scale = beam probability.  Both compute beam_prob * (expf(x - max) / expf(logf(sum))) with the same reduction
    order, so at R = nb*K - 1 mode 2 returns the R best entries of the row_softmax output -- same bits, same order
    (score desc, flat index asc)."""
    rng = np.random.default_rng(nb + K)
    nq = 3
    x, bs = _beam_inputs(rng, nq, nb, K, 2)
    xd, bd = _dev(x, cuda), _dev(bs, cuda)
    R = nb * K - 1
    sc, parent, code = _beam_step_raw(xd, bd, K, R, 2)
    allp = ops.row_softmax(xd, log=False, scale=bd.reshape(-1)).cpu().numpy().reshape(nq, nb * K)
    for q in range(nq):
        order = np.lexsort((np.arange(nb * K), -allp[q].astype(np.float64)))[:R]
        assert np.array_equal(parent[q] * K + code[q], order)
        assert np.array_equal(sc[q].view(np.uint32), allp[q][order].view(np.uint32))


def _random_trie(rng, n_nodes, K):
    """Children sets of one trie level with K = 256 codes (masks of 8 words): nodes with a single child at word
    edges (codes 0, 31, 32, 255, 128), sparse and dense nodes; children numbered contiguously in code order."""
    bits = rng.random((n_nodes, K)) < rng.uniform(0.02, 0.6, size=(n_nodes, 1))
    for i, c in enumerate([0, 31, 32, 255, 128]):
        bits[i] = False
        bits[i, c] = True
    bits[np.flatnonzero(~bits.any(1)), 7] = True
    W = (K + 31) // 32
    words = np.zeros((n_nodes, W), np.uint64)
    for c in range(K):
        words[:, c // 32] |= bits[:, c].astype(np.uint64) << np.uint64(c % 32)
    tbase = (1000 + np.concatenate([[0], np.cumsum(bits.sum(1))[:-1]])).astype(np.int32)
    return bits, words.astype(np.uint32), tbase


@pytest.mark.parametrize("nb,R", [(12, 12), (12, 1), (64, 64)])
def test_beam_step_tree_masks_and_child_index(cuda, nb, R):
    """Tree form, K = 256: masked codes hold the row's LARGEST logits and must never be chosen; the allowed
    candidates are selected as by float64 (normaliser over eos and all K codes, bound as mode 0); out_node equals
    tbase[node] + popcount(mask below c) computed in numpy, exactly.  nb = 64: nb*K = 16384, the opt-in size."""
    rng = np.random.default_rng(nb + R)
    nq, K, n_nodes = 3, 256, 40
    bits, words, tbase = _random_trie(rng, n_nodes, K)
    node = rng.integers(0, n_nodes, size=(nq, nb)).astype(np.int32)
    node[0, :5] = np.arange(5)                                         # the single-child nodes
    x = (rng.standard_normal((nq * nb, K + 1)) * 3).astype(np.float32)
    allowed = bits[node.reshape(-1)]                                   # [nq*nb, K]
    top = x.max(1, keepdims=True)
    x[:, 1:] = np.where(allowed, x[:, 1:], top + 5 + rng.random((nq * nb, K)).astype(np.float32))
    bs = (-rng.random((nq, nb)) * 5).astype(np.float32)
    sc, parent, code, child = (a.cpu().numpy() for a in ops.beam_step_tree(
        _dev(x, cuda), _dev(bs, cuda), K, R, _dev(node, cuda), _dev(words.view(np.int32), cuda), _dev(tbase, cuda)))
    parent, code = parent.astype(np.int64), code.astype(np.int64)
    ref, err = _beam_ref(x, bs, K, 0)
    below = np.cumsum(bits, 1) - bits                                  # children with a lower code
    for q in range(nq):
        nd = node[q, parent[q]]
        assert np.all(bits[nd, code[q]]), "a masked code was chosen"
        assert np.array_equal(child[q], tbase[nd] + below[nd, code[q]])
        ok = allowed.reshape(nq, nb * K)[q]
        rq_ = np.where(ok, ref[q], -np.inf)
        flat = parent[q] * K + code[q]
        tol = float((err[q][ok] + np.abs(ref[q][ok]) * U).max())
        order = np.lexsort((np.arange(nb * K), -rq_))[:R]
        same_ranking(sc[q], flat, rq_[order], order, tol=tol, full_scores=rq_)
        assert np.all(np.abs(sc[q].astype(np.float64) - ref[q][flat]) <= tol)


def test_beam_step_refusals_on_the_host(cuda):
    """Shapes the kernels cannot hold are refused by the C ABI before any launch: nb*K = 16385 (plain and tree),
    R > nb*K (plain), nb < R (tree), and nb*K = 16384 with K = 1, whose nb-float tables would push the workgroup's
    LDS past 160 KiB."""
    def plain(nb, K, R, mode=0):
        x = torch.zeros((nb, K + (mode != 2)), dtype=torch.float32, device=cuda)
        return _beam_step_raw(x, torch.zeros((1, nb), dtype=torch.float32, device=cuda), K, R, mode)

    def tree(nb, K, R):
        W = (K + 31) // 32
        return ops.beam_step_tree(torch.zeros((nb, K + 1), dtype=torch.float32, device=cuda),
                                  torch.zeros((1, nb), dtype=torch.float32, device=cuda), K, R,
                                  torch.zeros((1, nb), dtype=torch.int32, device=cuda),
                                  torch.full((1, W), -1, dtype=torch.int32, device=cuda),
                                  torch.zeros(1, dtype=torch.int32, device=cuda))

    for call in (lambda: plain(5, 3277, 1), lambda: plain(5, 3277, 1, mode=2), lambda: plain(2, 3, 7),
                 lambda: plain(2, 3, 7, mode=2), lambda: plain(16384, 1, 1), lambda: plain(8192, 2, 1, mode=2),
                 lambda: tree(5, 3277, 1), lambda: tree(2, 4, 3), lambda: tree(16384, 1, 1)):
        with pytest.raises(hip.MeviHipError):
            call()
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# 5. pair_dot


@pytest.mark.parametrize("n", [1, 63, 257])
@pytest.mark.parametrize("dim", [4, 36, 100, 772])
def test_pair_dot_edges(cuda, dim, n):
    """Bit-exact against oracle_dot_f32 (the same sequential fmaf chain) at dims that are not a multiple of the 32-wide
    slab, with both operands column slices of wider matrices (lda, ldb > dim, 16-byte offset), and indices that point
    at the last row."""
    rng = np.random.default_rng(dim * 7 + n)
    na, nb_ = 11, 300
    wa = rng.standard_normal((na, dim + 12)).astype(np.float32)
    wb = rng.standard_normal((nb_, dim + 8)).astype(np.float32)
    ia = rng.integers(0, na, size=n)
    ib = rng.integers(0, nb_, size=n)
    ia[-1], ib[-1], ib[0] = na - 1, nb_ - 1, nb_ - 1
    A, B = _dev(wa, cuda)[:, 4:4 + dim], _dev(wb, cuda)[:, 8:8 + dim]
    assert A.stride(0) == dim + 12 and B.stride(0) == dim + 8
    got = ops.pair_dot(A, _dev(ia, cuda), B, _dev(ib, cuda)).cpu().numpy()
    dot = _oracle_dot()
    a, b = np.ascontiguousarray(wa[:, 4:4 + dim]), np.ascontiguousarray(wb[:, 8:8 + dim])
    ref = np.array([dot(a[i], b[j]) for i, j in zip(ia, ib)], np.float32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


# ----------------------------------------------------------------------------------------------------------------------
# 6. FineStage.rerank: kernel path and > MAX_SEGMENT fallbacks


def _restate_rerank(dot, q, emb, cluster, beams, aggregate, w=None, doc_proba=None, recon=None, ratio=0.0):
    """The reference's fine stage, literally: per beam cluster (dict lookup, beam order, repeats scored again) the
    fmaf-chain q.d; get_inference_scores in f32 -- w * (ratio * p + (1 - ratio) * qd), each an f32 operation, the
    Python scalars rounded to f32 as torch does; p = doc_proba[d] or <recon[b*R + r], d>; the aggregate loop of
    main_models.py:4001-4011 (_ref_aggregate); sort by (score desc, id asc)."""
    B, R, _ = beams.shape
    out = []
    for b in range(B):
        docs, scs = [], []
        for r in range(R):
            cur = cluster.get(tuple(int(v) for v in beams[b, r]))
            if cur is None:
                continue
            s = np.array([dot(q[b], emb[d]) for d in cur], np.float32)
            if w is not None:
                if recon is not None and ratio:
                    p = np.array([dot(recon[b * R + r], emb[d]) for d in cur], np.float32)
                elif doc_proba is not None and ratio:
                    p = doc_proba[cur]
                else:
                    p = None
                if p is not None:
                    s = np.float32(ratio) * p + np.float32(1 - ratio) * s
                s = np.float32(w[b, r]) * s
            docs += list(cur)
            scs.append(s)
        docs = np.array(docs, np.int64)
        scs = np.concatenate(scs).astype(np.float32) if scs else np.zeros(0, np.float32)
        if aggregate is not None:
            scs, docs = _ref_aggregate(scs, docs, aggregate)
        else:
            o = np.lexsort((docs, -scs))
            scs, docs = scs[o], docs[o]
        out.append((docs, scs))
    return out


def _cluster_dict(labels):
    cluster = {}
    for d in range(labels.shape[0]):
        for c in range(labels.shape[1]):
            cluster.setdefault(tuple(int(v) for v in labels[d, c]), []).append(d)
    return cluster


def _check_rerank(cuda, fs, q, beams, ref, monkeypatch, max_segment, aggregate, **kw):
    if max_segment is not None:
        monkeypatch.setattr(fine, "MAX_SEGMENT", max_segment)
    out, ndoc = fs.rerank(_dev(q, cuda), beams, aggregate=aggregate, **kw)
    for b, (docs, scs) in enumerate(ref):
        assert np.array_equal(out[b][0], docs), f"query {b}: ids differ"
        assert np.array_equal(out[b][1].view(np.uint32), scs.view(np.uint32)), f"query {b}: score bits differ"


@pytest.fixture(scope="module")
def multiclus(cuda):
    """1500 documents in 3 distinct clusters each (M = 2, codes < 6; code 6 never used, so clusters with it are
    empty); 7 queries with 5 beams, clusters repeated in some beam lists, one query with only empty clusters."""
    from mevi_amd.fine import FineStage
    from mevi_amd.rq import ClusterIndex

    rng = np.random.default_rng(21)
    N, dim, K, C, B, R = 1500, 64, 7, 3, 7, 5
    paths = np.argsort(rng.random((N, 36)), 1)[:, :C]
    labels = np.stack([paths // 6, paths % 6], -1).astype(np.int32)    # [N, C, 2], distinct paths per document
    emb = rng.standard_normal((N, dim)).astype(np.float32)
    q = rng.standard_normal((B, dim)).astype(np.float32)
    beams = rng.integers(0, 6, size=(B, R, 2))
    beams[1, 3] = beams[1, 0]
    beams[2, 1:3] = beams[2, 4]
    beams[3] = 6
    beams[4, 2] = 6
    w = rng.random((B, R)).astype(np.float32)
    doc_proba = rng.random(N).astype(np.float32)
    recon = rng.standard_normal((B * R, dim)).astype(np.float32)
    fs = FineStage(_dev(emb, cuda), ClusterIndex.from_topk_labels(labels, K))
    return dict(fs=fs, q=q, emb=emb, beams=beams, w=w, doc_proba=doc_proba, recon=recon, cluster=_cluster_dict(labels))


@pytest.mark.parametrize("max_segment", [None, 40])
@pytest.mark.parametrize("weights", [None, "w", "w+doc_proba", "w+recon"])
@pytest.mark.parametrize("aggregate", [None, "add", "max"])
def test_rerank_equals_reference_procedure_on_both_paths(cuda, multiclus, monkeypatch, aggregate, weights, max_segment):
    """Bit-exact (ids and scores) against _restate_rerank, multi-cluster documents reached through several beams,
    with the default MAX_SEGMENT (LDS kernels) and with MAX_SEGMENT = 40, which sends the same inputs through the
    device-sort fallbacks of a > 16384-candidate query."""
    m = multiclus
    ratio = 0.3 if weights in ("w+doc_proba", "w+recon") else 0.0
    kw, rkw = {}, {}
    if weights is not None:
        kw = dict(beam_weights=_dev(m["w"], cuda), ratio=ratio)
        rkw = dict(w=m["w"], ratio=ratio)
        if weights == "w+doc_proba":
            kw["doc_proba"], rkw["doc_proba"] = _dev(m["doc_proba"], cuda), m["doc_proba"]
        if weights == "w+recon":
            kw["beam_recon"], rkw["recon"] = _dev(m["recon"], cuda), m["recon"]
    ref = _restate_rerank(_oracle_dot(), m["q"], m["emb"], m["cluster"], m["beams"], aggregate, **rkw)
    assert max(len(r[0]) for r in ref) > 40
    _check_rerank(cuda, m["fs"], m["q"], m["beams"], ref, monkeypatch, max_segment, aggregate, **kw)


@pytest.mark.parametrize("aggregate", ["add", "max"])
def test_rerank_of_a_query_beyond_the_lds_sort(cuda, monkeypatch, aggregate):
    """True size, no monkeypatch: one cluster of 20 000 documents (dim 64) gives query 0 more than 16384 candidates
    (and more than 16384 unique documents), next to queries that stay small; every document sits in two clusters, so
    query 0 reaches many of them through several beams, and repeats a cluster.  With beam weights each occurrence has
    its own score.  Bit-exact against _restate_rerank."""
    from mevi_amd.fine import FineStage
    from mevi_amd.rq import ClusterIndex

    rng = np.random.default_rng(33)
    big, extra, dim, K, R, B = 20000, 2000, 64, 8, 4, 3
    N = big + extra
    labels = np.zeros((N, 2, 2), np.int32)
    labels[:big, 1] = np.stack([rng.integers(1, 3, big), rng.integers(0, K, big)], -1)
    p = np.argsort(rng.random((extra, 7 * K)), 1)[:, :2] + K       # two distinct paths among codes (1..7, 0..7)
    labels[big:] = np.stack([p // K, p % K], -1)
    emb = rng.standard_normal((N, dim)).astype(np.float32)
    q = rng.standard_normal((B, dim)).astype(np.float32)
    beams = np.array([[[0, 0], [1, 3], [2, 5], [1, 3]],
                      [[3, 1], [4, 2], [3, 1], [5, 0]],
                      [[6, 6], [7, 7], [1, 2], [2, 2]]])
    w = rng.random((B, R)).astype(np.float32)
    cluster = _cluster_dict(labels)
    ref = _restate_rerank(_oracle_dot(), q, emb, cluster, beams, aggregate, w=w)
    assert len(ref[0][0]) > fine.MAX_SEGMENT and max(len(r[0]) for r in ref[1:]) < fine.MAX_SEGMENT
    fs = FineStage(_dev(emb, cuda), ClusterIndex.from_topk_labels(labels, K))
    _check_rerank(cuda, fs, q, beams, ref, monkeypatch, None, aggregate, beam_weights=_dev(w, cuda))
