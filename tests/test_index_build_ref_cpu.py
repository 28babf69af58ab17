"""The references of tests/index_build_ref.py held to simpler statements of themselves, without a device: brute-force
cluster means, the exactness condition of the integer-valued runs, the beam restatement against the oracle's, and the two
conditions on the beam inputs (firm share, measured f32-softmax discrepancy) the GPU comparison's constants rest on."""
import numpy as np
import pytest

import index_build_ref as ib
import pq_ref
from oracle import rq as orq

ALL_BEAM = [(s, R, False) for s, Rs in ib.BEAM_CASES.items() for R in Rs] + \
           [(s, R, True) for s, Rs in ib.PQ_BEAM_CASES.items() for R in Rs]


def _chain(pq):
    return ib.pq_beam_search_chain if pq else ib.rq_beam_search_chain


@pytest.mark.parametrize("n,dim,K", [(1, 3, 2), (500, 7, 5), (4000, 33, 64)])
def test_cluster_means64_equals_a_per_cluster_loop(n, dim, K):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    lab = rng.integers(0, max(K - 1, 1), size=n).astype(np.int32)         # the last cluster stays empty (K > 1)
    old = rng.standard_normal((K, dim)).astype(np.float32)
    for o in (old, None):
        m, cnt, sq, m64 = ib.cluster_means64(x, lab, K, o, return_f64=True)
        for k in range(K):
            rows = x[lab == k].astype(np.float64)
            want = rows.sum(0) / len(rows) if len(rows) else (o[k] if o is not None else np.zeros(dim))
            assert np.allclose(m64[k], want, rtol=1e-13, atol=1e-15)
            assert cnt[k] == len(rows)
        assert m.dtype == np.float32 and np.array_equal(m, m64.astype(np.float32))
        assert abs(sq - float((x.astype(np.float64) ** 2).sum())) <= 1e-13 * sq
    assert (ib.cluster_means_bound(x, lab, K, n)[cnt == 0] == 0).all()


def test_block_split_matches_the_documented_one():
    assert ib.cluster_means_blocks(0) == (1, 0) and ib.cluster_means_blocks(64) == (1, 64) and ib.cluster_means_blocks(65) == (2, 33)
    assert ib.cluster_means_blocks(65536) == (1024, 64) and ib.cluster_means_blocks(65537) == (1024, 65)
    assert ib.cluster_means_blocks(2_000_000) == (1024, 1954) and ib.cluster_means_blocks(8_841_823)[1] == 8635
    assert ib.cluster_means_chunk(256) == 64 and ib.cluster_means_chunk(4096) == 4 and ib.cluster_means_chunk(7) == 256


def test_integer_runs_are_exact_in_f32():
    """|x| <= 8, integer-valued: a workgroup's f32 sum stays an integer below 2^24 (exact) iff rows-per-workgroup * 8 < 2^24;
    the squares sum to an integer below 2^53."""
    for n, dim, K in ib.INT_MEANS_CASES:
        assert -(-n // 1024) * 8 < 2 ** 24 and ib.cluster_means_blocks(n)[1] * 8 < 2 ** 24
        assert n * dim * 64 < 2 ** 53
        assert 1 <= K <= 4096 and ib.cluster_means_chunk(K) >= 1
    assert {c[0] for c in ib.INT_MEANS_CASES} >= {0, 1, 63, 64, 65, 4097, 65536, 65537, 2_000_000}
    assert {c[1] for c in ib.INT_MEANS_CASES} >= {1, 3, 4, 100, 256, 260, 768, 1028}
    assert {c[2] for c in ib.INT_MEANS_CASES} >= {1, 7, 100, 256, 1000, 4096}
    assert {(65537, 768, 256), (4097, 260, 4096), (65537, 768, 100)} <= set(ib.INT_MEANS_CASES)


def test_bound_covers_a_sequential_f32_sum():
    """The bound's premise replayed on the CPU: rows added one by one in f32 per workgroup, workgroups in float64."""
    rng = np.random.default_rng(3)
    n, dim, K = 70_001, 5, 3                     # 1024 workgroups of 69 rows
    x = (rng.standard_normal((n, dim)) + 3.0).astype(np.float32)
    lab = (rng.random(n) < 0.9).astype(np.int32) * 2
    nb, P = ib.cluster_means_blocks(n)
    tot = np.zeros((K, dim), np.float64)
    for b in range(nb):
        acc = np.zeros((K, dim), np.float32)
        for r in range(b * P, min(n, (b + 1) * P)):
            acc[lab[r]] += x[r]
        tot += acc
    _, cnt, _, m64 = ib.cluster_means64(x, lab, K, return_f64=True)
    got = np.where(cnt[:, None] > 0, tot / np.maximum(cnt, 1)[:, None], 0.0).astype(np.float32)
    bound = ib.cluster_means_bound(x, lab, K, n)
    assert (np.abs(got - m64) <= bound).all()
    assert np.abs(got - m64).max() > 0                                  # the replay does round


@pytest.mark.parametrize("shape", list(ib.BEAM_CASES), ids=str)
def test_chain_agrees_with_the_oracle_beam_search(shape):
    """oracle.rq.rq_beam_search sums the squared differences with numpy (pairwise), the chain with the sequential fmaf.  At
    level j the two score rows differ by at most e_j, the sum of the two summations' own errors, measured against float64 on
    the greedy path's residuals; a probability moves by at most 2 e_j relative per level, so tol = 2 sum_j e_j, gap = 4 tol.
    The comparison must not be vacuous: at least 85 % of the positions firm up to R = 40.  At R = 260 the low ranks are
    dense and the numpy sum's error at dim 768 (1.9e-5 at level 0, tol 7.6e-5) leaves fewer decidable BETWEEN THE TWO
    DISTANCE ARITHMETICS -- measured 0.69 at (130, 768, 4, 32), >= 0.93 elsewhere -- so half is asked there.  (The device
    comparison is not affected: its score rows equal the chain's bit for bit.)"""
    n, dim, M, K = shape
    x, cb = ib.beam_case_inputs(shape)
    codes, res, tol = orq.rq_encode(x, cb), x.copy(), 0.0
    for j in range(M):
        d64 = ((res[:, None, :].astype(np.float64) - cb[j][None].astype(np.float64)) ** 2).sum(-1)
        e_chain = np.abs(-orq.rq_encode(res, cb[j:j + 1], return_neg_dist=True)[1][:, 0] - d64).max()
        diff = res[:, None, :] - cb[j][None]
        e_numpy = np.abs((diff * diff).sum(-1, dtype=np.float32) - d64).max()
        tol += 2 * float(e_chain + e_numpy)
        res = res - cb[j][codes[:, j]]
    tol = max(tol, ib.SCORE_RTOL)
    for R in ib.BEAM_CASES[shape]:
        lab, sc = ib.rq_beam_search_chain(x, cb, R)
        wl, ws = orq.rq_beam_search(x, cb, R)
        ok, share = ib.beams_agree_rel(lab, sc, wl, ws, tol, 4 * tol)
        print(f"{shape} R={R}: tol {tol:.3g}, firm share {share:.3f}")
        assert ok and share >= (ib.FIRM_SHARE_MIN if R <= 40 else 0.5), (shape, R, tol, share)
        if R == 1:
            assert np.array_equal(lab[:, 0], orq.rq_encode(x, cb))       # greedy = the encoder


@pytest.mark.parametrize("shape", list(ib.PQ_BEAM_CASES), ids=str)
def test_pq_chain_reproduces_pq_ref(shape):
    x, cb = ib.beam_case_inputs(shape, pq=True)
    for R in ib.PQ_BEAM_CASES[shape]:
        wl, ws = pq_ref.beam_search(x, cb, R)
        l32, s32 = ib.pq_beam_search_chain(x, cb, R, softmax_dtype=np.float32)
        # the same f32 steps on differently shaped arrays (numpy's vector exp and K-term sum paths differ by a few ulp)
        assert np.array_equal(l32, wl) and (np.abs(s32.astype(np.float64) - ws) <= ib.MEASURED_F32_SOFTMAX_RDIFF * ws).all()
        lab, sc, cut = ib.pq_beam_search_chain(x, cb, R, return_cut_gap=True)
        ok, share = ib.beams_agree_rel(wl, ws, lab, sc, ib.SCORE_RTOL, ib.GAP_RTOL, cut)
        assert ok and share >= ib.FIRM_SHARE_MIN, (shape, R, share)


def test_beam_cases_cover_the_branches():
    for cases in (ib.BEAM_CASES, ib.PQ_BEAM_CASES):
        for (n, dim, M, K), Rs in cases.items():
            assert n % 128 != 0 and dim % 4 == 0
            for R in Rs:
                assert R <= K ** M and R in {1, 3, 10, K - 1, K, K + 4, 40, 260}
                nb = 1
                for _ in range(M):
                    assert R >= nb * K or nb * K <= 16384                 # what the beam step accepts
                    nb = min(R, nb * K) if R < nb * K else nb * K
    assert 40 in ib.BEAM_CASES[(200, 100, 8, 4)] and 40 >= 4 * 4          # keep-all at two consecutive levels
    assert any(M == 1 for (_, _, M, _) in ib.BEAM_CASES) and any(K == 256 for (_, _, _, K) in ib.BEAM_CASES)


@pytest.mark.parametrize("shape,R,pq", ALL_BEAM, ids=str)
def test_firm_share_condition(shape, R, pq):
    """A CONDITION on the inputs, not a measurement: at GAP_RTOL the reference alone must leave >= 85 % of the positions
    decidable (rows with an undecidable top-R cut counting as not firm), and no score may underflow."""
    x, cb = ib.beam_case_inputs(shape, pq)
    lab, sc, cut = _chain(pq)(x, cb, R, return_cut_gap=True)
    ok, share = ib.beams_agree_rel(lab, sc, lab, sc, ib.SCORE_RTOL, ib.GAP_RTOL, cut)
    assert ok and share >= ib.FIRM_SHARE_MIN, (shape, R, share)
    assert sc.min() > 0 and lab.shape == (shape[0], min(R, shape[3] ** shape[2]), shape[2])


def test_constants_come_from_the_measured_f32_softmax_discrepancy():
    """SCORE_RTOL = 4 x the largest relative difference between the float64-softmax restatement and the same restatement
    with every softmax step in np.float32, over all cases; GAP_RTOL = 4 x SCORE_RTOL."""
    worst = {False: 0.0, True: 0.0}
    for shape, R, pq in ALL_BEAM:
        x, cb = ib.beam_case_inputs(shape, pq)
        _, s64 = _chain(pq)(x, cb, R)
        _, s32 = _chain(pq)(x, cb, R, softmax_dtype=np.float32)
        worst[pq] = max(worst[pq], float((np.abs(s32.astype(np.float64) - s64) / s64).max()))
    print("f32-softmax relative discrepancy: rq %.3g, pq %.3g" % (worst[False], worst[True]))
    measured = max(worst.values())
    # the upper bound is what the constants rest on; the lower one only catches a stale record (numpy builds differ by an ulp or two)
    assert 0.25 * ib.MEASURED_F32_SOFTMAX_RDIFF <= measured <= ib.MEASURED_F32_SOFTMAX_RDIFF
    assert ib.SCORE_RTOL == 4 * ib.MEASURED_F32_SOFTMAX_RDIFF and ib.GAP_RTOL == 4 * ib.SCORE_RTOL


def test_beams_agree_rel_bites():
    shape = (301, 64, 3, 16)
    x, cb = ib.beam_case_inputs(shape)
    lab, sc, cut = ib.rq_beam_search_chain(x, cb, 10, return_cut_gap=True)
    args = (ib.SCORE_RTOL, ib.GAP_RTOL, cut)
    assert ib.beams_agree_rel(lab, sc, lab, sc, *args)[0]
    bad = lab.copy()
    bad[5, 3, 2] ^= 1
    assert not ib.beams_agree_rel(bad, sc, lab, sc, *args)[0]
    assert not ib.beams_agree_rel(lab[:, ::-1], sc[:, ::-1], lab, sc, *args)[0]
    off = sc.copy()
    off[7, 9] *= 1 + 3 * ib.SCORE_RTOL
    assert not ib.beams_agree_rel(lab, off, lab, sc, *args)[0]
    assert not ib.beams_agree_rel(lab[:, :9], sc[:, :9], lab, sc, *args)[0]
    tie = np.tile(np.float32([0.5, 0.25, 0.25, 0.125]), (2, 1))           # an exact tie is not firm, its neighbours are
    tl = np.arange(8, dtype=np.int32).reshape(2, 4, 1)
    sw = tl[:, [0, 2, 1, 3]]
    assert ib.beams_agree_rel(sw, tie, tl, tie, 1e-6, 1e-5) == (True, 0.5)
