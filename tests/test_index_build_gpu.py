"""The offline index build's kernels against exact references at production shapes (tests/index_build_ref.py):
mevi_cluster_means_f32 bit for bit on integer-valued rows and inside its derived bound on real-valued corpora,
mevi_rq_neg_dist_f32 bit for bit against the oracle's fmaf chain over its tile edges, mevi_gather_sub_f32 bit for bit
(fan-out, permutation, in place), ProductQuantization.beam_search beyond the goldens, and the invariants of rq.kmeans."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

import index_build_ref as ib
import synth
from mevi_amd import hip, rq
from oracle import rq as orq

pytestmark = pytest.mark.gpu

OK, ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -3
SENTINEL = -12345.5


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- cluster means, bit for bit ------------------------------------------------------------------------------------------------

def _label_patterns(n, K, rng):
    nb, P = ib.cluster_means_blocks(n)
    yield "uniform", rng.integers(0, K, size=n)
    yield "one cluster", np.full(n, K // 2)
    yield "one label per workgroup", (np.arange(n) // max(P, 1)) % K
    lab = rng.integers(0, max(K - 1, 1), size=n)
    if n:
        lab[((n - 1) // P) * P:] = K - 1                   # cluster K-1 lives in the last, partial, workgroup only
    yield "last workgroup only", lab


@pytest.mark.parametrize("n,dim,K", ib.INT_MEANS_CASES)
def test_cluster_means_bit_for_bit_on_integer_rows(cuda, n, dim, K):
    """Rows of integers in [-8, 8]: every f32 workgroup sum is exact (test_index_build_ref_cpu.py holds the condition), so
    centroids must equal the float64 means rounded once, counts and the sum of squares exactly, and two calls each other."""
    rng = np.random.default_rng(n + 7 * dim + 13 * K)
    x = rng.integers(-8, 9, size=(n, dim)).astype(np.float32)
    old = rng.integers(-8, 9, size=(K, dim)).astype(np.float32)
    xt, ot = _t(x, cuda), _t(old, cuda)
    for name, lab in _label_patterns(n, K, rng):
        lab = lab.astype(np.int32)
        lt = _t(lab, cuda)
        for o, od in ((old, ot), (None, None)) if name == "one cluster" or n == 0 else ((old, ot),):
            c1, n1, sq1 = rq.cluster_means(xt, lt, K, old=od)
            c2, n2, sq2 = rq.cluster_means(xt, lt, K, old=od)
            want, cnt, sq = ib.cluster_means64(x, lab, K, o)
            assert torch.equal(c1, c2) and torch.equal(n1, n2) and sq1 == sq2, name
            got = c1.cpu().numpy()
            bad = np.argwhere(_bits(got) != _bits(want))
            assert len(bad) == 0, (name, o is None, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
            assert np.array_equal(n1.cpu().numpy(), cnt), name
            assert sq1 == float(sq), (name, sq1, float(sq))


def _raw_means(x, codes_ptr, stride, K, n, dim, old, cent, counts, sumsq, ws, ws_ptr, ws_bytes):
    return hip.lib().mevi_cluster_means_f32(hip.ptr(x), n, dim, codes_ptr, stride, K, hip.ptr(old) if old is not None else None,
                                            hip.ptr(cent), hip.ptr(counts), hip.ptr(sumsq) if sumsq is not None else None,
                                            ws_ptr, ws_bytes, hip.stream_ptr())


def test_cluster_means_raw_abi(cuda):
    """code_stride > 1, the nullable arguments, and the refusals -- which must leave every output as it was."""
    rng = np.random.default_rng(2)
    n, dim, K, M = 1000, 36, 9, 3
    x = rng.integers(-8, 9, size=(n, dim)).astype(np.float32)
    codes = rng.integers(0, K - 1, size=(n, M)).astype(np.int32)          # cluster K-1 empty in every column
    xt, ct = _t(x, cuda), _t(codes, cuda)
    L = hip.lib()
    need = L.mevi_cluster_means_workspace_bytes(n, dim, K)
    assert need > 0 and L.mevi_cluster_means_workspace_bytes(n, dim, 0) == 0
    ws = torch.empty(need + 512, dtype=torch.uint8, device=cuda)
    assert ws.data_ptr() % 256 == 0

    def fresh():
        return (torch.full((K, dim), SENTINEL, device=cuda), torch.full((K,), -7, dtype=torch.int32, device=cuda),
                torch.full((1,), -1.0, dtype=torch.float64, device=cuda))

    for j in range(M):                       # column j of the [n, M] code matrix, no old centroids, no sum of squares
        cent, counts, _ = fresh()
        st = _raw_means(xt, ct.data_ptr() + 4 * j, M, K, n, dim, None, cent, counts, None, ws, ws.data_ptr(), need)
        torch.cuda.synchronize()
        assert st == OK
        want, cnt, _ = ib.cluster_means64(x, codes[:, j], K, None)
        assert np.array_equal(_bits(cent.cpu().numpy()), _bits(want)) and np.array_equal(counts.cpu().numpy(), cnt)
        assert (cent[K - 1] == 0).all()
    cent, counts, sumsq = fresh()
    st = _raw_means(xt, ct.data_ptr(), M, K, n, dim, None, cent, counts, sumsq, ws, ws.data_ptr(), need)
    torch.cuda.synchronize()
    assert st == OK and float(sumsq.item()) == float((x.astype(np.float64) ** 2).sum())

    cent, counts, sumsq = fresh()
    refusals = [
        (ws.data_ptr(), need - 1, K, ERR_WORKSPACE),                      # one byte short
        (ws.data_ptr() + 16, need, K, ERR_WORKSPACE),                     # large enough, not 256-byte aligned
        (None, need, K, ERR_WORKSPACE),
        (ws.data_ptr(), need, 4097, ERR_INVALID_ARG),                     # K beyond the LDS table
        (ws.data_ptr(), need, 0, ERR_INVALID_ARG),
    ]
    for ws_ptr, nbytes, k, code in refusals:
        st = _raw_means(xt, ct.data_ptr(), M, k, n, dim, None, cent, counts, sumsq, ws, ws_ptr, nbytes)
        assert st == code, (nbytes, k, st)
        with pytest.raises(hip.MeviHipError):
            hip.check(st, "mevi_cluster_means_f32")
    torch.cuda.synchronize()
    assert (cent == SENTINEL).all() and (counts == -7).all() and float(sumsq.item()) == -1.0


# ---- cluster means, real-valued rows ---------------------------------------------------------------------------------------------

def _means_within_bound(x_t, lab_t, K, record_property, tag):
    n, dim = x_t.shape
    old = torch.zeros((K, dim), device=x_t.device)
    c, cnt_t, sq = rq.cluster_means(x_t, lab_t, K, old=old)
    got = c.cpu().numpy().astype(np.float64)
    x, lab = x_t.cpu().numpy(), lab_t.cpu().numpy()
    _, cnt, sq64, m64 = ib.cluster_means64(x, lab, K, np.zeros((K, dim), np.float32), return_f64=True)
    bound = ib.cluster_means_bound(x, lab, K, n)
    err = np.abs(got - m64)
    nz = m64 != 0
    ulps = float((err[nz] / (ib.U32 * np.abs(m64[nz]))).max())
    sq_units = abs(sq - float(sq64)) / float(sq64) / ib.U64
    P = ib.cluster_means_blocks(n)[1]
    print(f"{tag}: rows per workgroup {P}, clusters {int((cnt > 0).sum())}/{K} (largest {int(cnt.max())}), "
          f"max |mean error| = {ulps:.3f} x 2^-24 |mean|, largest error/bound {float((err[bound > 0] / bound[bound > 0]).max()):.4f}, "
          f"sum_sq off by {sq_units:.1f} x 2^-53 (bound {ib.sum_sq_rtol(n, dim, K) / ib.U64:.0f})")
    record_property(f"{tag}_max_mean_err_in_2^-24_mean", ulps)
    record_property(f"{tag}_sum_sq_err_in_2^-53", sq_units)
    assert np.array_equal(cnt_t.cpu().numpy(), cnt)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), (tag, worst, err[worst], bound[worst])
    assert abs(sq - float(sq64)) <= ib.sum_sq_rtol(n, dim, K) * float(sq64), (tag, sq, float(sq64))


@pytest.mark.parametrize("kind", ["iid", "clustered", "ance_scale"])
def test_cluster_means_within_derived_bound_on_corpora(cuda, kind, record_property):
    """300 000 rows x 768, K = 256 (64-column chunks, 12 passes, 293 rows per workgroup added in f32): |mean - float64 mean|
    inside cluster_means_bound elementwise, sum of squares inside its summation depth.  Labels: nearest of 256 corpus rows."""
    n, dim, K = 300_000, 768, 256
    x, _ = synth.corpus(kind, cuda, n, dim)
    g = torch.Generator(device=cuda).manual_seed(5)
    centres = x[torch.randperm(n, generator=g, device=cuda)[:K]].contiguous()
    lab = rq.rq_encode(x, centres[None].contiguous()).view(-1)
    _means_within_bound(x, lab, K, record_property, kind)


def test_cluster_means_within_derived_bound_on_long_blocks(cuda, record_property):
    """2 M rows x 64, K = 4, 90 % of the rows in one cluster: 1954 rows per workgroup, ~1760 of them into one f32 accumulator."""
    n, dim, K = 2_000_000, 64, 4
    x, _ = synth.corpus("iid", cuda, n, dim)
    g = torch.Generator(device=cuda).manual_seed(6)
    lab = torch.where(torch.rand((n,), device=cuda, generator=g) < 0.9, torch.full((n,), 2, device=cuda),
                      torch.randint(0, K, (n,), device=cuda, generator=g)).to(torch.int32)
    _means_within_bound(x, lab, K, record_property, "long_blocks")


# ---- distance rows -----------------------------------------------------------------------------------------------------------

def _neg_dist(xt, ct, n, dim, K, out_ptr):
    return hip.lib().mevi_rq_neg_dist_f32(hip.ptr(xt), n, dim, hip.ptr(ct), K, out_ptr, hip.stream_ptr())


@pytest.mark.parametrize("dim", [4, 28, 32, 36, 100, 768])
def test_neg_dist_rows_bit_identical_to_oracle(cuda, dim):
    """The STORE branch over its tails: rows past n in the last 128-row block, centroids past K in the last chunk of 32, a dim
    that is not a multiple of the 32-float slab.  One guard row before and after the [n, K] output must survive."""
    rng = np.random.default_rng(dim)
    for n in (1, 127, 128, 129, 1000):
        for K in (1, 3, 8, 31, 32, 33, 40, 256, 300):
            ties = (n + K) % 2 == 1 and K >= 3
            if ties:                                             # duplicated centroids, small integers: exact ties
                x = rng.integers(-4, 5, size=(n, dim)).astype(np.float32)
                cb = rng.integers(-2, 3, size=(K, dim)).astype(np.float32)
                cb[K - 1] = cb[0]
                cb[2] = cb[1]
            else:
                x = rng.standard_normal((n, dim)).astype(np.float32)
                cb = rng.standard_normal((K, dim)).astype(np.float32)
            xt, ct = _t(x, cuda), _t(cb, cuda)
            buf = torch.full(((n + 2) * K + 64,), SENTINEL, device=cuda)
            hip.check(_neg_dist(xt, ct, n, dim, K, buf.data_ptr() + 4 * K), "mevi_rq_neg_dist_f32")
            codes = rq.rq_encode(xt, ct[None].contiguous(), mode="exact").cpu().numpy()[:, 0]
            out = buf.cpu().numpy()
            got = out[K:(n + 1) * K].reshape(n, K)
            wc, wd = orq.rq_encode(x, cb[None], return_neg_dist=True)
            assert np.array_equal(_bits(got), _bits(wd[:, 0])), (n, K, dim, int((_bits(got) != _bits(wd[:, 0])).sum()))
            assert (out[:K] == SENTINEL).all() and (out[(n + 1) * K:] == SENTINEL).all(), (n, K, dim)
            assert np.array_equal(np.argmax(got, axis=1), codes) and np.array_equal(codes, wc[:, 0])   # lowest index on ties
            if ties:
                assert not np.isin(codes, [2, K - 1]).any() or K == 3


def test_neg_dist_and_gather_sub_refusals(cuda):
    """Misaligned float4 operands, a dim that is not a multiple of 4 and row counts beyond one launch are refused with the
    codes mevi_rq_encode_f32 uses, before anything is launched: the outputs keep their sentinel."""
    n, dim, K = 8, 8, 4
    x = torch.zeros((n + 1) * dim, device=cuda)
    c = torch.zeros((K + 1) * dim, device=cuda)
    out = torch.full((n * max(K, dim) + 8,), SENTINEL, device=cuda)
    src = torch.arange(n, device=cuda)
    code = torch.zeros(n, dtype=torch.int32, device=cuda)
    L, s = hip.lib(), hip.stream_ptr()
    xp, cp, op = x.data_ptr(), c.data_ptr(), out.data_ptr()
    assert xp % 16 == 0 and cp % 16 == 0 and op % 16 == 0
    assert L.mevi_rq_neg_dist_f32(xp + 4, n, dim, cp, K, op, s) == ERR_INVALID_ARG
    assert L.mevi_rq_neg_dist_f32(xp, n, dim, cp + 8, K, op, s) == ERR_INVALID_ARG
    assert L.mevi_rq_neg_dist_f32(xp, n, 6, cp, K, op, s) == ERR_INVALID_ARG
    assert L.mevi_rq_neg_dist_f32(xp, n, dim, None, K, op, s) == ERR_INVALID_ARG
    assert L.mevi_rq_neg_dist_f32(xp, 128 * 0x7fffffff + 1, dim, cp, K, op, s) == ERR_UNSUPPORTED
    assert L.mevi_rq_neg_dist_f32(xp, n, dim, cp, K, op + 4, s) == OK           # the score rows need float alignment only
    assert L.mevi_gather_sub_f32(xp + 4, src.data_ptr(), cp, code.data_ptr(), n, dim, op + 16, s) == ERR_INVALID_ARG
    assert L.mevi_gather_sub_f32(xp, src.data_ptr(), cp + 4, code.data_ptr(), n, dim, op + 16, s) == ERR_INVALID_ARG
    assert L.mevi_gather_sub_f32(xp, src.data_ptr(), cp, code.data_ptr(), n, dim, op + 4, s) == ERR_INVALID_ARG
    assert L.mevi_gather_sub_f32(xp, src.data_ptr(), cp, code.data_ptr(), n, 6, op + 16, s) == ERR_INVALID_ARG
    assert L.mevi_gather_sub_f32(xp, src.data_ptr(), cp, code.data_ptr(), 4 * 0x7fffffff + 1, dim, op + 16, s) == ERR_UNSUPPORTED
    with pytest.raises(hip.MeviHipError):
        hip.check(L.mevi_gather_sub_f32(xp, src.data_ptr(), cp, code.data_ptr(), n, dim, op + 4, s), "mevi_gather_sub_f32")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert o[0] == SENTINEL and (o[1:1 + n * K] == 0).all() and (o[1 + n * K:] == SENTINEL).all()


# ---- residual hand-down --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [4, 100, 252, 256, 260, 768, 1028])
def test_gather_sub_bit_exact(cuda, dim):
    """out[r] = x[src[r]] - c[code[r]] in f32: repeated sources (beam fan-out), a permutation, and the identity written over x
    itself (the form rq.train_rq_codebook relies on).  The rows before and after `out` must survive."""
    rng = np.random.default_rng(dim)
    Kc = 5
    cb = rng.standard_normal((Kc, dim)).astype(np.float32)
    ct = _t(cb, cuda)
    L = hip.lib()
    for n in (1, 3, 4, 5, 1001):
        code = rng.integers(0, Kc, size=n).astype(np.int32)
        variants = {"repeats": rng.integers(0, (n + 1) // 2, size=n), "permutation": rng.permutation(n), "in place": np.arange(n)}
        for name, src in variants.items():
            x = rng.standard_normal((int(src.max()) + 1, dim)).astype(np.float32)
            buf = torch.full((n + 2, dim), SENTINEL, device=cuda)
            if name == "in place":
                buf[1:n + 1] = _t(x, cuda)
                xt = buf[1:n + 1]
            else:
                xt = _t(x, cuda)
            st_, cd_ = _t(src.astype(np.int64), cuda), _t(code, cuda)
            st = L.mevi_gather_sub_f32(xt.data_ptr(), hip.ptr(st_), hip.ptr(ct), hip.ptr(cd_), n, dim, buf[1:].data_ptr(),
                                       hip.stream_ptr())
            hip.check(st, "mevi_gather_sub_f32")
            out = buf.cpu().numpy()
            assert np.array_equal(_bits(out[1:n + 1]), _bits(x[src] - cb[code])), (name, n, dim)
            assert (out[0] == SENTINEL).all() and (out[n + 1] == SENTINEL).all(), (name, n, dim)


def test_training_residual_is_the_level_by_level_difference(cuda, monkeypatch):
    """What rq.train_rq_codebook hands to level j is x minus the chosen centroids of levels < j, subtracted one level at a
    time in f32, bit for bit (the in-place mevi_gather_sub_f32), and `x` itself is left alone."""
    rng = np.random.default_rng(4)
    n, dim, M, K = 3001, 100, 4, 8
    x = rng.standard_normal((n, dim)).astype(np.float32)
    xt = _t(x, cuda)
    seen = []
    real = rq.kmeans

    def spy(res, *a, **kw):
        seen.append(res.clone())
        return real(res, *a, **kw)

    monkeypatch.setattr(rq, "kmeans", spy)
    book, codes = rq.train_rq_codebook(xt, M, K, seed=5, n_init=1, max_iter=4)
    torch.cuda.synchronize()
    assert len(seen) == M and np.array_equal(_bits(xt.cpu().numpy()), _bits(x))
    book, codes, want = book.cpu().numpy(), codes.cpu().numpy(), x.copy()
    for j in range(M):
        assert np.array_equal(_bits(seen[j].cpu().numpy()), _bits(want)), j
        want = want - book[j][codes[:, j]]


# ---- beam_search beyond the goldens --------------------------------------------------------------------------------------------

def _pq_object(shape, pq, cb, cuda):
    n, dim, M, K = shape
    obj = rq.ProductQuantization("pq" if pq else "rq", M, int(np.log2(K)), "l2", dim, device=cuda)
    obj.load_codebook(cb)
    return obj


@pytest.mark.parametrize("shape,pq", [(s, False) for s in ib.BEAM_CASES] + [(s, True) for s in ib.PQ_BEAM_CASES], ids=str)
def test_beam_search_matches_the_chain_reference(cuda, shape, pq):
    """Keep-all levels (row_softmax mode 1) and their hand-over to the top-R step, M = 1, R = 1, K = 256, row counts that
    are no multiple of 128 -- against the float64-softmax restatement under the relative comparison, whose constants come
    from the measured f32-softmax discrepancy (tests/index_build_ref.py)."""
    cases = ib.PQ_BEAM_CASES if pq else ib.BEAM_CASES
    x, cb = ib.beam_case_inputs(shape, pq)
    obj = _pq_object(shape, pq, cb, cuda)
    chain = ib.pq_beam_search_chain if pq else ib.rq_beam_search_chain
    n, dim, M, K = shape
    for R in cases[shape]:
        lab, sc = obj.beam_search(torch.from_numpy(x), R, return_proba=True)
        lab, sc = lab.cpu().numpy(), sc.cpu().numpy()
        wl, ws, cut = chain(x, cb, R, return_cut_gap=True)
        ok, _ = ib.beams_agree_rel(lab, sc, wl, ws, ib.SCORE_RTOL, ib.GAP_RTOL, cut)
        rel = np.abs(sc.astype(np.float64) - ws) / ws
        print(f"{'pq' if pq else 'rq'} {shape} R={R}: max relative score difference {rel[cut > ib.GAP_RTOL].max():.3g}, "
              f"label rows differing {int((lab != wl).any((1, 2)).sum())}")
        assert lab.shape == (n, min(R, K ** M), M) and ok, (shape, R)
        own_ok, own_share = ib.beams_agree_rel(lab, sc, lab, sc, ib.SCORE_RTOL, ib.GAP_RTOL, cut)   # pays for undecided rows too
        assert own_ok and own_share >= ib.FIRM_SHARE_MIN, (shape, R, own_share)
        if R == 1:
            enc = obj.forward(torch.from_numpy(x))[1].cpu().numpy()
            assert np.array_equal(lab[:, 0], enc) and np.array_equal(lab[:, 0], wl[:, 0])


def test_topk_document_mapping_concatenates(cuda):
    shape = (301, 64, 3, 16)
    x, cb = ib.beam_case_inputs(shape)
    obj = _pq_object(shape, False, cb, cuda)
    whole = obj.beam_search(torch.from_numpy(x), 3).cpu()
    parts = [obj.get_topk_document_mapping(x, r, 3, 3, batch_size=100) for r in range(3)]
    assert [len(p) for p in parts] == [100, 100, 101]
    assert torch.equal(torch.cat(parts), whole)
    assert torch.equal(obj.get_topk_document_mapping(torch.from_numpy(x), 0, 1, 3, batch_size=100), whole)


def test_beam_search_refuses_what_the_beam_step_cannot_sort(cuda):
    """R = 100 at K = 256: level 1 would sort 100 * 256 > 16384 candidates.  The refusal surfaces as an error."""
    shape = (67, 96, 2, 256)
    x, cb = ib.beam_case_inputs(shape)
    obj = _pq_object(shape, False, cb, cuda)
    with pytest.raises(hip.MeviHipError, match="16384"):
        obj.beam_search(torch.from_numpy(x), 100, return_proba=True)


# ---- k-means invariants ----------------------------------------------------------------------------------------------------------

def _inertia64(x, centres, labels):
    d = x.double() - centres.double()[labels.long()]
    return float((d * d).sum().item())


@pytest.mark.parametrize("kind", ["clustered", "ance_scale"])
@pytest.mark.parametrize("dim,K", [(64, 16), (64, 256), (768, 16), (768, 256)])
def test_kmeans_invariants(cuda, kind, dim, K, monkeypatch, record_property):
    n = 20_000
    x, _ = synth.corpus(kind, cuda, n, dim, block=4096, n_clusters=300)
    # -- an explicit Lloyd loop: the float64 inertia never rises, neither at an update nor at an assignment
    g = torch.Generator(device=cuda).manual_seed(9)
    centres = x[torch.randperm(n, generator=g, device=cuda)[:K]].contiguous()
    labels = rq.rq_encode(x, centres[None].contiguous(), mode="exact").view(-1)
    trace = [_inertia64(x, centres, labels)]
    for _ in range(5):
        centres, counts, sumsq = rq.cluster_means(x, labels, K, old=centres)
        trace.append(_inertia64(x, centres, labels))
        labels = rq.rq_encode(x, centres[None].contiguous(), mode="exact").view(-1)
        trace.append(_inertia64(x, centres, labels))
    assert all(b <= a for a, b in zip(trace, trace[1:])), trace
    # -- rq.kmeans: labels = exact argmin of the returned centres; the returned inertia against the direct float64 value
    last = {}
    real = rq.cluster_means

    def spy(data, lab, k, old=None):
        last["data"], last["labels"] = data, lab.clone()
        return real(data, lab, k, old=old)

    monkeypatch.setattr(rq, "cluster_means", spy)
    cent, lab, inertia = rq.kmeans(x, K, seed=1, n_init=2, max_iter=20)
    torch.cuda.synchronize()
    assert torch.isfinite(cent).all() and cent.shape == (K, dim)
    assert torch.equal(lab, rq.rq_encode(x, cent[None].contiguous(), mode="exact").view(-1))
    assert last["data"].shape[0] == n                                   # the final update ran on the full data
    direct = _inertia64(x, cent, last["labels"])
    cnt = torch.bincount(last["labels"].long(), minlength=K).double()
    scale = float((cnt * (cent.double() ** 2).sum(1)).sum().item())
    ratio = abs(inertia - direct) / (2 * ib.U32 * scale)
    print(f"{kind} dim={dim} K={K}: inertia {inertia:.6g}, direct {direct:.6g}, |difference| = {ratio:.4f} x bound")
    record_property("inertia_error_over_bound", ratio)
    assert ratio <= 1.0, (inertia, direct, scale)


def test_kmeans_with_more_centres_than_distinct_points(cuda):
    rng = np.random.default_rng(1)
    base = rng.standard_normal((10, 64)).astype(np.float32)
    x = _t(base[rng.integers(0, 10, size=500)], cuda)
    cent, lab, inertia = rq.kmeans(x, 16, seed=0, n_init=2, max_iter=10)
    torch.cuda.synchronize()
    assert torch.isfinite(cent).all() and np.isfinite(inertia)
    assert torch.equal(lab, rq.rq_encode(x, cent[None].contiguous(), mode="exact").view(-1))
    assert _inertia64(x, cent, lab) <= 1e-9                              # every point sits on a centre
