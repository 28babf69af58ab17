"""Split-precision GEMM (csrc/gemm_split.hip: three f16 MFMAs per product on (hi, lo) float16 row images) against a
float64 reference.  Bar (stated per assertion): |error| <= 2e-6 * sum_k |a_k w_k| per output -- the f32 chain's own
worst case at these K is ~4e-7 of that sum, the split form measures ~1.5e-7 --, every epilogue, both kernels (tile
stream / few-rows), ragged shapes, strided outputs; and a row gives the same BITS alone or inside a large batch."""
import numpy as np
import pytest
import torch

from mevi_amd import ops

pytestmark = pytest.mark.gpu
TOL = 2e-6


def _ref(x, w, bias, act, residual):
    y = x.double() @ w.double().T
    den = x.double().abs() @ w.double().abs().T
    if bias is not None:
        y, den = y + bias.double(), den + bias.double().abs()
    if act == "relu":
        y = torch.relu(y)
    elif act == "gelu":
        y = torch.nn.functional.gelu(y)
    if residual is not None:
        y, den = y + residual.double(), den + residual.double().abs()
    return y, den


def _image_value(s):
    """f64 value of a SplitRows image: 2^-e (hi + lo)."""
    kp = s.img.shape[1] // 2
    h = s.img.view(torch.float16).double()
    return ((h[:, :kp] + h[:, kp:]) * torch.exp2(-s.exp.double())[:, None])[:, :s.k]


@pytest.mark.parametrize("M,N,K", [(3000, 768, 768), (517, 100, 36), (256, 96, 32), (1030, 2304, 768), (7, 3072, 768),
                                   (70000, 256, 64), (300, 36, 64), (1, 768, 3072), (2100, 260, 2048),
                                   (5, 100, 96), (300, 36, 152), (40, 64, 220), (3000, 800, 96)])   # Kp = 96, 160, 224: not whole 64-k chunks
def test_split_gemm_matches_float64(cuda, M, N, K):
    g = torch.Generator(device=cuda).manual_seed(M + N + K)
    x = torch.randn((M, K), device=cuda, generator=g) * torch.exp(2 * torch.randn((M, 1), device=cuda, generator=g))
    w = torch.randn((N, K), device=cuda, generator=g) * K ** -0.5 * torch.exp(torch.randn((N, 1), device=cuda, generator=g))
    b = torch.randn((N,), device=cuda, generator=g)
    r = torch.randn((M, N), device=cuda, generator=g)
    ws = ops.split_rows(w)
    xs = ops.split_rows(x)
    assert (_image_value(xs) - x.double()).abs().max() <= 2.0 ** -21 * x.abs().max()      # 22-bit operand images
    for kw, act in ((dict(), None), (dict(bias=b, relu=True), "relu"), (dict(bias=b, gelu=True), "gelu"),
                    (dict(residual=r), None), (dict(bias=b, residual=r), None)):
        got = ops.linear(xs, ws, **kw)
        ref, den = _ref(x, w, kw.get("bias"), act, kw.get("residual"))
        assert torch.isfinite(got).all()
        err = ((got.double() - ref).abs() / den.clamp_min(1e-30)).max().item()
        assert err <= TOL, (sorted(kw), err)
        assert torch.equal(ops.linear(x, ws, **kw), got)                                     # f32 input: split on the way in


@pytest.mark.parametrize("M,N,K", [(3000, 3072, 768), (300, 64, 32), (5, 2048, 768), (1100, 100, 768)])
@pytest.mark.parametrize("act", ["relu", "gelu", None])
def test_gemm_writing_a_split_image(cuda, M, N, K, act):
    """linear(..., for_gemm=True): the result as the next GEMM's operand image (exponent from the Cauchy-Schwarz
    bound): its value equals the f32 result to 22 bits of the row BOUND, and feeding it on gives the second layer."""
    g = torch.Generator(device=cuda).manual_seed(M + N)
    x = torch.randn((M, K), device=cuda, generator=g) * torch.exp(torch.randn((M, 1), device=cuda, generator=g))
    w1 = torch.randn((N, K), device=cuda, generator=g) * K ** -0.5
    b1 = torch.randn((N,), device=cuda, generator=g) * 0.1
    w2 = torch.randn((40, N), device=cuda, generator=g) * N ** -0.5
    xs, w1s, w2s = ops.split_rows(x), ops.weight_split(w1), ops.weight_split(w2)
    kw = dict(bias=b1, relu=act == "relu", gelu=act == "gelu")
    h32 = ops.linear(xs, w1s, **kw)
    hs = ops.linear(xs, w1s, for_gemm=True, **kw)
    assert isinstance(hs, ops.SplitRows) and hs.shape == (M, N)
    hv = _image_value(hs)
    bound = torch.exp2(15 - hs.exp.double())[:, None]                      # the row's exponent puts the bound below 2^15
    assert (h32.double().abs() <= bound).all()
    assert ((hv - h32.double()).abs() <= bound * 2.0 ** -36 + h32.double().abs() * 2.0 ** -21).all()
    assert (hs.norm.double() >= torch.linalg.vector_norm(h32.double(), dim=1)).all()
    y = ops.linear(hs, w2s)
    ref, den = _ref(h32, w2, None, None, None)
    assert ((y.double() - ref).abs() / den.clamp_min(1e-30)).max().item() <= TOL


def test_rows_keep_their_bits_in_any_batch(cuda):
    """Few rows (gemm_split_skinny_kernel) and the same rows inside a large batch (the tile stream): identical bits,
    for the f32 and the image output, with every epilogue."""
    g = torch.Generator(device=cuda).manual_seed(5)
    x = torch.randn((4000, 768), device=cuda, generator=g)
    b = torch.randn((3072,), device=cuda, generator=g)
    r = torch.randn((4000, 768), device=cuda, generator=g)
    wi, wo = ops.weight_split(torch.randn((3072, 768), device=cuda, generator=g) * 768 ** -0.5), \
        ops.weight_split(torch.randn((768, 3072), device=cuda, generator=g) * 3072 ** -0.5)
    xs = ops.split_rows(x)
    h = ops.linear(xs, wi, bias=b, relu=True, for_gemm=True)
    y = ops.linear(h, wo, residual=r)
    for m in (1, 5, 33, 100):
        hm = ops.linear(xs[:m], wi, bias=b, relu=True, for_gemm=True)
        assert torch.equal(hm.img, h.img[:m]) and torch.equal(hm.exp, h.exp[:m]) and torch.equal(hm.norm, h.norm[:m])
        assert torch.equal(ops.linear(hm, wo, residual=r[:m]), y[:m])
        assert torch.equal(ops.linear(xs[:m], wi, bias=b, relu=True), ops.linear(xs, wi, bias=b, relu=True)[:m])


def test_rows_keep_their_bits_across_tile_heights_and_the_row_split(cuda):
    """Round 5: the tile stream runs 256 / 128 / 64 activation rows per tile (chosen per GEMM by its tile rounds) and cuts GEMMs of
    several rounds into whole rounds + a remainder launch.  Whatever batch a row travels in -- 600 ... 20 000 rows from the head
    or the middle of a 70 000-row batch -- it has the bits it has in the big batch: f32 + residual, plain f32, and the image."""
    g = torch.Generator(device=cuda).manual_seed(11)
    M = 70000
    x = torch.randn((M, 768), device=cuda, generator=g)
    r = torch.randn((M, 768), device=cuda, generator=g)
    b = torch.randn((2304,), device=cuda, generator=g)
    wo = ops.weight_split(torch.randn((768, 768), device=cuda, generator=g) * 768 ** -0.5)
    wq = ops.weight_split(torch.randn((2304, 768), device=cuda, generator=g) * 768 ** -0.5)
    xs = ops.split_rows(x)
    y = ops.linear(xs, wo, residual=r)
    q = ops.linear(xs, wq, bias=b)
    h = ops.linear(xs, wq, bias=b, relu=True, for_gemm=True)
    for lo, m in ((0, 600), (0, 873), (0, 1418), (0, 2048), (0, 4096), (0, 9600), (0, 20000), (30000, 873), (41111, 5000), (69000, 1000)):
        sub = xs[lo:lo + m]
        assert torch.equal(ops.linear(sub, wo, residual=r[lo:lo + m]), y[lo:lo + m]), (lo, m)
        assert torch.equal(ops.linear(sub, wq, bias=b), q[lo:lo + m]), (lo, m)
        hm = ops.linear(sub, wq, bias=b, relu=True, for_gemm=True)
        assert torch.equal(hm.img, h.img[lo:lo + m]) and torch.equal(hm.exp, h.exp[lo:lo + m]), (lo, m)


def test_strided_output_and_fused_rmsnorm(cuda):
    g = torch.Generator(device=cuda).manual_seed(9)
    x = torch.randn((1500, 768), device=cuda, generator=g) * 30
    lnw = 1 + 0.1 * torch.randn((768,), device=cuda, generator=g)
    w = ops.weight_split(torch.randn((1536, 768), device=cuda, generator=g) * 768 ** -0.5)
    h = ops.rmsnorm(x, lnw, 1e-6)
    old = ops.GEMM_MODE
    try:
        ops.GEMM_MODE = "split"
        hs = ops.rmsnorm(x, lnw, 1e-6, for_gemm=True)                       # the norm written as an operand image
    finally:
        ops.GEMM_MODE = old
    ref = ops.split_rows(h)
    assert torch.equal(hs.img, ref.img) and torch.equal(hs.exp, ref.exp) and torch.equal(hs.norm, ref.norm)
    cache = torch.full((1500, 5, 1536), float("nan"), device=cuda)
    ops.linear(hs, w, out=cache[:, 2, :])                                   # the decoder's K|V cache slot
    assert torch.equal(cache[:, 2, :], ops.linear(hs, w)) and torch.isnan(cache[:, 1, :]).all() and torch.isnan(cache[:, 3, :]).all()


def test_extreme_rows(cuda):
    """Row scaling across the f32 range: all-zero rows, rows of magnitude 1e-30 and 1e+30 (exponents at the int8 clamp
    region), one huge element beside tiny ones -- same 2e-6 bar relative to sum |a||w|; non-finite inputs stay non-finite
    in their own rows only."""
    g = torch.Generator(device=cuda).manual_seed(11)
    M, N, K = 700, 256, 512
    x = torch.randn((M, K), device=cuda, generator=g)
    x[0] = 0
    x[1] *= 1e-30
    x[2] *= 1e30
    x[3, 1:] *= 1e-6
    x[3, 0] = 5e4
    w = torch.randn((N, K), device=cuda, generator=g) * K ** -0.5
    w[7] = 0
    w[8] *= 1e-5                    # (1e-30 rows x this column stay above the f32 underflow any GEMM would hit)
    got = ops.linear(ops.split_rows(x), ops.split_rows(w))
    ref, den = _ref(x, w, None, None, None)
    assert torch.isfinite(got).all() and (got[0] == 0).all() and (got[:, 7] == 0).all()
    err = ((got.double() - ref).abs() / den.clamp_min(1e-300))
    err[0], err[:, 7] = 0, 0
    assert err.max().item() <= TOL
    x[5, 9], x[6, 3] = float("inf"), float("nan")
    got = ops.linear(ops.split_rows(x), ops.split_rows(w))
    bad = ~torch.isfinite(got)
    assert bad[5].any() and bad[6].any() and not bad[[0, 1, 2, 3, 4, 7, 8]].any()


def test_norm_and_projection_in_one_kernel_keep_the_two_kernel_bits(cuda, monkeypatch):
    """mevi_gemm_nt_rmsnorm_split_* (the latency path: every workgroup normalises its rows itself) against
    mevi_rmsnorm_split_f16 + mevi_gemm_nt_split_*: identical outputs -- f32 with bias / relu / residual / strided output, and
    the image-writing form (image, exponents, norms) -- for 1 .. 40 rows; unsupported shapes fall back silently."""
    monkeypatch.setattr(ops, "FUSE_NORM", True)       # off by default (measured no faster): MEVI_FUSE_NORM=1
    g = torch.Generator(device=cuda).manual_seed(21)
    rnd = lambda *s_: torch.randn(s_, device=cuda, generator=g)      # noqa: E731
    lnw = 1 + 0.1 * rnd(768)
    for M, N in ((1, 768), (10, 2304), (11, 3072), (32, 768), (33, 1536), (40, 1536)):
        x = rnd(M, 768) * torch.exp(rnd(M, 1))
        w = ops.weight_split(rnd(N, 768) * 768 ** -0.5)
        b, r = rnd(N) * 0.1, rnd(M, N)
        assert ops.FUSE_NORM and hip_lib().mevi_gemm_rmsnorm_supported(M, N, 768)
        two = lambda **kw: ops.linear(ops._rmsnorm_split(x, lnw, 1e-6), w, **kw)         # noqa: E731
        one = lambda **kw: ops.linear(ops.rmsnorm(x, lnw, 1e-6, for_gemm=True), w, **kw)  # noqa: E731
        assert isinstance(ops.rmsnorm(x, lnw, 1e-6, for_gemm=True), ops.NormedRows)
        for kw in ({}, {"bias": b}, {"bias": b, "relu": True}, {"residual": r}, {"bias": b, "residual": r, "gelu": True}):
            assert torch.equal(one(**kw), two(**kw)), (M, N, sorted(kw))
        big = torch.full((M, 3, N), float("nan"), device=cuda)
        one(out=big[:, 1, :])
        assert torch.equal(big[:, 1, :], two()) and torch.isnan(big[:, 0, :]).all()
        h1, h2 = one(bias=b, relu=True, for_gemm=True), two(bias=b, relu=True, for_gemm=True)
        assert torch.equal(h1.img, h2.img) and torch.equal(h1.exp, h2.exp) and torch.equal(h1.norm, h2.norm)
    # not on the fused path: many rows (the tile stream), another width -- the lazy rows materialise, same results
    x = rnd(3000, 768)
    w = ops.weight_split(rnd(768, 768) * 0.03)
    nr = ops.rmsnorm(x[:300], lnw, 1e-6, for_gemm=True)
    assert not isinstance(nr, ops.NormedRows) or torch.equal(ops.linear(nr, w), ops.linear(ops._rmsnorm_split(x[:300], lnw, 1e-6), w))
    assert isinstance(ops.rmsnorm(x, lnw, 1e-6, for_gemm=True), ops.SplitRows)


def hip_lib():
    from mevi_amd import hip

    return hip.lib()


# ---- the folded T5LayerNorm (ops.ResidualRows: residual_start, linear_normed, linear_residual) against float64 ----------------------
# Bars: the image of a stream row decodes to x within 2^-21 of the binade of the row's exponent (2^(15 - e) is the power of two above
# the bound the exponent was taken from); bound >= max |row|; a 16-column block sum of squares is an f32 fma chain of 4 plus two adds,
# within 8 f32 ulps of the float64 sum of the same 16 f32 values (f32-rounded: rows of 1e30 overflow to inf in f32, as in the
# reference's own x.pow(2)); products under the GEMM bar 2e-6 sum |a||w| -- with the norm folded, |a| is |rmsnorm(x)| and the f32 row
# scale adds a few ulps of |y| <= that sum.


def _stream_rows(M, D, g, extremes=True):
    """Rows with the residual stream's statistics: scale 5-20, a handful of channels 50-100x the rest; zero rows and rows of
    1e-30 / 1e30 when `extremes`."""
    x = torch.randn((M, D), device="cuda", generator=g) * (5 + 15 * torch.rand((M, 1), device="cuda", generator=g))
    x[:, [c for c in (3, 100, 401, 700, 1000) if c < D]] *= 75
    if extremes and M >= 4:
        x[1] = 0
        x[2] *= 1e-30
        x[3] *= 1e30
    return x


def _check_stream(r, x64=None, tag=""):
    """image vs x, bound >= max |row|, ssq vs float64 of the returned (or given) f32 rows."""
    x = r.x.double()
    D = r.x.shape[1]
    img = _image_value(ops.SplitRows(r.img, r.exp, D))
    binade = torch.exp2(15 - r.exp.double())[:, None]
    assert ((img - x).abs() <= 2.0 ** -21 * binade).all(), tag
    assert (r.bound.double() >= x.abs().amax(1)).all(), tag
    ref = (x.view(x.shape[0], D // 16, 16) ** 2).sum(2).float().double()
    got = r.ssq.double()
    inf = torch.isinf(ref)
    assert torch.equal(torch.isinf(got), inf), tag
    assert ((got - ref).abs()[~inf] <= 8 * 2.0 ** -24 * ref[~inf] + 2.0 ** -140).all(), tag
    if x64 is not None:
        assert torch.equal(r.x, x64.float()) if x64.dtype == torch.float32 else True


@pytest.mark.parametrize("D", [16, 32, 768, 1024])
def test_residual_start_image_bound_and_block_sums(cuda, D):
    """mevi_split_rows_ssq_f16: ragged row counts, a strided ldx, zero rows, rows of 1e-30 / 1e30."""
    g = torch.Generator(device=cuda).manual_seed(D)
    for M in (1, 7, 333):
        x = _stream_rows(M, D, g)
        r = ops.residual_start(x)
        assert r.ssq.shape == (M, D // 16) and r.bound.shape == (M,)
        _check_stream(r, tag=(D, M))
        big = torch.full((M, D + 48), float("nan"), device=cuda)
        big[:, 16:16 + D] = x
        rs = ops.residual_start(big[:, 16:16 + D])                          # ldx = D + 48
        assert torch.equal(rs.img, r.img) and torch.equal(rs.exp, r.exp) and torch.equal(rs.bound, r.bound)
        assert torch.equal(rs.ssq, r.ssq)
    if D >= 4:
        assert (r.ssq[1] == 0).all() and r.bound[1] == 0


def _rms64(x, ln, eps):
    x = x.double()
    return x * torch.rsqrt(x.pow(2).mean(1, keepdim=True) + eps) * ln.double()


@pytest.mark.parametrize("N", [768, 2304, 3072])
def test_linear_normed_against_float64(cuda, N):
    """act(rmsnorm(x) (W (.) w_ln)^T + b) from the stream's image and block sums: f32 and image outputs, 7 / 300 / 5000 rows (the
    latency kernels and the tile stream) against float64 rmsnorm(x) W^T."""
    K, eps = 768, 1e-6
    g = torch.Generator(device=cuda).manual_seed(N)
    ln = torch.exp(0.5 * torch.randn((K,), device=cuda, generator=g))
    ln[[5, 77, 600]] = torch.tensor([12.0, 25.0, 30.0], device=cuda)
    w = torch.randn((N, K), device=cuda, generator=g) * K ** -0.5
    b = torch.randn((N,), device=cuda, generator=g) * 0.1
    ws = ops.weight_split(ops.fold_weight(w, ln))
    for M in (7, 300, 5000):
        x = _stream_rows(M, K, g, extremes=False)
        x[1] = 0                                                           # rmsnorm of a zero row: 0 (eps)
        r = ops.residual_start(x)
        h64 = _rms64(x, ln, eps)
        ref, den = h64 @ w.double().T, h64.abs() @ w.double().abs().T
        got = ops.linear_normed(r, ws, eps)
        assert torch.isfinite(got).all() and (got[1] == 0).all()
        err = ((got.double() - ref).abs() / den.clamp_min(1e-30)).max().item()
        assert err <= TOL, (M, N, err)
        hs = ops.linear_normed(r, ws, eps, bias=b, relu=True, for_gemm=True)
        refb = torch.relu(ref + b.double())
        hv = _image_value(hs)
        binade = torch.exp2(15 - hs.exp.double())[:, None]
        assert ((hv - refb).abs() <= TOL * (den + b.double().abs()) + 2.0 ** -21 * binade).all(), (M, N)
        assert (hs.norm.double() >= torch.linalg.vector_norm(refb, dim=1) * (1 - 1e-5)).all()
        if M == 300:                                                         # the bar is not loose: an unnormed product misses it
            assert ((ops.linear(ops.split_rows(x), ws).double() - ref).abs() / den.clamp_min(1e-30)).max() > 1e-3


def _residual_case(cuda, N, K, M, seed):
    g = torch.Generator(device=cuda).manual_seed(seed)
    x = _stream_rows(M, N, g, extremes=False)
    a = torch.relu(torch.randn((M, K), device=cuda, generator=g)) * torch.exp(torch.randn((M, 1), device=cuda, generator=g))
    w = torch.randn((N, K), device=cuda, generator=g) * K ** -0.5
    w[[3, 100]] *= 60                                                      # rows that write the outlier channels
    return x, a, w


@pytest.mark.parametrize("N,K", [(768, 768), (768, 3072), (1024, 768), (1024, 3072)])
def test_linear_residual_against_float64(cuda, N, K):
    """x + a W^T as ResidualRows, a with per-row norms and with one norm_max for all rows, and (K == N) the one-position decoder's
    x + rmsnorm(x) W^T (normed_eps): x against float64, the image against x, bound >= max |x|, ssq against float64 of the returned
    x -- on a 70 000-row batch; rows 1, 7, 33, 300, 5000 (from its head and its middle) have the same bits alone."""
    M, eps = 70000, 1e-6
    x, a, w = _residual_case(cuda, N, K, M, seed=N + K)
    r = ops.residual_start(x)
    ws = ops.weight_split(w)
    a_s = ops.split_rows(a)
    a_c = ops.SplitRows(a_s.img, a_s.exp, K, None, float(a_s.norm.max()) * 1.0001)
    forms = {"rows": (a_s, None), "norm_max": (a_c, None)}
    ref_of = {"rows": lambda: x.double() + a.double() @ w.double().T}
    den_of = {"rows": lambda: x.double().abs() + a.double().abs() @ w.double().abs().T}
    ref_of["norm_max"], den_of["norm_max"] = ref_of["rows"], den_of["rows"]
    if K == N:
        ln = torch.exp(0.5 * torch.randn((N,), device=cuda))
        wf = ops.weight_split(ops.fold_weight(w, ln))
        forms["normed"] = (r, wf)
        ref_of["normed"] = lambda: x.double() + _rms64(x, ln, eps) @ w.double().T
        den_of["normed"] = lambda: x.double().abs() + _rms64(x, ln, eps).abs() @ w.double().abs().T
    for name, (opnd, wf) in forms.items():
        wgt = ws if wf is None else wf
        kw = dict(normed_eps=eps) if name == "normed" else {}
        out = ops.linear_residual(opnd, wgt, r, **kw)
        err = ((out.x.double() - ref_of[name]()).abs() / den_of[name]().clamp_min(1e-30)).max().item()
        assert err <= TOL, (name, N, K, err)
        _check_stream(out, tag=(name, N, K))
        for lo, m in ((0, 1), (0, 7), (0, 33), (0, 300), (0, 5000), (33333, 300), (41111, 5000)):
            rm = ops.ResidualRows(r.x[lo:lo + m], r.img[lo:lo + m], r.exp[lo:lo + m], r.bound[lo:lo + m], r.ssq[lo:lo + m])
            om = rm if name == "normed" else opnd[lo:lo + m]
            sub = ops.linear_residual(om, wgt, rm, **kw)
            for f in ("x", "img", "exp", "bound", "ssq"):
                assert torch.equal(getattr(sub, f), getattr(out, f)[lo:lo + m]), (name, lo, m, f)


def test_folded_stream_through_24_sub_layers(cuda, record_property):
    """12 blocks of t5-base shape on the folded stream, alternating linear_normed and linear_residual: q|k|v-like
    projection -> (its v third as the context) -> o, then relu(wi) as an image -> wo.  The carried bound grows by ||a|| wnorm_max
    at every add and is never re-measured: its drift above the true max |x| is recorded (binades), it never falls below, and
    the final stream is within the per-sub-layer bar of a float64 run of the same chain (each GEMM's error 2e-6 sum |a||w| of
    its own inputs, accumulated: the reference is fed the HIP stream's inputs at every sub-layer, so the bar checks each step
    at the end of a deep chain, where the image is coarsest)."""
    D, FFW, M, eps = 768, 3072, 512, 1e-6
    g = torch.Generator(device=cuda).manual_seed(24)
    x = _stream_rows(M, D, g, extremes=False)
    x[1] = 0
    r = ops.residual_start(x)
    drift, errs = [], []
    for l in range(12):
        ln0, ln1 = [torch.exp(0.5 * torch.randn((D,), device=cuda, generator=g)) for _ in range(2)]
        ln0[l * 7] = ln1[l * 11 + 1] = 20.0
        wv = torch.randn((D, D), device=cuda, generator=g) * D ** -0.5
        wo = torch.randn((D, D), device=cuda, generator=g) * D ** -0.5
        wi = torch.randn((FFW, D), device=cuda, generator=g) * D ** -0.5
        w2 = torch.randn((D, FFW), device=cuda, generator=g) * FFW ** -0.5
        wo[[3, 100]] *= 60
        w2[[401, 700]] *= 60
        for wn, ln, wout, relu in ((wv, ln0, wo, False), (wi, ln1, w2, True)):
            x64 = r.x.double()
            h64 = _rms64(r.x, ln, eps) @ wn.double().T
            dh = _rms64(r.x, ln, eps).abs() @ wn.double().abs().T
            if relu:
                h64 = torch.relu(h64)
                h = ops.linear_normed(r, ops.weight_split(ops.fold_weight(wn, ln)), eps, relu=True, for_gemm=True)
                hv = _image_value(h)
            else:
                hf = ops.linear_normed(r, ops.weight_split(ops.fold_weight(wn, ln)), eps)
                h, hv = ops.split_rows(hf), hf.double()
            assert ((hv - h64).abs() <= 2 * TOL * dh + 2.0 ** -21 * hv.abs().amax(1, keepdim=True)).all(), l
            r = ops.linear_residual(h, ops.weight_split(wout), r)
            ref = x64 + hv @ wout.double().T
            den = x64.abs() + hv.abs() @ wout.double().abs().T
            errs.append(((r.x.double() - ref).abs() / den.clamp_min(1e-30)).max().item())
            assert errs[-1] <= TOL, (l, relu, errs[-1])
            _check_stream(r, tag=(l, relu))
            live = r.x.abs().amax(1) > 0
            drift.append(torch.log2(r.bound[live].double() / r.x[live].abs().amax(1).double()).max().item())
    record_property("bound_drift_binades", drift)
    record_property("sub_layer_errors", errs)
    print("bound drift (binades) per sub-layer:", [round(d, 2) for d in drift])
    assert min(drift) >= 0
