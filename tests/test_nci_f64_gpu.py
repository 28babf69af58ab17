"""The seq2seq arm's adaptor (nci.Adaptor) and PAWA head (NCIModel._logits, ops.head_logits, ops.adaptive_logits_rows,
PrefixTables) at t5-base width (d 768, ff 3072, 12 x 64 heads; adaptor: 8 heads of 96, FFN 2048) against the float64
restatement (tests/nci_ref64.py) applied to the same f32 inputs, in every form the model evaluates them in:

  (a) Adaptor.step on the plain cache, 1 and 4 layers, positions 0..4, 1 .. 2000 rows (every GEMM launcher), both GEMM
      modes, and a narrow adaptor (d 256: add_layernorm's LDS path);
  (b) ids of 8 codes: up to 9 keys in the adaptor's self-attention;
  (c) every row of the prefix tables (head matrices, adaptor vectors, K|V) in each regime of the byte budget;
  (d) the head alone at its dispatch edges: fused / unfused GEMM + finish, the rows kernels over a table, the column form;
  (e) every decode position of generate(), in each regime, against the full-prefix reference of the beams the search
      itself follows (so near-ties cannot make the two diverge);
  (f) controls: a reference with one layer-norm gain (or alpha) off by 1e-3 misses the bar.

Bar (tests/f64_bar.py; derivation in tests/test_t5_f64_gpu.py): e_hip <= 4 e_32 + 2^-22 max |ref64| over ALL rows, with
ref64 on the GPU and ref32 on the host from the same f32 inputs; e_hip, e_32 and the bar are recorded per comparison.

Weights.  The T5 part is test_t5_f64_gpu.realistic_weights (2 + 2 layers).  The adaptor part has the statistics of trained
checkpoints that the seeded initialiser lacks: log-normal LN gains with a few entries of 10-30, LN biases up to O(1),
projection biases of O(0.1), a handful of channels 50-100x the rest in decode_embeddings and in the rows of out_proj and
linear2 that write them, one all-zero decode_embeddings row that is a code token (ZERO_TOK, used in every batch),
adaptor_linear at scale d^-0.5 with a few output rows x 30, lm_head of O(1)."""
import sys

import numpy as np
import pytest
import torch

import f64_bar
import nci_ref64 as n64
import t5_ref64 as r64
import test_t5_f64_gpu as t5f
from f64_bar import check, refs
from mevi_amd import hip, nci, ops

pytestmark = pytest.mark.gpu
D, FFA = 768, 2048
ZERO_TOK = 3                       # 2 + 0 * K + 1: code 1 of position 0
SKINNY_MAX = 1500000               # gemm_split.hip: SPLIT_SKINNY_MAX_OUTPUTS
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def release_what_this_module_cached():
    """The weights (host: up to 600 MB a piece) and float64 references (device) are shared inside this module only."""
    before = set(f64_bar._CACHE)
    yield
    for key in set(f64_bar._CACHE) - before:
        del f64_bar._CACHE[key]
    _CACHE.clear()


# ---- weights ---------------------------------------------------------------------------------------------------------------
def adaptor_weights(M, K, d=D, layers=2, seed=1, head=True):
    """state_dict-named adaptor / head weights (CPU f32) with the statistics of the module docstring."""
    key = ("aw", M, K, d, layers, seed, head)
    if key in _CACHE:
        return _CACHE[key]
    g = torch.Generator().manual_seed(seed + 1000 * M + K)
    rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    V = K * (M + 2) + 2
    big = torch.ones(d)
    big[torch.randperm(d, generator=g)[:5]] = 50 + 50 * torch.rand(5, generator=g)

    def ln():
        w = torch.exp(0.5 * rn(d))
        w[torch.randperm(d, generator=g)[:4]] = 10 + 20 * torch.rand(4, generator=g)
        b = 0.3 * rn(d)
        b[torch.randperm(d, generator=g)[:4]] = torch.tensor([1.0, -1.0, 1.5, -0.8])
        return w, b

    emb = rn(V, d) * big
    emb[ZERO_TOK] = 0
    W = {"decode_embeddings.weight": emb, "adaptor_embeddings": torch.rand(1, 1, d, generator=g)}
    for l in range(layers):
        p = f"adaptor.layers.{l}"
        for a in ("self_attn", "multihead_attn"):
            W[f"{p}.{a}.in_proj_weight"], W[f"{p}.{a}.in_proj_bias"] = rn(3 * d, d) * d ** -0.5, 0.1 * rn(3 * d)
            W[f"{p}.{a}.out_proj.weight"], W[f"{p}.{a}.out_proj.bias"] = rn(d, d) * d ** -0.5 * big[:, None], 0.1 * rn(d)
        W[f"{p}.linear1.weight"], W[f"{p}.linear1.bias"] = rn(FFA, d) * d ** -0.5, 0.1 * rn(FFA)
        W[f"{p}.linear2.weight"], W[f"{p}.linear2.bias"] = rn(d, FFA) * FFA ** -0.5 * big[:, None], 0.1 * rn(d)
        for n_ in (1, 2, 3):
            W[f"{p}.norm{n_}.weight"], W[f"{p}.norm{n_}.bias"] = ln()
    if head:
        al = rn(d * V, d) * d ** -0.5
        for i, v in zip(torch.randint(0, d, (6,), generator=g).tolist(), (1, 2, 2 + K, 3, 2 + M * K, 2 + (M - 1) * K + K - 1)):
            al[i * V + v] *= 30                          # output rows (head-matrix entries) of valid columns
        W["adaptor_linear.weight"] = al
        W["lm_head.weight"] = rn(V, d)
    _CACHE[key] = W
    return W


def model_weights(M, K, layers=2):
    """(weights, cfg dict) of a whole NCI model: realistic T5 (2 encoder, 2 decoder layers) + the adaptor part."""
    key = ("mw", M, K, layers)
    if key not in _CACHE:
        W = dict(t5f.realistic_weights(2, 2))
        W.update(adaptor_weights(M, K, D, layers))
        _CACHE[key] = (W, dict(t5f.cfg(2, 2), M=M, K=K, adaptor_layer_num=layers))
    return _CACHE[key]


def cast(W, dt, dev):
    """r64.cast, once per (weights, dtype, device)."""
    key = ("cast", id(W), dt, str(dev))
    if key not in _CACHE:
        _CACHE[key] = (W, r64.cast(W, dt, dev))       # W kept: its id stays taken
    return _CACHE[key][1]


def prefix_tokens(codes, K):
    """codes i64 [n, p] -> decoder tokens [n, p + 1]: 0, then 2 + jK + code."""
    n, p = codes.shape
    return np.concatenate([np.zeros((n, 1), np.int64), 2 + np.arange(p)[None, :] * K + codes], 1)


def teacher_tokens(n, T, K, seed):
    tok = prefix_tokens(np.random.default_rng(seed).integers(0, K, (n, T - 1)), K)
    tok[0, 1] = ZERO_TOK
    return torch.from_numpy(tok)


def misses(hip_out, ref64, ref32):
    """f64_bar.check's rule, as a predicate (the controls)."""
    hip_out, ref64, ref32 = hip_out.double().cpu(), ref64.double().cpu(), ref32.double().cpu()
    e_hip, e_32 = (hip_out - ref64).abs().max().item(), (ref32 - ref64).abs().max().item()
    return e_hip > 4.0 * e_32 + 2.0 ** -22 * ref64.abs().max().item()


def perturbed(W, name):
    """W with the largest entry of the layer-norm gain `name` raised by 1e-3 relative."""
    key = ("pert", id(W), name)
    if key not in _CACHE:
        w = W[name].clone()
        w[w.abs().argmax()] *= 1.001
        _CACHE[key] = dict(W, **{name: w})
    return _CACHE[key]


# ---- (a), (b): Adaptor.step on the plain cache ----------------------------------------------------------------------------
def gemm_launcher(m, n):
    """gemm_split_launch's choice for an [m, n] output."""
    if m * n > SKINNY_MAX:
        return "stream"
    return "t16" if ((n + 31) // 32) * ((m + 31) // 32) <= 128 else "t32"


def test_row_counts_straddle_the_gemm_launchers():
    used = {(N, gemm_launcher(m, N)) for m in ROWS for N in (D, 2 * D, FFA)}
    assert used == {(N, k) for N in (D, 2 * D, FFA) for k in ("t16", "t32", "stream")}


def adaptor_hip(cuda, d, layers, n, T, K, mode="split"):
    """Adaptor.step at t = 0 .. T-1 on new_cache(n) under teacher-forced tokens: (outputs [n, T, d], caches), computed once."""
    key = ("hip_a", d, layers, n, T, K, mode)
    if key not in _CACHE:
        assert ops.GEMM_MODE == mode
        W = adaptor_weights(T - 1, K, d, layers, head=False)
        ad = nci.Adaptor(W, nci.NCIConfig(M=T - 1, K=K, adaptor_layer_num=layers, d_model=d), cuda)
        assert isinstance(ad.layers[0]["wq"], ops.SplitRows) == (mode == "split")
        tok = teacher_tokens(n, T, K, seed=n)
        emb = W["decode_embeddings.weight"].to(cuda)
        cache = ad.new_cache(n)
        outs = [ad.step(emb[tok[:, t].to(cuda)].contiguous(), t, cache) for t in range(T)]
        _CACHE[key] = (torch.stack(outs, 1).cpu(), [c.cpu() for c in cache])
    return _CACHE[key]


def adaptor_refs(d, layers, n, T, K, W=None, tag=""):
    Wa = adaptor_weights(T - 1, K, d, layers, head=False) if W is None else W
    tok = teacher_tokens(n, T, K, seed=n)
    cfg = dict(d_model=d, adaptor_layer_num=layers)

    def run(dt, dev):
        Wd = cast(Wa, dt, dev)
        out, _, kvs = n64.adaptor(Wd, cfg, Wd["decode_embeddings.weight"][tok.to(dev)])
        return out, kvs[0]

    return refs(("adaptor", d, layers, n, T, K, tag), run)


ROWS = [1, 10, 65, 161, 800, 2000]


def _adaptor_case(cuda, record_property, d, layers, n, T, K, mode, positions, name):
    got, cache = adaptor_hip(cuda, d, layers, n, T, K, mode)
    (ref64, kv64), (ref32, kv32) = adaptor_refs(d, layers, n, T, K)
    for t in positions:
        check(f"{name}/t{t}", got[:, t], ref64[:, t], ref32[:, t], None, record_property)
    if layers == 1:
        check(f"{name}/cache_kv", cache[0], kv64, kv32, None, record_property)


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("layers", [1, 4])
def test_adaptor_step_against_float64(cuda, layers, n, record_property):
    """Outputs of positions 0..4 (and, for one layer, the K|V written into the cache) at row counts on both sides of the
    split GEMM's launcher crossovers for N = 768, 1536, 2048 (test_row_counts_straddle_the_gemm_launchers)."""
    _adaptor_case(cuda, record_property, D, layers, n, 5, 8, "split", range(5), f"adaptor_step/L{layers}/n{n}")


def test_adaptor_step_with_the_f32_gemm_against_float64(cuda, monkeypatch, record_property):
    monkeypatch.setattr(ops, "GEMM_MODE", "exact")
    _adaptor_case(cuda, record_property, D, 4, 161, 5, 8, "exact", range(5), "adaptor_step/exact/L4/n161")


@pytest.mark.parametrize("n", [1, 10, 65])
def test_narrow_adaptor_step_against_float64(cuda, n, record_property):
    """d = 256 (8 heads of 32): add_layernorm's LDS path."""
    _adaptor_case(cuda, record_property, 256, 2, n, 5, 8, "split", range(5), f"adaptor_step/d256/L2/n{n}")


@pytest.mark.parametrize("n", [10, 161])
def test_adaptor_step_over_nine_keys_against_float64(cuda, n, record_property):
    """M = 8, K = 4: T = 9 positions, the self-attention of positions 7 and 8 reads 8 and 9 keys."""
    _adaptor_case(cuda, record_property, D, 2, n, 9, 4, "split", (0, 7, 8), f"adaptor_step/T9/L2/n{n}")


def test_control_adaptor_bar_is_not_loose(cuda):
    """(f) A reference whose last LN3 gain is off by 1e-3 (one entry) misses the bar of the HIP result held above."""
    got, _ = adaptor_hip(cuda, D, 1, 10, 5, 8)
    W = perturbed(adaptor_weights(4, 8, D, 1, head=False), "adaptor.layers.0.norm3.weight")
    (ref64, _), (ref32, _) = adaptor_refs(D, 1, 10, 5, 8, W=W, tag="perturbed")
    for t in range(5):
        assert misses(got[:, t], ref64[:, t], ref32[:, t]), t
    (ref64, _), (ref32, _) = adaptor_refs(D, 1, 10, 5, 8)
    assert not any(misses(got[:, t], ref64[:, t], ref32[:, t]) for t in range(5))


# ---- models and table budgets ----------------------------------------------------------------------------------------------
def budgets(M, K, layers, d=D):
    """Byte budgets, from PrefixTables' own arithmetic, that put the tables in each regime."""
    kv = lambda p: K ** p * 2 * d * 4 * layers            # noqa: E731
    tm = lambda p: K ** p * (K + 1) * d * 4                # noqa: E731
    av = lambda p: K ** p * d * 4                          # noqa: E731
    full = lambda P: sum(kv(p) + tm(p) for p in range(P))  # noqa: E731
    return {"head_matrices_everywhere": full(M + 1), "adaptor_vectors_only_at_2": full(2) + kv(2) + av(2),
            "tables_end_before_2": full(2), "final_position_in_chunks": full(M) + av(M), "positions_0_to_2": full(3)}


def assert_regime(tab, regime, M):
    none = [t is None for t in tab.tmat]
    assert [a is None for a in tab.avec] == [not x for x in none]
    if regime == "head_matrices_everywhere":
        assert tab.levels == M + 1 and not any(none)
    elif regime == "adaptor_vectors_only_at_2":
        assert tab.levels == 3 and none == [False, False, True]
    elif regime == "tables_end_before_2":
        assert tab.levels == 2 and none == [False, False]
    elif regime == "final_position_in_chunks":
        assert tab.levels == M + 1 and none == [False] * M + [True]
    elif regime == "positions_0_to_2":
        assert tab.levels == 3 and none == [False, False, False]
    else:
        raise AssertionError(regime)


def build_model(cuda, M, K, table_bytes, layers=2):
    W, cfg = model_weights(M, K, layers)
    return nci.NCIModel(W, device=cuda, prefix_table_bytes=table_bytes, **cfg), W, cfg


# ---- (c): PrefixTables rows -------------------------------------------------------------------------------------------------
TABLE_REGIMES = ["head_matrices_everywhere", "adaptor_vectors_only_at_2", "tables_end_before_2", "final_position_in_chunks"]


@pytest.mark.parametrize("regime", TABLE_REGIMES)
def test_prefix_table_rows_against_float64(cuda, monkeypatch, regime, record_property):
    """M = 3, K = 8 (1, 8, 64, 512 prefixes): every tmat / avec / kv row against the restatement of that prefix."""
    M, K, layers = 3, 8, 2
    monkeypatch.setattr(nci.PrefixTables, "FINAL_CHUNK", 100)       # 512 final prefixes: five chunks of 100 and one of 12
    model, W, cfg = build_model(cuda, M, K, budgets(M, K, layers)[regime], layers)
    tab = model.tables()
    assert_regime(tab, regime, M)
    digits = np.stack(np.meshgrid(*[np.arange(K)] * M, indexing="ij"), -1).reshape(-1, M)     # row j = base-K digits of j
    tok = torch.from_numpy(prefix_tokens(digits, K))

    def run(dt, dev):
        Wd = cast(W, dt, dev)
        out, _, kvs = n64.adaptor(Wd, cfg, Wd["decode_embeddings.weight"][tok.to(dev)])
        tm = [n64.head_matrix(Wd, cfg, out[::K ** (M - p), p], p).reshape(K ** p, -1) for p in range(M + 1)]
        return out, kvs, tm

    (a64, kv64, tm64), (a32, kv32, tm32) = refs(("tables", M, K), run)
    compared = 0
    for p in range(tab.levels):
        step = K ** (M - p)                                   # prefix j of position p = full prefix j * K^(M-p), cut at p
        if tab.tmat[p] is not None:
            assert tab.tmat[p].shape == (K ** p, (K + 1) * D)
            check(f"tables/{regime}/tmat{p}", tab.tmat[p], tm64[p], tm32[p], None, record_property)
        else:
            assert tab.avec[p].shape == (K ** p, D)
            check(f"tables/{regime}/avec{p}", tab.avec[p], a64[::step, p], a32[::step, p], None, record_property)
        compared += 1
        for l in range(layers):
            if p < len(tab.kv[l]):
                assert tab.kv[l][p].shape == (K ** p, 2 * D)
                check(f"tables/{regime}/kv{l}_{p}", tab.kv[l][p], kv64[l][::step, p], kv32[l][::step, p], None, record_property)
                compared += 1
    n_kv = {"final_position_in_chunks": M}.get(regime, tab.levels)     # the chunked final position keeps no K|V
    assert [len(k) for k in tab.kv] == [n_kv] * layers and compared == tab.levels + layers * n_kv


# ---- (d): the head alone ----------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(33, 59), (33, 60), (33, 256), (33, 257), (64, 30), (64, 31), (65, 30), (65, 31), (257, 7), (257, 8)]


def _gains(g, dim):
    w = torch.exp(0.5 * torch.randn(dim, generator=g))
    w[torch.randperm(dim, generator=g)[:4]] = 10 + 20 * torch.rand(4, generator=g)
    return w


def stream_rows(g, m, dim):
    """Final-normed decoder states: rmsnorm of a stream with a few channels 50-100x the rest, times log-normal gains."""
    big = torch.ones(dim)
    big[torch.randperm(dim, generator=g)[:5]] = 50 + 50 * torch.rand(5, generator=g)
    x = torch.randn(m, dim, generator=g) * big
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * _gains(g, dim)


def post_ln_rows(g, m, dim):
    """Adaptor outputs: a LayerNorm's output (gains with entries of 10-30, biases up to O(1))."""
    x = torch.randn(m, dim, generator=g)
    return n64.layernorm(x, _gains(g, dim), 0.3 * torch.randn(dim, generator=g))


def head_weights(ncol, dim=D):
    key = ("hw", ncol, dim)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(ncol)
        w = torch.randn(ncol * dim, dim, generator=g) * dim ** -0.5
        w[torch.randint(0, ncol * dim, (6,), generator=g)] *= 30
        _CACHE[key] = (w, torch.randn(ncol * dim, generator=g))
    return _CACHE[key]


def head_hip(cuda, monkeypatch, ncol, m):
    """ops.head_logits with ops.FUSED_HEAD on and off: computed once."""
    key = ("hip_d", ncol, m)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(100 * ncol + m)
        s, a = stream_rows(g, m, D), post_ln_rows(g, m, D)
        w, e = head_weights(ncol)
        assert ops.GEMM_MODE == "split"
        ws, ed, sd, ad = ops.weight(w.to(cuda)), e.to(cuda), s.to(cuda), a.to(cuda)
        out = {}
        for fused in (True, False):
            monkeypatch.setattr(ops, "FUSED_HEAD", fused)
            out[fused] = ops.head_logits(ad, ws, ed, sd, D ** -0.5, ncol).cpu()
        _CACHE[key] = (s, a, out)
    return _CACHE[key]


def head_refs(ncol, m, s, a, alpha, tag=""):
    w, e = head_weights(ncol)

    def run(dt, dev):
        te = (a.to(dev, dt) @ w.to(dev, dt).T + e.to(dev, dt)).view(m, ncol, D)
        return ((s.to(dev, dt) * alpha)[:, None, :] * te).sum(-1)

    return refs(("head", ncol, m, tag), run)


@pytest.mark.parametrize("ncol,m", HEAD_SHAPES)
def test_head_logits_against_float64(cuda, monkeypatch, ncol, m, record_property):
    """ops.head_logits fused (GEMM with the logits epilogue + finish) and unfused (GEMM + rows kernel) on both sides of the
    fused path's m n > 1.5 M, at the 64-column chunk edge and the 256-row tile edge."""
    fusable = bool(hip.lib().mevi_gemm_nt_split_head_supported(m, ncol * D, D, D))
    assert fusable == (m * ncol * D > SKINNY_MAX)
    s, a, out = head_hip(cuda, monkeypatch, ncol, m)
    ref64, ref32 = head_refs(ncol, m, s, a, D ** -0.5)
    check(f"head/ncol{ncol}/m{m}/{'fused' if fusable else 'latency_gemm'}", out[True], ref64, ref32, None, record_property)
    check(f"head/ncol{ncol}/m{m}/two_kernels", out[False], ref64, ref32, None, record_property)


def test_control_head_bar_is_not_loose(cuda, monkeypatch):
    """(f) A reference with alpha off by 1e-3 misses the bar."""
    ncol, m = 33, 60
    s, a, out = head_hip(cuda, monkeypatch, ncol, m)
    ref64, ref32 = head_refs(ncol, m, s, a, D ** -0.5 * 1.001, tag="alpha")
    assert misses(out[True], ref64, ref32) and misses(out[False], ref64, ref32)
    ref64, ref32 = head_refs(ncol, m, s, a, D ** -0.5)
    assert not misses(out[True], ref64, ref32) and not misses(out[False], ref64, ref32)


@pytest.mark.parametrize("ncol,m", [(33, 60), (33, 257), (64, 31), (65, 31), (257, 8)])
@pytest.mark.parametrize("dim", [768, 256, 1000])
def test_logits_over_a_table_against_float64(cuda, dim, ncol, m, record_property):
    """adaptive_logits_rows with t_index into a 9-row table (the 768 kernel; at dim 256 and 1000 the generic kernel<NI>), and
    the column form scale + adaptive_logits with lm_head's rows apart."""
    g = torch.Generator().manual_seed(dim + 7 * ncol + m)
    s = stream_rows(g, m, dim)
    t9 = torch.randn(9, ncol, dim, generator=g) * _gains(g, dim)          # adaptor_linear(a): a carries the LN's gains
    e = torch.randn(ncol, dim, generator=g)
    te9 = t9 + e                                                         # f32: the rows form's input
    idx = torch.randint(0, 9, (m,), generator=g)
    idx[0], idx[-1] = 8, 0
    alpha = dim ** -0.5
    sd, idxd = s.to(cuda), idx.to(cuda)
    rows = ops.adaptive_logits_rows(sd, alpha, te9.view(9, -1).to(cuda), ncol, t_index=idxd)
    cols = ops.adaptive_logits(ops.scale(sd, alpha), t9.view(9, -1).to(cuda), e.to(cuda), t_index=idxd)

    def run_rows(dt, dev):
        return ((s.to(dev, dt) * alpha)[:, None, :] * te9.to(dev, dt)[idx.to(dev)]).sum(-1)

    def run_cols(dt, dev):
        return ((s.to(dev, dt) * alpha)[:, None, :] * (t9.to(dev, dt)[idx.to(dev)] + e.to(dev, dt))).sum(-1)

    ref64, ref32 = refs(("table_rows", dim, ncol, m), run_rows)
    check(f"head_table/rows/dim{dim}/ncol{ncol}/m{m}", rows, ref64, ref32, None, record_property)
    ref64, ref32 = refs(("table_cols", dim, ncol, m), run_cols)
    check(f"head_table/columns/dim{dim}/ncol{ncol}/m{m}", cols, ref64, ref32, None, record_property)


# ---- (e): whole decode positions through the real search -------------------------------------------------------------------
SEARCHES = {
    # name: (M, K, budget name or byte count, module switch or None)
    "3x8/head_matrices_everywhere": (3, 8, "head_matrices_everywhere", None),
    "3x8/adaptor_vectors_only_at_2": (3, 8, "adaptor_vectors_only_at_2", None),
    "3x8/tables_end_before_2": (3, 8, "tables_end_before_2", None),
    "3x8/final_position_in_chunks": (3, 8, "final_position_in_chunks", None),
    "3x8/no_tables": (3, 8, 0, None),
    "4x32/positions_0_to_2": (4, 32, "positions_0_to_2", None),
    "8x4/no_tables": (8, 4, 0, None),
    "3x8/column_logits": (3, 8, "adaptor_vectors_only_at_2", "ROW_LOGITS"),
    "3x8/copied_adaptor_cache": (3, 8, "final_position_in_chunks", "INDEXED_ADAPTOR_CACHE"),
}
BEAMS, QUERY_LENGTHS, QUERY_S = 10, [24, 5, 17, 9], 24


def search_hip(cuda, monkeypatch, name):
    """generate() of 4 ragged queries with model._logits wrapped: [(p, pidx, tokens, logits)] per position, computed once.
    pidx is _search's own running prefix index (a local there: it is maintained in every regime, also beyond the tables)."""
    key = ("hip_e", name)
    if key in _CACHE:
        return _CACHE[key]
    M, K, budget, switch = SEARCHES[name]
    layers = 2
    table_bytes = budget if isinstance(budget, int) else budgets(M, K, layers)[budget]
    monkeypatch.setattr(nci.PrefixTables, "FINAL_CHUNK", 100)
    if switch is not None:
        monkeypatch.setattr(nci, switch, False)
    model, W, cfg = build_model(cuda, M, K, table_bytes, layers)
    rec = []
    inner = model._logits

    def logits(tokens, p, *args, **kw):
        frame = sys._getframe(1)
        assert frame.f_code.co_name == "_search"
        out = inner(tokens, p, *args, **kw)
        rec.append((p, frame.f_locals["pidx"].cpu().clone(), tokens.cpu().clone(), out.cpu().clone()))
        return out

    model._logits = logits
    ids, mask = t5f.batch(QUERY_LENGTHS, QUERY_S, seed=4)
    model.generate(ids, mask, num_beams=BEAMS)
    if table_bytes:
        tab = model.tables()
        if switch == "INDEXED_ADAPTOR_CACHE":                  # no chunked final position without the indexed cache
            assert tab.levels == M and all(t is not None for t in tab.tmat)
        else:
            assert_regime(tab, budget, M)
    else:
        assert model._tables is None
    _CACHE[key] = (rec, W, cfg, ids, mask)
    return _CACHE[key]


def search_refs(W, cfg, ids, mask, p, pidx, tag=""):
    """position_logits of the rows whose prefixes are the base-K digits of pidx (row r: query r // beams alive)."""
    K, B = cfg["K"], ids.shape[0]
    n = pidx.numel()
    assert n % B == 0
    query = torch.arange(n) // (n // B)
    digits = np.stack([pidx.numpy()] + [(pidx.numpy() // K ** (p - i)) % K for i in range(1, p + 1)], 1)[:, 1:]
    tok = torch.from_numpy(prefix_tokens(digits, K))

    def enc(dt, dev):
        Wd = cast(W, dt, dev)
        return r64.encoder(Wd, cfg, Wd["shared.weight"][ids.to(dev)], mask.to(dev))

    def run(dt, dev):
        e = refs(("e_enc", id(W), tag), enc)[0 if dt == torch.float64 else 1]
        return n64.position_logits(cast(W, dt, dev), cfg, tok.to(dev), e[query.to(dev)], mask[query].to(dev))

    return tok, refs(("e", id(W), tag, p, tuple(pidx.tolist())), run)


@pytest.mark.parametrize("name", list(SEARCHES))
def test_every_decode_position_of_generate_against_float64(cuda, monkeypatch, name, record_property):
    """Each position's [rows, K + 1] logits, as the beam step receives them, against the reference's logits of the same
    (query, prefix) rows -- under every table regime, without tables (per-beam adaptor, R > K at position 1), with ids of 8
    codes (copied decoder caches), with the column form of the head and with the gathered adaptor cache."""
    rec, W, cfg, ids, mask = search_hip(cuda, monkeypatch, name)
    M, K, B = cfg["M"], cfg["K"], ids.shape[0]
    assert [r[0] for r in rec] == list(range(M + 1))
    live, rows = 1, 0
    for p, pidx, tokens, got in rec:
        assert pidx.numel() == B * live and got.shape == (B * live, K + 1)
        tok, (ref64, ref32) = search_refs(W, cfg, ids, mask, p, pidx)
        assert torch.equal(tok[:, -1], tokens)                   # the row's own token is its prefix's last code
        check(f"search/{name}/p{p}", got, ref64, ref32, None, record_property)
        rows += got.shape[0]
        live = min(BEAMS, live * K)
    assert rows == sum(B * min(BEAMS, K ** p) for p in range(M + 1))


def test_control_search_bar_is_not_loose(cuda, monkeypatch):
    """(f) A reference whose decoder final_layer_norm gain is off by 1e-3 (one entry) misses every position's bar."""
    rec, W, cfg, ids, mask = search_hip(cuda, monkeypatch, "3x8/no_tables")
    Wp = perturbed(W, "decoder.final_layer_norm.weight")
    for p, pidx, _, got in rec:
        _, (ref64, ref32) = search_refs(Wp, cfg, ids, mask, p, pidx, tag="perturbed")
        assert misses(got, ref64, ref32), p
        _, (ref64, ref32) = search_refs(W, cfg, ids, mask, p, pidx)
        assert not misses(got, ref64, ref32), p
