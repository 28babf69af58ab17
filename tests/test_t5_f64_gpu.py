"""The T5 blocks of mevi_amd/t5.py at t5-base width (d 768, ff 3072, 12 x 64 heads) against the float64 restatement
(tests/t5_ref64.py) applied to the same f32 inputs -- both norm paths (default, and ops.FOLD_NORM: the T5LayerNorms folded
into the projections), every attention regime the stacks dispatch to, 1 .. 20 000 tokens, the decoder's tower step, cached
steps and cross-attention, and a 12-layer stack.

Bars.  Per block, with e_hip = max |hip - ref64| and e_32 = max |ref32 - ref64| over the real positions (ref32 = the same
restatement in float32 on the host):

    e_hip <= 4 e_32 + 2^-22 max |ref64|.

Why this size.  The component contracts the suite already holds (tests/test_gemm_split_gpu.py, tests/test_t5_gpu.py) are:
a split GEMM is within 2e-6 sum_k |a_k w_k| of float64 and measures ~1.5e-7 of it, the f32 chain's own typical error at
K = 768 .. 3072; an operand image keeps 22 bits, i.e. it is within 2^-21 of the binade of its exponent's bound, and the
bound sits above the row's max (the attention contexts' ctx_bound, the stream's carried bound); softmax and norms are f32
operations with a few ulps each.  Every one of these is an f32 rounding of the kind the host's f32 run makes, of the same
size up to a small factor -- hence 4 e_32 -- except the image's absolute floor, which sits at 2^-22 of the bound's binade
rather than of each value, and feeds through norms that rescale the row to O(max |ref64|) -- hence the 2^-22 max |ref64|
term.  A block that loses 2 bits or more against f32 fails the bar; a 1 % error (a wrong norm width, a missed block of
the sums of squares) fails it by four orders of magnitude, a non-finite value fails it outright.  Both numbers are
recorded with record_property (junit `e_hip`, `e_32`, `bar`).

Weights have the statistics of real T5 checkpoints that the seeded initialiser lacks: log-normal layer-norm weights with a
few entries of 10-30, a handful of residual channels 50-100x the rest (in the embeddings and in the rows of the
projections that write the stream), embeddings of scale 5-20, and one all-zero embedding row (its rmsnorm is 0: the eps
and the exponent clamps).  Token id ZERO_ID is used in every batch."""
import numpy as np
import pytest
import torch

import t5_ref64 as r64
from f64_bar import check, refs      # the bar above and the (ref64, ref32) cache, shared with tests/test_bert_f64_gpu.py
from mevi_amd import ops, t5

pytestmark = pytest.mark.gpu
D, FF, H, DKV = 768, 3072, 12, 64
VOCAB, ZERO_ID = 600, 3
OUTLIERS = (5, 111, 400, 401, 700)
CFG = dict(d_model=D, d_ff=FF, num_heads=H, d_kv=DKV, num_layers=12, num_decoder_layers=12, layer_norm_epsilon=1e-6,
           relative_attention_num_buckets=32)
_CACHE = {}


def realistic_weights(n_enc=12, n_dec=12, seed=0):
    """state_dict-named weights (CPU f32) with the statistics named in the module docstring."""
    key = ("w", n_enc, n_dec, seed)
    if key in _CACHE:
        return _CACHE[key]
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    inner = H * DKV
    big = torch.ones(D)
    big[list(OUTLIERS)] = 50 + 50 * torch.rand(len(OUTLIERS), generator=g)

    def ln():
        w = torch.exp(0.5 * rn(D))
        w[torch.randperm(D, generator=g)[:4]] = 10 + 20 * torch.rand(4, generator=g)
        return w

    emb = rn(VOCAB, D) * (5 + 15 * torch.rand(VOCAB, 1, generator=g)) * big
    emb[ZERO_ID] = 0
    W = {"shared.weight": emb}
    for st, n, dec in (("encoder", n_enc, False), ("decoder", n_dec, True)):
        for l in range(n):
            p = f"{st}.block.{l}.layer"
            atts = ("0.SelfAttention", "1.EncDecAttention") if dec else ("0.SelfAttention",)
            for i, a in enumerate(atts):
                W[f"{p}.{a}.q.weight"] = rn(inner, D) * (D * DKV) ** -0.5
                W[f"{p}.{a}.k.weight"] = rn(inner, D) * D ** -0.5
                W[f"{p}.{a}.v.weight"] = rn(inner, D) * D ** -0.5
                W[f"{p}.{a}.o.weight"] = rn(D, inner) * inner ** -0.5 * big[:, None]
                W[f"{p}.{i}.layer_norm.weight"] = ln()
            f = len(atts)
            W[f"{p}.{f}.DenseReluDense.wi.weight"] = rn(FF, D) * D ** -0.5
            W[f"{p}.{f}.DenseReluDense.wo.weight"] = rn(D, FF) * FF ** -0.5 * big[:, None]
            W[f"{p}.{f}.layer_norm.weight"] = ln()
        W[f"{st}.block.0.layer.0.SelfAttention.relative_attention_bias.weight"] = rn(32, H) * 2
        W[f"{st}.final_layer_norm.weight"] = ln()
    _CACHE[key] = W
    return W


def dims(n_enc, n_dec):
    return t5.T5Dims(**dict(CFG, num_layers=n_enc, num_decoder_layers=n_dec))


def cfg(n_enc, n_dec):
    return dict(CFG, num_layers=n_enc, num_decoder_layers=n_dec)


def batch(lengths, S, seed, holes=False):
    """ids i64 [B, S] (ZERO_ID in every batch), right-padded mask (or one with holes)."""
    rng = np.random.default_rng(seed)
    B = len(lengths)
    ids = rng.integers(0, VOCAB, (B, S))
    mask = np.zeros((B, S), np.int64)
    for i, L in enumerate(lengths):
        mask[i, :L] = 1
    ids[0, min(1, lengths[0] - 1)] = ZERO_ID
    if holes:
        mask[:, 1] = 0
        mask[0, 2] = 0
    return torch.from_numpy(ids), torch.from_numpy(mask)


@pytest.fixture(params=[False, True], ids=["default", "folded"])
def fold(request, monkeypatch):
    """ops.FOLD_NORM (MEVI_FOLD_NORM=1) for the stacks built in the test (fold_norm_ok is read in their __init__).  At this
    width the folded blocks miss the bar (test_folded_blocks_at_t5_base_width_are_refused), so fold_norm_ok refuses them and
    the stacks keep the default path: the tests below hold it to the same bars either way.  Returns whether they fold."""
    monkeypatch.setattr(ops, "FOLD_NORM", request.param)
    folds = ops.fold_norm_ok(D)
    assert folds == (request.param and D <= ops.FOLD_NORM_MAX_WIDTH)
    return folds


ENC_REGIMES = {
    # name: (lengths, S, pack, expected path); lengths keep the real tokens under 0.9 B S where packing is meant
    "padded": ([32, 5, 17, 32, 9, 30], 32, False, "padded"),
    "latency_6_tokens": ([6], 8, True, "mfma16"),
    "packed_le32_300_tokens": ([3 + (7 * i) % 30 for i in range(22)], 32, True, "mfma16"),
    "packed_33_64": ([33 + (11 * i) % 27 for i in range(8)], 64, True, "varlen_short"),
    "passages_65_128": ([65 + (13 * i) % 50 for i in range(6)], 128, True, "h16"),
    "holes": ([32, 20, 31, 12, 28, 30], 32, True, "scatter"),
    "tokens_20k": ([90 + (7 * i) % 36 for i in range(168)], 128, True, "h16"),
}


def _path(mask, pack):
    m = mask.bool()
    if not pack or m.sum() > 0.9 * m.numel():
        return "padded"
    seq_off, longest = t5.packed_offsets(mask)
    if seq_off is None:
        return "scatter"
    assert t5.varlen_ok(longest, DKV)
    return "mfma16" if longest <= 32 else ("varlen_short" if longest <= 64 else "h16")


@pytest.mark.parametrize("regime", list(ENC_REGIMES))
def test_encoder_layer_against_float64(cuda, fold, regime, record_property):
    """One encoder block + the final norm (EncoderStack with one layer) in each attention regime, packed and padded, 6 to
    ~18 000 real tokens (the latency GEMM kernels, the tile stream at several tile heights and its remainder launch)."""
    lengths, S, pack, path = ENC_REGIMES[regime]
    holes = regime == "holes"
    ids, mask = batch(lengths, S, seed=len(lengths) + S, holes=holes)
    assert _path(mask, pack) == path
    W = realistic_weights()
    enc = t5.EncoderStack(W, dims(1, 0), cuda)
    assert enc.fold == fold
    got = enc.forward(W["shared.weight"].to(cuda), ids.to(cuda), mask.to(cuda), pack=pack)

    def run(dt, dev):
        Wd = r64.cast(W, dt, dev)
        return r64.encoder(Wd, cfg(1, 0), Wd["shared.weight"][ids.to(dev)], mask.to(dev), n_layers=1)

    ref64, ref32 = refs(("enc1", regime), run)
    check(f"encoder_layer/{regime}/{'folded' if fold else 'default'}", got, ref64, ref32, mask.bool(), record_property)


def _enc_states(B, S, seed):
    """Final-normed encoder-like states of B queries (the f32 rows the decoder reads) and their mask."""
    lengths = [4 + (5 * i + seed) % (S - 4) for i in range(B)]
    ids, mask = batch(lengths, S, seed)
    W = realistic_weights()
    key = ("encstates", B, S, seed)
    if key not in _CACHE:
        Wd = r64.cast(W, torch.float64, "cuda")
        _CACHE[key] = r64.encoder(Wd, cfg(1, 0), Wd["shared.weight"][ids.to("cuda")], mask.to("cuda"), n_layers=1).float()
    return _CACHE[key], mask


@pytest.mark.parametrize("wov", [True, False], ids=["wov", "two_gemms"])
@pytest.mark.parametrize("enc_norm", [True, False], ids=["enc_norm", "no_enc_norm"])
@pytest.mark.parametrize("pack", [True, False], ids=["packed_kv", "padded_kv"])
def test_tower_step_against_float64(cuda, fold, monkeypatch, wov, enc_norm, pack, record_property):
    """The towers' one-position decoder (DecoderStack(max_len=1).step at t = 0, one layer + final norm) on 32 queries:
    MEVI_TOWER_WOV on (o(v(.)) as one pre-multiplied weight) and off, cross-attention contexts as the o-projection's image
    (set_encoder_norm) or f32, over packed K|V (kv_off) and padded K|V with the mask."""
    monkeypatch.setattr(t5, "WOV_FUSE", wov)
    W = realistic_weights()
    enc, mask = _enc_states(32, 32, seed=1)
    dec = t5.DecoderStack(W, dims(0, 1), cuda, n_layers=1, max_len=1)
    assert dec.fold == fold and ("wov" in dec.layers[0]) == wov
    if enc_norm:
        dec.set_encoder_norm(ops.norm_out_bound(W["encoder.final_layer_norm.weight"].to(cuda), D))
        assert dec.layers[0]["xvb"] is not None
    xkv = dec.cross_kv(enc, mask.to(cuda), pack=pack)
    assert (xkv.kv_off is not None) == pack
    x0 = W["shared.weight"][torch.zeros(32, dtype=torch.long)].to(cuda)
    got = dec.step(x0, 0, dec.new_cache(32), xkv, mask.to(cuda), 1)

    def run(dt, dev):
        Wd = r64.cast(W, dt, dev)
        return r64.tower_step(Wd, cfg(0, 1), Wd["shared.weight"][torch.zeros(32, dtype=torch.long, device=dev)],
                              enc.to(dev, dt), mask.to(dev), n_layers=1)

    ref64, ref32 = refs(("tower1",), run)
    name = f"tower_step/{'wov' if wov else 'two_gemms'}/{'enc_norm' if enc_norm else 'no_enc_norm'}/" \
           f"{'packed' if pack else 'padded'}/{'folded' if fold else 'default'}"
    check(name, got, ref64, ref32, None, record_property)


def test_cached_decoder_steps_against_float64(cuda, fold, record_property):
    """NCI-style steps t = 0..3 of a one-layer decoder on 8 queries x 10 beams: cross-attention with kv_div = 10 over
    packed K|V with the encoder norm set; the caches are not re-ordered, key_rows names every position's ancestor row
    (attention_cached).  Each step against the full-prefix float64 decoder over the row's ancestor tokens."""
    B, R, T = 8, 10, 4
    n = B * R
    W = realistic_weights()
    enc, mask = _enc_states(B, 40, seed=2)
    dec = t5.DecoderStack(W, dims(0, 1), cuda, n_layers=1, max_len=T)
    assert dec.fold == fold
    dec.set_encoder_norm(ops.norm_out_bound(W["encoder.final_layer_norm.weight"].to(cuda), D))
    xkv = dec.cross_kv(enc, mask.to(cuda), pack=True)
    assert xkv.kv_off is not None
    rng = np.random.default_rng(5)
    tok = rng.integers(0, VOCAB, (T, n))
    tok[0] = 0
    tok[2, 3] = ZERO_ID
    par = [np.arange(n)] + [(np.arange(n) // R) * R + rng.integers(0, R, n) for _ in range(1, T)]
    anc = np.zeros((T, n, T), np.int64)       # anc[t, r, j]: the cache row holding position j of row r's prefix at step t
    for t in range(T):
        anc[t, :, t] = np.arange(n)
        for j in range(t - 1, -1, -1):
            anc[t, :, j] = par[j + 1][anc[t, :, j + 1]]
    cache = dec.new_cache(n)
    emb = W["shared.weight"]
    for t in range(T):
        kr = torch.from_numpy(anc[t, :, :t + 1].astype(np.int32)).to(cuda)
        got = dec.step(emb[torch.from_numpy(tok[t, :])].to(cuda), t, cache, xkv, None, R, key_rows=kr)
        prefix_tok = torch.from_numpy(np.stack([tok[j, anc[t, :, j]] for j in range(t + 1)], 1))   # [n, t + 1]

        def run(dt, dev, prefix_tok=prefix_tok):
            Wd = r64.cast(W, dt, dev)
            e = enc.to(dev, dt).repeat_interleave(R, 0)
            m = mask.to(dev).repeat_interleave(R, 0)
            return r64.decoder(Wd, cfg(0, 1), Wd["shared.weight"][prefix_tok.to(dev)], e, m, n_layers=1)[:, -1]

        ref64, ref32 = refs(("cached", t), run)
        check(f"cached_step_t{t}/{'folded' if fold else 'default'}", got, ref64, ref32, None, record_property)


def test_cross_attention_over_padded_kv_with_kv_div(cuda, fold, record_property):
    """kv_div = 10 over PADDED K|V with the key mask (cross_kv(pack=False)), encoder norm unset (f32 contexts), position 0 of
    a max_len-4 decoder (the cache path of t = 0, not the tower's wov)."""
    B, R = 6, 10
    W = realistic_weights()
    enc, mask = _enc_states(B, 32, seed=3)
    dec = t5.DecoderStack(W, dims(0, 1), cuda, n_layers=1, max_len=4)
    xkv = dec.cross_kv(enc, mask.to(cuda), pack=False)
    assert xkv.kv_off is None and xkv.mask is not None and dec.layers[0]["xvb"] is None
    tok = torch.from_numpy(np.random.default_rng(9).integers(0, VOCAB, B * R))
    tok[7] = ZERO_ID
    got = dec.step(W["shared.weight"][tok].to(cuda), 0, dec.new_cache(B * R), xkv, mask.to(cuda), R)

    def run(dt, dev):
        Wd = r64.cast(W, dt, dev)
        return r64.tower_step(Wd, cfg(0, 1), Wd["shared.weight"][tok.to(dev)], enc.to(dev, dt).repeat_interleave(R, 0),
                              mask.to(dev).repeat_interleave(R, 0), n_layers=1)

    ref64, ref32 = refs(("xpad",), run)
    check(f"cross_padded_kvdiv10/{'folded' if fold else 'default'}", got, ref64, ref32, None, record_property)


def test_twelve_layer_encoder_and_tower_step_against_float64(cuda, fold, record_property):
    """Depth: encoder stacks of 1, 3, 6 and 12 layers on 32 queries (packed, mfma16), and the 12-layer tower step on the
    12-layer encoder's output.  The bar is the per-block rule at each depth: e_32 is the f32 run of the same depth, so the
    bar grows with depth the way f32 rounding does.  The per-depth errors are recorded (error growth)."""
    lengths = [3 + (7 * i) % 30 for i in range(32)]
    ids, mask = batch(lengths, 32, seed=12)
    W = realistic_weights()

    def run(dt, dev):
        Wd = r64.cast(W, dt, dev)
        out, hs = r64.encoder(Wd, cfg(12, 12), Wd["shared.weight"][ids.to(dev)], mask.to(dev), return_all=True)
        per = {n: r64.final_norm(Wd, cfg(12, 12), hs[n], "encoder") for n in (1, 3, 6)}
        per[12] = out
        x0 = Wd["shared.weight"][torch.zeros(32, dtype=torch.long, device=dev)]
        per["tower"] = r64.tower_step(Wd, cfg(12, 12), x0, out, mask.to(dev))
        return per

    ref64, ref32 = refs(("deep",), run)
    tag = "folded" if fold else "default"
    for n in (1, 3, 6, 12):
        enc = t5.EncoderStack(W, dims(n, 0), cuda)
        assert enc.fold == fold
        got = enc.forward(W["shared.weight"].to(cuda), ids.to(cuda), mask.to(cuda))
        check(f"encoder_depth_{n}/{tag}", got, ref64[n], ref32[n], mask.bool(), record_property)
    tower = t5.TwinTower(W, dims=dims(12, 12), device=cuda)
    assert tower.encoder.fold == fold and tower.decoder.fold == fold
    got = tower.encode_query({"input_ids": ids, "attention_mask": mask})
    check(f"tower_depth_12/{tag}", got, ref64["tower"], ref32["tower"], None, record_property)


def test_folded_blocks_at_t5_base_width_are_refused(cuda, monkeypatch, record_property):
    """Why ops.FOLD_NORM_MAX_WIDTH stops below 768: with the width limit lifted, the folded encoder block of the padded regime
    misses the bar on the row of the all-zero embedding (measured 9.2e-5 against a bar of 8.7e-5; the default path 4.2e-5): the
    stream's image exponent comes from a bound that sits up to 11.8 binades above that row after the attention sub-layer.  The
    folded blocks' errors in every encoder regime and the tower step are recorded here; they must stay finite and within 2^-14 of
    max |ref64| (gross errors: a wrong norm width or block count, a context bound that overflows the image).  Raising the limit
    makes the `folded` variants of the tests above run this path under their full bars."""
    monkeypatch.setattr(ops, "FOLD_NORM", True)
    assert not ops.fold_norm_ok(D)
    monkeypatch.setattr(ops, "FOLD_NORM_MAX_WIDTH", 1024)
    assert ops.fold_norm_ok(D)
    W = realistic_weights()
    worst = {}
    for regime, (lengths, S, pack, path) in ENC_REGIMES.items():
        ids, mask = batch(lengths, S, seed=len(lengths) + S, holes=regime == "holes")
        enc = t5.EncoderStack(W, dims(1, 0), cuda)
        assert enc.fold
        got = enc.forward(W["shared.weight"].to(cuda), ids.to(cuda), mask.to(cuda), pack=pack)

        def run(dt, dev, ids=ids, mask=mask):
            Wd = r64.cast(W, dt, dev)
            return r64.encoder(Wd, cfg(1, 0), Wd["shared.weight"][ids.to(dev)], mask.to(dev), n_layers=1)

        ref64, ref32 = refs(("enc1", regime), run)
        worst[regime] = check(f"forced_fold/encoder_layer/{regime}", got, ref64, ref32, mask.bool(), record_property,
                              factor=float("inf"))
        assert worst[regime][0] <= 2.0 ** -14 * ref64.abs().max().item(), (regime, worst[regime])
    enc_states, mask = _enc_states(32, 32, seed=1)
    dec = t5.DecoderStack(W, dims(0, 1), cuda, n_layers=1, max_len=1)
    assert dec.fold
    dec.set_encoder_norm(ops.norm_out_bound(W["encoder.final_layer_norm.weight"].to(cuda), D))
    x0 = W["shared.weight"][torch.zeros(32, dtype=torch.long)].to(cuda)
    got = dec.step(x0, 0, dec.new_cache(32), dec.cross_kv(enc_states, mask.to(cuda)), mask.to(cuda), 1)

    def run(dt, dev):
        Wd = r64.cast(W, dt, dev)
        return r64.tower_step(Wd, cfg(0, 1), Wd["shared.weight"][torch.zeros(32, dtype=torch.long, device=dev)],
                              enc_states.to(dev, dt), mask.to(dev), n_layers=1)

    ref64, ref32 = refs(("tower1",), run)
    e = check("forced_fold/tower_step", got, ref64, ref32, None, record_property, factor=float("inf"))
    assert e[0] <= 2.0 ** -14 * ref64.abs().max().item()
