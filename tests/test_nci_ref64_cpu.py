"""tests/nci_ref64.py (the dtype-parametrised restatement of the adaptor and the PAWA head that the float64 GPU tests are
held to) pinned to the f32 oracle on the G1 goldens' weights: in float32 it reproduces oracle.t5.adaptor and
oracle.t5.nci_last_logits at the valid columns within the goldens' 5e-5, for random prefixes at every position; in float64
it agrees with its own float32 run to f32 rounding; and its one-key cross-attention is the constant nci.Adaptor uses."""
import json
import os

import numpy as np
import pytest
import torch

import nci_ref64 as n64
import t5_ref64 as r64
from oracle import t5 as ot5

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 5e-5
NAMES = ["g1_nci_M4_K32_R10", "g1_nci_M3_K256_R10", "g1_nci_M2_K4_R10"]


def _load(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    cfg = json.loads(str(g["cfg"]))
    return cfg, ot5.load_weights(g), torch.from_numpy(g["input_ids"]), torch.from_numpy(g["attention_mask"])


def _prefixes(cfg, p, n, seed):
    """n random prefixes of position p: token 0, then 2 + jK + code for j < p."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, cfg["K"], (n, p))
    tok = np.concatenate([np.zeros((n, 1), np.int64), 2 + np.arange(p)[None, :] * cfg["K"] + codes], 1)
    return torch.from_numpy(tok)


@pytest.mark.parametrize("name", NAMES)
def test_float32_restatement_reproduces_the_oracle(name):
    cfg, W, ids, mask = _load(name)
    W32 = r64.cast(W, torch.float32)
    enc = ot5.encoder(W, cfg, ids, mask)
    for p in range(cfg["M"] + 1):
        tok = _prefixes(cfg, p, 6, seed=p)
        q = torch.arange(6) % ids.shape[0]
        emb = W32["decode_embeddings.weight"][tok]
        out, hs, kvs = n64.adaptor(W32, cfg, emb)
        assert len(hs) == cfg["adaptor_layer_num"] + 1 and len(kvs) == cfg["adaptor_layer_num"]
        assert (out - ot5.adaptor(W, cfg, emb)).abs().max() <= TOL
        for l in range(1, len(hs)):              # the per-layer states are the shallower adaptors' outputs
            assert (hs[l] - ot5.adaptor(W, dict(cfg, adaptor_layer_num=l), emb)).abs().max() <= TOL
        got = n64.position_logits(W32, cfg, tok, enc[q], mask[q])
        want = ot5.nci_last_logits(W, cfg, tok, enc[q], mask[q])[:, n64.valid_columns(cfg, p)]
        assert got.shape == (6, cfg["K"] + 1)
        assert (got - want).abs().max() <= TOL, (name, p)
        # the K|V the cache holds are the in_proj rows of each layer's input
        d = cfg["d_model"]
        w, b = W32["adaptor.layers.0.self_attn.in_proj_weight"], W32["adaptor.layers.0.self_attn.in_proj_bias"]
        assert torch.equal(kvs[0], emb @ w[d:].T + b[d:])


@pytest.mark.parametrize("name", NAMES)
def test_float64_restatement_agrees_with_float32_to_its_rounding(name):
    """The rule of tests/test_t5_ref64_cpu.py: within 2e-5 of max |ref64|, and not identical."""
    cfg, W, ids, mask = _load(name)
    W32, W64 = r64.cast(W, torch.float32), r64.cast(W, torch.float64)
    e32 = r64.encoder(W32, cfg, W32["shared.weight"][ids], mask)
    e64 = r64.encoder(W64, cfg, W64["shared.weight"][ids], mask)
    for p in range(cfg["M"] + 1):
        tok = _prefixes(cfg, p, 6, seed=10 + p)
        q = torch.arange(6) % ids.shape[0]
        a32 = n64.adaptor(W32, cfg, W32["decode_embeddings.weight"][tok])
        a64 = n64.adaptor(W64, cfg, W64["decode_embeddings.weight"][tok])
        assert a64[0].dtype == torch.float64 and a32[0].dtype == torch.float32
        for x32, x64 in zip([a32[0]] + a32[1][1:] + a32[2], [a64[0]] + a64[1][1:] + a64[2]):
            diff = (x32.double() - x64).abs().max()
            assert 0 < diff <= 2e-5 * x64.abs().max()
        l32 = n64.position_logits(W32, cfg, tok, e32[q], mask[q])
        l64 = n64.position_logits(W64, cfg, tok, e64[q], mask[q])
        assert l64.dtype == torch.float64
        diff = (l32.double() - l64).abs().max()
        assert 0 < diff <= 2e-5 * l64.abs().max(), (name, p)
        h32 = n64.head_matrix(W32, cfg, a32[0][:, -1], p)
        h64 = n64.head_matrix(W64, cfg, a64[0][:, -1], p)
        assert h64.shape == (6, cfg["K"] + 1, cfg["d_model"])
        assert 0 < (h32.double() - h64).abs().max() <= 2e-5 * h64.abs().max()


@pytest.mark.parametrize("name", NAMES)
def test_one_key_cross_attention_is_a_constant(name):
    """nci.Adaptor replaces each layer's cross-attention by out_proj(v_proj(memory)): softmax over one key is 1."""
    cfg, W, _, _ = _load(name)
    W64 = r64.cast(W, torch.float64)
    d = cfg["d_model"]
    x = torch.randn(5, 3, d, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) * 3
    mem = W64["adaptor_embeddings"].reshape(1, 1, d)
    for l in range(cfg["adaptor_layer_num"]):
        pre = f"adaptor.layers.{l}.multihead_attn"
        full = n64.mha(W64, pre, x, mem.expand(5, 1, d))[0]
        const = n64.cross_const(W64, pre, mem.reshape(1, d))
        assert (full - const).abs().max() <= 1e-12 * const.abs().max()


def test_the_float64_bar_catches_the_mutations_it_is_meant_for(monkeypatch):
    """The float32 restatement stands in for the HIP adaptor at base width (weights, tokens and bar of
    tests/test_nci_f64_gpu.py, one layer, 10 rows), with one fault at a time: q not scaled by (d/8)^-0.5, the cross-attention
    constant dropped, no value bias, unbiased variance.  Each must miss the bar of some position by more than the
    bar itself, so that a kernel within the bar of float64 apart from the fault still fails its GPU test."""
    import test_nci_f64_gpu as T

    d, n, steps, K = T.D, 10, 5, 8
    W = T.adaptor_weights(steps - 1, K, d, 1, head=False)
    tok = T.teacher_tokens(n, steps, K, seed=n)
    cfg = dict(d_model=d, adaptor_layer_num=1)

    def run(Wd):
        return n64.adaptor(Wd, cfg, Wd["decode_embeddings.weight"][tok])[0].double()

    ref64, ref32 = run(r64.cast(W, torch.float64)), run(W)
    err = lambda x: (x - ref64).abs().amax((0, 2))                                   # noqa: E731  per position
    bars = 4.0 * err(ref32) + 2.0 ** -22 * ref64.abs().amax((0, 2))
    assert (err(ref32) <= bars).all()

    def caught(Wm):
        return bool((err(run(Wm)) > 2 * bars).any())

    p = "adaptor.layers.0."
    s = (d // n64.NHEAD) ** 0.5                      # q k^T without the scale: the query projection times sqrt(96)
    scale1 = dict(W)
    scale1[p + "self_attn.in_proj_weight"], scale1[p + "self_attn.in_proj_bias"] = \
        W[p + "self_attn.in_proj_weight"].clone(), W[p + "self_attn.in_proj_bias"].clone()
    scale1[p + "self_attn.in_proj_weight"][:d] *= s
    scale1[p + "self_attn.in_proj_bias"][:d] *= s
    assert caught(scale1)
    no_cross = dict(W)
    no_cross[p + "multihead_attn.out_proj.weight"] = torch.zeros(d, d)
    no_cross[p + "multihead_attn.out_proj.bias"] = torch.zeros(d)
    assert caught(no_cross)
    no_vbias = dict(W)
    no_vbias[p + "self_attn.in_proj_bias"] = W[p + "self_attn.in_proj_bias"].clone()
    no_vbias[p + "self_attn.in_proj_bias"][2 * d:] = 0
    assert caught(no_vbias)
    monkeypatch.setattr(n64, "layernorm", lambda x, w, b, eps=n64.LN_EPS:
                        (x - x.mean(-1, keepdim=True)) * torch.rsqrt(x.var(-1, keepdim=True) + eps) * w + b)
    assert caught(W)                                 # unbiased variance: off by 1 / (2 d) relative
