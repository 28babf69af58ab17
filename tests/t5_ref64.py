"""The T5 blocks of mevi_amd/t5.py restated in plain torch at a chosen dtype (TEST INFRASTRUCTURE ONLY).

float64 is the yardstick the HIP blocks are held to (tests/test_t5_f64_gpu.py); float32 is the same arithmetic at f32
rounding, pinned to oracle/t5.py and the reference goldens (tests/test_t5_ref64_cpu.py).  Unlike oracle.t5.rmsnorm /
attention, nothing here casts to float32: every operation runs in the dtype of its inputs.  Weights are the reference's
state_dict names (a flat dict of tensors, any dtype/device: `cast` moves them).  Only the buckets come from the oracle.
"""
import numpy as np
import torch

from oracle.t5 import relative_position_bucket

NEG = -1e9


def cast(W, dtype, device=None):
    return {k: v.to(device=device if device is not None else v.device, dtype=dtype) for k, v in W.items()}


def rmsnorm(x, w, eps):
    """T5LayerNorm: w * x / sqrt(mean(x^2) + eps), in x's dtype."""
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def bias(W, pre, qlen, klen, bidirectional, buckets=32, q_pos0=0):
    """[1, H, qlen, klen] relative position bias of query positions q_pos0.. against key positions 0.."""
    rel = np.arange(klen)[None, :] - (q_pos0 + np.arange(qlen))[:, None]
    b = torch.from_numpy(relative_position_bucket(rel, bidirectional, buckets))
    table = W[pre + ".relative_attention_bias.weight"]
    return table[b.to(table.device)].permute(2, 0, 1).unsqueeze(0)


def mask_bias(key_mask, dtype):
    """[b, 1, 1, k] additive key mask (T5's extended attention mask: 0 or -1e9)."""
    return (1.0 - key_mask[:, None, None, :].to(dtype)) * NEG


def causal_bias(qlen, klen, dtype, device, q_pos0=0):
    keep = torch.arange(klen, device=device)[None, :] <= (q_pos0 + torch.arange(qlen, device=device))[:, None]
    return ((~keep).to(dtype) * NEG)[None, None]


def attention(W, pre, x, kv, add, H):
    """T5Attention (no 1/sqrt(d) scaling): x [b, q, d] queries, kv [b, k, d] (None: x), add = additive scores bias
    broadcastable to [b, H, q, k] (position bias + masks).  Returns the o-projected output [b, q, d]."""
    def heads(t):
        return t.view(t.shape[0], t.shape[1], H, -1).transpose(1, 2)

    src = x if kv is None else kv
    q = heads(x @ W[pre + ".q.weight"].T)
    k = heads(src @ W[pre + ".k.weight"].T)
    v = heads(src @ W[pre + ".v.weight"].T)
    p = torch.softmax(q @ k.transpose(-1, -2) + add, dim=-1)
    ctx = (p @ v).transpose(1, 2).reshape(x.shape[0], x.shape[1], -1)
    return ctx @ W[pre + ".o.weight"].T


def ffn(W, p, x):
    return torch.relu(x @ W[p + ".DenseReluDense.wi.weight"].T) @ W[p + ".DenseReluDense.wo.weight"].T


def encoder_layer(W, cfg, l, x, add, prefix="encoder"):
    """One T5Block of the encoder: x + SelfAttention(norm x), then + FFN(norm .).  add: position bias + key mask."""
    H, eps = cfg["num_heads"], cfg["layer_norm_epsilon"]
    p = f"{prefix}.block.{l}.layer"
    x = x + attention(W, f"{p}.0.SelfAttention", rmsnorm(x, W[f"{p}.0.layer_norm.weight"], eps), None, add, H)
    return x + ffn(W, f"{p}.1", rmsnorm(x, W[f"{p}.1.layer_norm.weight"], eps))


def decoder_layer(W, cfg, l, x, prefix_x, enc, sadd, xadd, prefix="decoder"):
    """One T5Block of the decoder for the query positions x [b, q, d]: self-attention over prefix_x [b, t, d] (the rows of
    the positions it attends to, x's own included; None: x itself), cross-attention over enc, FFN.  sadd / xadd: additive
    scores biases."""
    H, eps = cfg["num_heads"], cfg["layer_norm_epsilon"]
    p = f"{prefix}.block.{l}.layer"
    ln0 = W[f"{p}.0.layer_norm.weight"]
    hq = rmsnorm(x, ln0, eps)
    hk = hq if prefix_x is None else rmsnorm(prefix_x, ln0, eps)
    x = x + attention(W, f"{p}.0.SelfAttention", hq, hk, sadd, H)
    x = x + attention(W, f"{p}.1.EncDecAttention", rmsnorm(x, W[f"{p}.1.layer_norm.weight"], eps), enc, xadd, H)
    return x + ffn(W, f"{p}.2", rmsnorm(x, W[f"{p}.2.layer_norm.weight"], eps))


def final_norm(W, cfg, x, prefix):
    return rmsnorm(x, W[f"{prefix}.final_layer_norm.weight"], cfg["layer_norm_epsilon"])


def encoder(W, cfg, x, mask, prefix="encoder", n_layers=None, return_all=False):
    """T5Stack(is_decoder=False) from the embedded tokens x [b, s, d]: the final-normed states [, per-layer states]."""
    n_layers = cfg["num_layers"] if n_layers is None else n_layers
    S = x.shape[1]
    add = bias(W, f"{prefix}.block.0.layer.0.SelfAttention", S, S, True, cfg["relative_attention_num_buckets"])
    add = add + mask_bias(mask, x.dtype)
    hs = [x]
    for l in range(n_layers):
        x = encoder_layer(W, cfg, l, x, add, prefix)
        hs.append(x)
    out = final_norm(W, cfg, x, prefix)
    return (out, hs) if return_all else out


def decoder(W, cfg, x, enc, enc_mask, prefix="decoder", n_layers=None, return_all=False):
    """Full-prefix (no cache) decoder stack from the embedded decoder tokens x [b, t, d]: causal self-attention with the
    unidirectional bias, cross-attention over enc [b, s, d] under enc_mask.  The final-normed states [, per-layer]."""
    n_layers = cfg["num_decoder_layers"] if n_layers is None else n_layers
    T = x.shape[1]
    sadd = bias(W, f"{prefix}.block.0.layer.0.SelfAttention", T, T, False, cfg["relative_attention_num_buckets"])
    sadd = sadd + causal_bias(T, T, x.dtype, x.device)
    xadd = mask_bias(enc_mask, x.dtype)
    hs = [x]
    for l in range(n_layers):
        x = decoder_layer(W, cfg, l, x, None, enc, sadd, xadd, prefix)
        hs.append(x)
    out = final_norm(W, cfg, x, prefix)
    return (out, hs) if return_all else out


def tower_step(W, cfg, x0, enc, enc_mask, prefix="decoder", n_layers=None, return_all=False):
    """The towers' one-step decoder: position 0 only (its self-attention has one key, softmax weight 1, so the context is
    v), cross-attention over enc.  x0 [b, d] -> final-normed [b, d] [, per-layer states]."""
    n_layers = cfg["num_decoder_layers"] if n_layers is None else n_layers
    x = x0[:, None, :]
    sadd = bias(W, f"{prefix}.block.0.layer.0.SelfAttention", 1, 1, False, cfg["relative_attention_num_buckets"])
    xadd = mask_bias(enc_mask, x.dtype)
    hs = [x[:, 0]]
    for l in range(n_layers):
        x = decoder_layer(W, cfg, l, x, None, enc, sadd, xadd, prefix)
        hs.append(x[:, 0])
    out = final_norm(W, cfg, x, prefix)[:, 0]
    return (out, hs) if return_all else out


def tower_encode(W, cfg, ids, mask, emb="shared.weight"):
    """DocumentEncoder.encode: encoder on ids, then the one-step decoder on token 0 -> [b, d]."""
    enc = encoder(W, cfg, W[emb][ids], mask)
    x0 = W[emb][torch.zeros(ids.shape[0], dtype=torch.long, device=ids.device)]
    return tower_step(W, cfg, x0, enc, mask)
