"""The seq2seq arm's adaptor and PAWA head (mevi_amd/nci.py: Adaptor, NCIModel._logits, PrefixTables) restated in plain
torch at a chosen dtype (TEST INFRASTRUCTURE ONLY), in the style of tests/t5_ref64.py.

float64 is the yardstick the HIP forms are held to (tests/test_nci_f64_gpu.py); float32 is the same arithmetic at f32
rounding, pinned to oracle/t5.py on the G1 goldens' weights (tests/test_nci_ref64_cpu.py).  Every operation runs in the
dtype of its inputs and nothing casts.  Weights are the reference's state_dict names (t5_ref64.cast moves them); `cfg` is
the goldens' dict (d_model, M, K, adaptor_layer_num and the T5 keys)."""
import torch

import t5_ref64 as r64

NHEAD = 8        # nn.TransformerDecoderLayer(d, nhead=8)
LN_EPS = 1e-5    # nn.LayerNorm's default


def layernorm(x, w, b, eps=LN_EPS):
    """nn.LayerNorm: biased variance, in x's dtype."""
    xc = x - x.mean(-1, keepdim=True)
    return xc * torch.rsqrt(xc.pow(2).mean(-1, keepdim=True) + eps) * w + b


def _heads(t):
    return t.view(t.shape[0], t.shape[1], NHEAD, -1).transpose(1, 2)


def kv_proj(W, pre, mem):
    """The K|V rows nn.MultiheadAttention projects from `mem` [b, k, d] -> [b, k, 2d] (what Adaptor caches)."""
    d = mem.shape[-1]
    return mem @ W[pre + ".in_proj_weight"][d:].T + W[pre + ".in_proj_bias"][d:]


def mha(W, pre, x, mem, add=None):
    """nn.MultiheadAttention (8 heads, q scaled by (d/8)^-0.5, in_proj / out_proj with biases): queries x [b, t, d] over
    mem [b, k, d]; add = additive scores bias broadcastable to [b, 8, t, k].  Returns (output [b, t, d], K|V [b, k, 2d])."""
    d = x.shape[-1]
    q = x @ W[pre + ".in_proj_weight"][:d].T + W[pre + ".in_proj_bias"][:d]
    kv = kv_proj(W, pre, mem)
    s = (_heads(q) * (d // NHEAD) ** -0.5) @ _heads(kv[..., :d]).transpose(-1, -2)
    if add is not None:
        s = s + add
    ctx = (torch.softmax(s, dim=-1) @ _heads(kv[..., d:])).transpose(1, 2).reshape(x.shape)
    return ctx @ W[pre + ".out_proj.weight"].T + W[pre + ".out_proj.bias"], kv


def cross_const(W, pre, memory):
    """out_proj(v_proj(memory)) of the single memory vector [1, d]: what the one-key cross-attention reduces to."""
    d = memory.shape[-1]
    v = memory @ W[pre + ".in_proj_weight"][2 * d:].T + W[pre + ".in_proj_bias"][2 * d:]
    return v @ W[pre + ".out_proj.weight"].T + W[pre + ".out_proj.bias"]


def adaptor(W, cfg, tok_emb, n_layers=None):
    """nn.TransformerDecoder (post-LN) over the decode-token embeddings tok_emb [b, t, d]: causal self-attention, LN1;
    cross-attention over the single memory vector adaptor_embeddings, LN2; relu FFN, LN3.
    Returns (output [b, t, d], per-layer states [tok_emb, after layer 0, ...], per-layer self-attention K|V [b, t, 2d])."""
    b, t, d = tok_emb.shape
    n_layers = cfg["adaptor_layer_num"] if n_layers is None else n_layers
    mem = W["adaptor_embeddings"].reshape(1, 1, d).expand(b, 1, d)
    causal = r64.causal_bias(t, t, tok_emb.dtype, tok_emb.device)
    x = tok_emb
    hs, kvs = [x], []
    for l in range(n_layers):
        p = f"adaptor.layers.{l}"
        sa, kv = mha(W, p + ".self_attn", x, x, causal)
        x = layernorm(x + sa, W[p + ".norm1.weight"], W[p + ".norm1.bias"])
        x = layernorm(x + mha(W, p + ".multihead_attn", x, mem)[0], W[p + ".norm2.weight"], W[p + ".norm2.bias"])
        ff = torch.relu(x @ W[p + ".linear1.weight"].T + W[p + ".linear1.bias"]) @ W[p + ".linear2.weight"].T + W[p + ".linear2.bias"]
        x = layernorm(x + ff, W[p + ".norm3.weight"], W[p + ".norm3.bias"])
        hs.append(x)
        kvs.append(kv)
    return x, hs, kvs


def valid_columns(cfg, p, device=None):
    """Position p's valid tokens: eos (1), then the K codes 2 + pK .. 2 + (p + 1)K - 1."""
    K = cfg["K"]
    return torch.tensor([1] + list(range(2 + p * K, 2 + (p + 1) * K)), device=device)


def head_matrix(W, cfg, a, p):
    """adaptor_linear(a) restricted to position p's valid columns, plus lm_head's rows: [n, K + 1, d] with
    [n, c, i] = sum_e a[n, e] adaptor_linear.weight[i V + v_c, e] + lm_head.weight[v_c, i].  The columns are cut out of the
    weight before the product, so the [d V, d] product is never formed."""
    d = cfg["d_model"]
    lm = W["lm_head.weight"]
    cols = valid_columns(cfg, p, lm.device)
    w = W["adaptor_linear.weight"].view(d, lm.shape[0], d)[:, cols, :]            # [i, c, e]
    return torch.einsum("ne,ice->nci", a, w) + lm[cols]


def logits(W, cfg, seq, a, p):
    """[n, K + 1] = sum_i (seq[n, i] d^-0.5) head_matrix[n, c, i]: seq = the decoder stack's final-normed state, a = the
    adaptor's output, both of the last position p."""
    return ((seq * cfg["d_model"] ** -0.5)[:, None, :] * head_matrix(W, cfg, a, p)).sum(-1)


def position_logits(W, cfg, prefix_tokens, enc, enc_mask):
    """The valid columns' logits of the last position of prefix_tokens i64 [n, p + 1]: the full-prefix decoder
    (emb = decode_embeddings) over enc [n, s, d] under enc_mask, the adaptor on the same embeddings, the head."""
    p = prefix_tokens.shape[1] - 1
    emb = W["decode_embeddings.weight"][prefix_tokens]
    seq = r64.decoder(W, cfg, emb, enc, enc_mask)[:, -1]
    return logits(W, cfg, seq, adaptor(W, cfg, emb)[0][:, -1], p)
