"""The BERT encoder of mevi_amd/bert.py restated in plain torch at a chosen dtype (TEST INFRASTRUCTURE ONLY).

float64 is the yardstick the HIP tower is held to (tests/test_bert_f64_gpu.py); float32 is the same arithmetic at f32
rounding, pinned to oracle/bert.py and the reference's golden G8 (tests/test_bert_ref64_cpu.py).  Nothing here casts: every
operation runs in the dtype and on the device of its inputs (`cast` of t5_ref64 moves the weights).  Weights are the
reference's state_dict names; an optional `embeddings.task_type_embeddings.weight` (ERNIE with use_task_id) adds its row 0
to every position, as the model does with task_type_ids = 0.  cfg: num_attention_heads, layer_norm_eps, num_hidden_layers.
"""
import math

import torch

from t5_ref64 import cast  # noqa: F401  (re-exported: the tests move weights with it)

MASKED = -10000.0
TASK = "embeddings.task_type_embeddings.weight"


def layernorm(x, w, b, eps):
    """torch LayerNorm over the last dim in x's dtype: biased variance, eps inside the square root."""
    mu = x.mean(-1, keepdim=True)
    xc = x - mu
    var = xc.pow(2).mean(-1, keepdim=True)
    return xc / torch.sqrt(var + eps) * w + b


def embed(W, cfg, ids):
    """BertEmbeddings: LayerNorm(word[ids] + position[0..S-1] + token_type[0] (+ task_type[0])), [B, S, d]."""
    S = ids.shape[1]
    x = W["embeddings.word_embeddings.weight"][ids] + W["embeddings.position_embeddings.weight"][:S][None] \
        + W["embeddings.token_type_embeddings.weight"][0]
    if TASK in W:
        x = x + W[TASK][0]
    return layernorm(x, W["embeddings.LayerNorm.weight"], W["embeddings.LayerNorm.bias"], cfg["layer_norm_eps"])


def gelu(h):
    return h * 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0)))


def attention_block(W, cfg, l, x, add):
    """BertAttention of layer l: LayerNorm(dense(softmax(q k^T / sqrt(dh) + add) v) + x)."""
    B, S, d = x.shape
    H = cfg["num_attention_heads"]
    p = f"encoder.layer.{l}.attention."

    def lin(t, n):
        return t @ W[p + n + ".weight"].T + W[p + n + ".bias"]

    def heads(t):
        return t.view(B, S, H, d // H).transpose(1, 2)

    q, k, v = heads(lin(x, "self.query")), heads(lin(x, "self.key")), heads(lin(x, "self.value"))
    prob = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d // H) + add, dim=-1)
    ctx = (prob @ v).transpose(1, 2).reshape(B, S, d)
    return layernorm(lin(ctx, "output.dense") + x, W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"],
                     cfg["layer_norm_eps"])


def ffn_block(W, cfg, l, x):
    """BertIntermediate + BertOutput of layer l: LayerNorm(dense(gelu(dense(x))) + x)."""
    p = f"encoder.layer.{l}."
    h = gelu(x @ W[p + "intermediate.dense.weight"].T + W[p + "intermediate.dense.bias"])
    o = h @ W[p + "output.dense.weight"].T + W[p + "output.dense.bias"]
    return layernorm(o + x, W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"], cfg["layer_norm_eps"])


def encoder(W, cfg, ids, mask, n_layers=None, return_all=False):
    """BertModel without the pooler: last hidden state [B, S, d] [, the states after the embeddings and after every
    layer].  mask [B, S] of 0 / 1: masked keys get -10000 added to their scores."""
    n_layers = cfg["num_hidden_layers"] if n_layers is None else n_layers
    x = embed(W, cfg, ids)
    add = (1.0 - mask[:, None, None, :].to(x.dtype)) * MASKED
    hs = [x]
    for l in range(n_layers):
        x = ffn_block(W, cfg, l, attention_block(W, cfg, l, x, add))
        hs.append(x)
    return (x, hs) if return_all else x


def tower_encode(W, cfg, ids, mask, n_layers=None):
    """DocumentEncoder.encode of mtype 'bert': the last hidden state of position 0, [B, d]."""
    return encoder(W, cfg, ids, mask, n_layers)[:, 0, :]
