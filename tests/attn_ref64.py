"""Dtype-generic restatement of the attention entry points (TEST INFRASTRUCTURE ONLY; never calls mevi_amd.ops).

    context[b, t, h] = softmax_j(scale q[b, t, h] . k[c, j, h] + bias[h, q_pos0 + t, j] + mask terms) . v[c, j, h],  c = b // kv_div

in the four layouts include/mevi_hip.h describes.  Every function takes the f32 host tensors a case is made of and returns
`fn(dtype, device)`, which f64_bar.refs runs once in float64 on the GPU and once in float32 on the host.  As in the kernels,
`scale` multiplies q before the dot product, and a masked key (key mask 0, or causal key > query position) gets -1e9 added to
its logit -- its weight underflows to an exact zero in either precision as long as the row has one real key."""
import torch


def _attend(qh, kh, vh, add, blocked=False):
    """qh [..., tq, dh], kh / vh [..., tk, dh], add [..., tq, tk] (broadcastable) -> [..., tq, dh]; all of one dtype.

    Both sums run in the kernels' order: the logit is a chain over the head's dims d = 0, 1, ... and the context a chain over
    the keys j = 0, 1, ... (the scalar kernels' fmaf chains; the matrix cores accumulate k-blocks in the same direction).  In
    float64 the order is immaterial; in float32 it makes e_32 the rounding error of THAT summation -- a blocked matmul's
    partial sums are smaller and its error several times lower, which says nothing about a kernel (measured on 96-wide heads,
    8 keys: chain kernel 9.3e-6, blocked f32 matmul 8.3e-7, f32 chain 7.3e-6).  The 16 x 16 matrix-core kernels are held to the
    same order on a measurement: on the 31 cases that MEVI_ATTN_SHORT=chain moves from them to a scalar-chain kernel the two
    kernels' e_hip agree to within 7 % (12 of them to the last digit), e.g. 2.88e-6 / 3.06e-6 at 17 tokens, 7.12e-6 / 7.36e-6 on
    packed sequences -- their error is a chain's, not a blocked sum's.  blocked=True is the library matmul instead: the
    yardstick of attention_mfma_kernel, which has no chain twin and needs no mirroring, and a second figure that every other
    matrix-core case records beside e_32 (e_32_blocked: e_hip stays below 4 x it on all of them too)."""
    if blocked:
        s = qh @ kh.transpose(-1, -2) + add
        return torch.softmax(s, -1) @ vh
    s = torch.zeros((), dtype=qh.dtype, device=qh.device)
    for d in range(qh.shape[-1]):
        s = s + qh[..., :, d, None] * kh[..., None, :, d]
    s = s + add
    s = s - s.max(-1, keepdim=True).values
    e = torch.exp(s)
    p = e / e.sum(-1, keepdim=True)
    out = torch.zeros((), dtype=qh.dtype, device=qh.device)
    for j in range(kh.shape[-2]):
        out = out + p[..., :, j, None] * vh[..., None, j, :]
    return out


def _heads(x, H):
    """[..., t, H*dh] -> [..., H, t, dh]"""
    return x.reshape(*x.shape[:-1], H, x.shape[-1] // H).transpose(-2, -3)


def _additive(dtype, device, H, tq, tk, bias, q_pos0, causal):
    """[H, tq, tk]: the bias rows q_pos0 .. q_pos0 + tq - 1 (first tk columns of a table that may be wider) + the causal term"""
    add = torch.zeros((H, tq, tk), dtype=dtype, device=device)
    if bias is not None:
        add = add + bias.to(device=device, dtype=dtype)[:, q_pos0:q_pos0 + tq, :tk]
    if causal:
        key = torch.arange(tk, device=device)[None, :]
        qpos = q_pos0 + torch.arange(tq, device=device)[:, None]
        add = add + (key > qpos).to(dtype)[None] * -1e9
    return add


def padded(q, k, v, H, kv_div=1, bias=None, q_pos0=0, key_mask=None, causal=False, scale=1.0, blocked=False):
    """mevi_attention_f32 without kv_off: q [nb, tq, H*dh], k / v [nb / kv_div, tk, H*dh], key_mask [nb / kv_div, tk] (1 = attend)
    -> [nb, tq, H*dh]"""
    def fn(dtype, device):
        nb, tq, hd = q.shape
        tk = k.shape[1]
        qh = _heads(q.to(device=device, dtype=dtype) * scale, H)
        kh = _heads(k.to(device=device, dtype=dtype), H).repeat_interleave(kv_div, 0)
        vh = _heads(v.to(device=device, dtype=dtype), H).repeat_interleave(kv_div, 0)
        add = _additive(dtype, device, H, tq, tk, bias, q_pos0, causal)[None]
        if key_mask is not None:
            m = key_mask.to(device).repeat_interleave(kv_div, 0)
            add = add + (m == 0).to(dtype)[:, None, None, :] * -1e9
        return _attend(qh, kh, vh, add, blocked).transpose(1, 2).reshape(nb, tq, hd)
    return fn


def packed_self(q, k, v, seq_off, H, bias=None, causal=False, scale=1.0, blocked=False):
    """mevi_attention_varlen_f32: q / k / v [T, H*dh], sequence b = rows seq_off[b] .. seq_off[b + 1] - 1 (a list), bias row and
    column = position inside the sequence -> the rows seq_off[0] .. seq_off[-1] - 1 of the context, [rows, H*dh]"""
    def fn(dtype, device):
        out = []
        for a, b in zip(seq_off[:-1], seq_off[1:]):
            n = b - a
            if n == 0:
                continue
            qh, kh, vh = (_heads(x[a:b].to(device=device, dtype=dtype), H) for x in (q, k, v))
            add = _additive(dtype, device, H, n, n, bias, 0, causal)
            out.append(_attend(qh * scale, kh, vh, add, blocked).transpose(0, 1).reshape(n, -1))
        return torch.cat(out)
    return fn


def packed_keys(q, k, v, kv_off, H, kv_div=1, bias=None, q_pos0=0, causal=False, scale=1.0, blocked=False):
    """mevi_attention_f32 with kv_off: q [nb, tq, H*dh], k / v [rows, H*dh], kv batch c = rows kv_off[c] .. kv_off[c + 1] - 1
    (a list), every key real -> [nb, tq, H*dh]"""
    def fn(dtype, device):
        nb, tq, hd = q.shape
        out = []
        for c, (a, b) in enumerate(zip(kv_off[:-1], kv_off[1:])):
            qh = _heads(q[c * kv_div:(c + 1) * kv_div].to(device=device, dtype=dtype) * scale, H)
            kh, vh = (_heads(x[a:b].to(device=device, dtype=dtype), H)[None] for x in (k, v))
            add = _additive(dtype, device, H, tq, b - a, bias, q_pos0, causal)[None]
            out.append(_attend(qh, kh, vh, add, blocked).transpose(1, 2).reshape(kv_div, tq, hd))
        return torch.cat(out)
    return fn


def cached(q, k, v, key_rows, H, bias=None, q_pos0=0, causal=True, scale=1.0, blocked=False):
    """mevi_attention_cached_f32: q [n, H*dh], k / v [rows, T, H*dh], key j of row b = k[key_rows[b, j], j] -> [n, H*dh]"""
    n, tk = key_rows.shape
    pos = torch.arange(tk)[None, :]
    kg, vg = k[key_rows.long(), pos], v[key_rows.long(), pos]
    inner = padded(q[:, None, :], kg, vg, H, bias=bias, q_pos0=q_pos0, causal=causal, scale=scale, blocked=blocked)
    return lambda dtype, device: inner(dtype, device).reshape(n, -1)


def triple_loop(q, k, v, H, kv_div=1, bias=None, q_pos0=0, key_mask=None, causal=False, scale=1.0):
    """The padded form once more as literal loops over rows, heads, queries and keys in Python floats (float64): what the
    vectorised restatement is itself checked against on tiny shapes."""
    import math

    nb, tq, hd = q.shape
    tk, dh = k.shape[1], hd // H
    out = torch.zeros((nb, tq, hd), dtype=torch.float64)
    ql, kl, vl = q.double().tolist(), k.double().tolist(), v.double().tolist()
    for b in range(nb):
        c = b // kv_div
        for h in range(H):
            for t in range(tq):
                s = []
                for j in range(tk):
                    x = sum(ql[b][t][h * dh + d] * scale * kl[c][j][h * dh + d] for d in range(dh))
                    if bias is not None:
                        x += float(bias[h, q_pos0 + t, j])
                    if key_mask is not None and int(key_mask[c, j]) == 0:
                        x += -1e9
                    if causal and j > q_pos0 + t:
                        x += -1e9
                    s.append(x)
                m = max(s)
                e = [math.exp(x - m) for x in s]
                z = sum(e)
                for d in range(dh):
                    out[b, t, h * dh + d] = sum(e[j] / z * vl[c][j][h * dh + d] for j in range(tk))
    return out
