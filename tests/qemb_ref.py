"""numpy restatement of T5FineTuner.clus_repr (MEVI/main_models.py:1998-2047) with flatten=True, the --query_encoder nci
query embedding, plus the error bounds the GPU pool (csrc/query_pool.hip) is held to.

  enc f32 [B, S, d] (one row block per query), mask [B, S], dec f32 [B*R, T, d] or None, emb f32 [B*R, d] or None."""
import numpy as np

U = np.float32(2.0 ** -24)       # f32 unit roundoff


def pool_rows(qtower, enc, mask, dec, emb, R):
    """(rows f32 [B*R, L, d], row mask [B*R, L] or None) as clus_repr concatenates them: enc/encmask, dec, emb."""
    pieces = qtower.split("_")
    cands = []
    if "enc" in pieces or "encmask" in pieces:
        cands.append(np.repeat(enc, R, axis=0))
    if "dec" in pieces:
        cands.append(dec)
    if "emb" in pieces:
        cands.append(emb[:, None, :])
    h = np.concatenate(cands, axis=1).astype(np.float32)
    m = None
    if "encmask" in pieces:
        m = np.repeat(np.asarray(mask, np.int64), R, axis=0)
        m = np.concatenate([m, np.ones((m.shape[0], h.shape[1] - m.shape[1]), np.int64)], axis=1)
    return h, m


def clus_repr(qtower, accum, enc, mask, dec, emb, R, w=None, b=None):
    """f32 [B*R, d], each operation an f32 numpy operation in the reference's order."""
    h, m = pool_rows(qtower, enc, mask, dec, emb, R)
    if m is not None:
        h = h * m[:, :, None].astype(np.float32)
        ninf = np.where(m == 0, np.float32(-np.inf), np.float32(0.0)).astype(np.float32)
    if accum == "maxpool":
        if m is not None:
            h = h + ninf[:, :, None]
        return h.max(axis=1)
    if accum == "avgpool":
        if m is not None:
            return (h.sum(axis=1, dtype=np.float32) / m.sum(axis=1, keepdims=True).astype(np.float32)).astype(np.float32)
        return h.mean(axis=1, dtype=np.float32)
    assert accum == "attenpool"
    s = (h @ np.asarray(w, np.float32).reshape(-1, 1))[:, :, 0] + np.float32(b)
    if m is not None:
        s = s + ninf
    s = s - s.max(axis=1, keepdims=True)
    e = np.exp(s)
    p = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    return (h * p[:, :, None]).sum(axis=1, dtype=np.float32)


def exact_and_bound(qtower, accum, enc, mask, dec, emb, R, w=None, b=None):
    """(exact value in f64, elementwise bound) for avgpool / attenpool in f32 with L pooled rows:
      avgpool    |got - exact| <= gamma(L + 1) * sum_i |h_i| / n        (n = rows counted by the mean)
      attenpool  |got - exact| <= (2 * D + gamma(2 L + 8)) * sum_i p_i |h_i|,   D = max_i gamma(d + 1) * (|h_i|.|w| + |b|)
    with gamma(k) = k u / (1 - k u): the row scores carry at most D of absolute error each, so every softmax weight p_i
    is off by a relative 2 D plus the rounding of the exp / rescale / sum / divide chain."""
    h, m = pool_rows(qtower, enc, mask, dec, emb, R)
    h = h.astype(np.float64)
    L, d = h.shape[1], h.shape[2]
    g = lambda k: k * float(U) / (1 - k * float(U))  # noqa: E731
    keep = np.ones(h.shape[:2], bool) if m is None else m != 0
    hk = np.where(keep[:, :, None], h, 0.0)
    if accum == "avgpool":
        n = keep.sum(1)[:, None] if m is not None else L
        exact = hk.sum(1) / n
        return exact, g(L + 1) * np.abs(hk).sum(1) / n
    w = np.asarray(w, np.float64).reshape(-1)
    s = h @ w + float(b)
    s = np.where(keep, s, -np.inf)
    p = np.exp(s - s.max(1, keepdims=True))
    p = p / p.sum(1, keepdims=True)
    exact = (hk * p[:, :, None]).sum(1)
    D = (g(d + 1) * (np.abs(h) @ np.abs(w) + abs(float(b)))).max()
    return exact, (2 * D + g(2 * L + 8)) * (np.abs(hk) * p[:, :, None]).sum(1) + 1e-30


def load_golden(path):
    """(G1Q arrays, the npz of the G1 / G1T golden that holds the same model's weights: `w.*`, named by `weights_from`)."""
    import os

    g = np.load(path)
    return g, np.load(os.path.join(os.path.dirname(path), str(g["weights_from"])))
