"""Expected values of the scalar-quantised index (include/mevi_hip_sq.h) from numpy f32 and existing oracle calls only, and the
small generators the SQ tests share.  No number here is a tolerance: the bar of the GPU tests is bit equality (scores as uint32,
ids and code bytes equal).  numpy neither fuses a product into a sum nor approximates a division, so every line below is the one
f32 operation the header names.

  range   vmin = min over rows, vdiff = max - min (of the residual x - centroid[list of x] behind an IVF)
  encode  c = (int)(L * clamp((r - vmin) / vdiff, 0, 1)), 0 where vdiff == 0; 4 bits: dimension 2i in the low nibble of byte i
  decode  vmin + vdiff * T[c], T[c] = (c + 0.5f) / L
  score   oracle.dense.pair_dot(q, decoded rows of the list) -- the sequential fmaf chain from +0; for all but the smallest lists
          through one oracle.dense.ip_topk_exact call per list, which returns the same chains -- then ONE f32 add of the slot's
          bias when there is one
  probes  an entry outside [0, nlist) is empty, a list named twice counts once, at its FIRST slot and with that slot's bias
  result  np.lexsort((ids, -scores))[:k], padded with -FLT_MAX / -1; ids compare as unsigned 32-bit values."""
import numpy as np

from oracle import dense as odense


def levels(bits):
    """f32 [2^bits]: the quotients (c + 0.5f) / L."""
    L = (1 << bits) - 1
    return (np.arange(L + 1, dtype=np.float32) + np.float32(0.5)) / np.float32(L)


def residual(x, list_of=None, centroids=None):
    x = np.asarray(x, np.float32)
    if centroids is None:
        return x
    r = x - np.asarray(centroids, np.float32)[np.asarray(list_of)]
    assert r.dtype == np.float32
    return r


def train_range(x, list_of=None, centroids=None):
    """(vmin, vdiff) f32 [dim] over ALL rows."""
    r = residual(x, list_of, centroids)
    vmin, vmax = r.min(0), r.max(0)
    vdiff = vmax - vmin
    assert vmin.dtype == np.float32 and vdiff.dtype == np.float32
    return vmin, vdiff


def quantise(r, vmin, vdiff, bits):
    """int32 [n, dim]: the level of every element."""
    L = np.float32((1 << bits) - 1)
    r, vmin, vdiff = np.asarray(r, np.float32), np.asarray(vmin, np.float32), np.asarray(vdiff, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        xi = (r - vmin) / vdiff
    assert xi.dtype == np.float32
    xi = np.where(vdiff == 0, np.float32(0), xi)
    xi = np.minimum(np.maximum(xi, np.float32(0)), np.float32(1))
    prod = L * xi
    assert prod.dtype == np.float32
    return prod.astype(np.int32)                                    # truncation


def pack(levels_, bits):
    """u8 [n, dim * bits / 8] of int levels [n, dim]."""
    c = np.asarray(levels_).astype(np.uint8)
    if bits == 8:
        return c
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def unpack(codes, bits):
    """int64 levels [n, dim] of u8 codes."""
    codes = np.asarray(codes, np.uint8)
    if bits == 8:
        return codes.astype(np.int64)
    out = np.empty((codes.shape[0], codes.shape[1] * 2), np.int64)
    out[:, 0::2] = codes & 15
    out[:, 1::2] = codes >> 4
    return out


def encode(x, vmin, vdiff, bits, list_of=None, centroids=None, rows=None):
    """u8 codes of x[rows] (rows None: of x), residuals taken with the list of the SOURCE row."""
    r = residual(x, list_of, centroids)
    if rows is not None:
        r = r[np.asarray(rows)]
    return pack(quantise(r, vmin, vdiff, bits), bits)


def decode(codes, vmin, vdiff, bits):
    """f32 [n, dim]: vmin + vdiff * T[c], the product and the sum rounded separately."""
    t = levels(bits)[unpack(codes, bits)]
    prod = np.asarray(vdiff, np.float32) * t
    out = np.asarray(vmin, np.float32) + prod
    assert prod.dtype == np.float32 and out.dtype == np.float32
    return out


def clean_slots(row, nlist):
    """[(slot, list)] of one probe row that survive: in range, first mention."""
    seen, out = set(), []
    for s, l in enumerate(np.asarray(row).tolist()):
        if 0 <= l < nlist and l not in seen:
            seen.add(l)
            out.append((s, l))
    return out


def sq_expected(q, codes, vmin, vdiff, bits, offsets, row_ids, probe, probe_score, k, max_list_len=None):
    """(scores f32 [nq, k], ids i64 [nq, k]).  codes u8 list-major, offsets i64 [nlist + 1], row_ids i64 [nd] or None (the id is
    the list-major row), probe [nq, nprobe], probe_score f32 [nq, nprobe] or None (no addition)."""
    q = np.ascontiguousarray(q, np.float32)
    offsets = np.asarray(offsets, np.int64)
    nlist = len(offsets) - 1
    rows = decode(codes, vmin, vdiff, bits)
    out_s = np.full((len(q), k), -odense.FLT_MAX, np.float32)
    out_i = np.full((len(q), k), -1, np.int64)
    slots = [clean_slots(probe[i], nlist) for i in range(len(q))]

    def bounds(l):
        a, b = int(offsets[l]), int(offsets[l + 1])
        return a, (b if max_list_len is None else min(b, a + max_list_len))

    chains = {}                                       # (query, list) -> the chains of the query over the list's rows
    for l in sorted({l for row in slots for _, l in row}):
        a, b = bounds(l)
        if b <= a:
            continue
        who = [i for i, row in enumerate(slots) if any(l_ == l for _, l_ in row)]
        if len(who) * (b - a) <= 64:                  # small: the definition itself, one call per row
            for i in who:
                chains[i, l] = odense.pair_dot(q[i], rows[a:b])
            continue
        # one call per list: k = all rows returns every chain (the same pinned fmaf chain from +0 as pair_dot), sorted; they are
        # put back by row (tests/test_sq_cpu.py holds the two routes equal bit for bit)
        s, c = odense.ip_topk_exact(q[who], rows[a:b], b - a)
        assert (np.sort(c, axis=1) == np.arange(b - a)).all()
        back = np.empty_like(s)
        np.put_along_axis(back, c, s, axis=1)
        for t, i in enumerate(who):
            chains[i, l] = back[t]
    for i in range(len(q)):
        scores, ids = [], []
        for s, l in slots[i]:
            a, b = bounds(l)
            if b <= a:
                continue
            chain = chains[i, l]
            assert chain.dtype == np.float32 and chain.shape == (b - a,)
            if probe_score is not None:
                chain = chain + np.float32(probe_score[i, s])
                assert chain.dtype == np.float32
            scores.append(chain)
            ids.append(np.arange(a, b, dtype=np.int64) if row_ids is None else np.asarray(row_ids, np.int64)[a:b])
        if not scores:
            continue
        scores, ids = np.concatenate(scores), np.concatenate(ids)
        best = np.lexsort((ids, -scores))[:k]
        out_s[i, :len(best)], out_i[i, :len(best)] = scores[best], ids[best]
    return out_s, out_i


def float64_scores(q, codes, vmin, vdiff, bits, bias):
    """Float64 scores of one query over rows `codes` from the f32 decoded rows' exact values, for checking the reference."""
    rows = decode(codes, vmin, vdiff, bits).astype(np.float64)
    return rows @ np.asarray(q, np.float64) + np.float64(bias)


def random_index(seed, dim, bits, nq, nd, nlist, nprobe, lens=None, repeats=False):
    """A random index given directly: (q, codes list-major, vmin, vdiff, bits, offsets, row_ids = a permutation, probe,
    probe_score).  The range has negative and positive minima; the probe rows name distinct lists, or with `repeats` independent
    draws (a list may come twice in a row)."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    if lens is None:
        list_of = np.sort(rng.integers(0, nlist, size=nd))
        lens = np.bincount(list_of, minlength=nlist)
    lens = np.asarray(lens, np.int64)
    nd = int(lens.sum())
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(lens)
    codes = rng.integers(0, 256, size=(nd, dim * bits // 8)).astype(np.uint8)
    vmin = (rng.standard_normal(dim) - 0.3).astype(np.float32)
    vdiff = (rng.random(dim) * 2 + 0.01).astype(np.float32)
    row_ids = np.concatenate([np.sort(c) for c in np.split(rng.permutation(nd).astype(np.int64), offsets[1:-1])]) if nd else np.zeros(0, np.int64)
    probe = (rng.integers(0, nlist, size=(nq, nprobe)) if repeats else np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)])).astype(np.int32)
    probe_score = rng.standard_normal((nq, nprobe)).astype(np.float32)
    return q, codes, vmin, vdiff, bits, offsets, row_ids, probe, probe_score
