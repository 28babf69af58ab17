"""Inputs and expected answers of the IVF-Flat build tests (tests/test_ivf_build_gpu.py): the nearest centroid by inner
product is oracle.dense.ip_topk_exact(x, centroids, 1) (sequential fmaf chains, lowest index on ties), the inverted lists
are numpy's stable argsort of the labels with the labels outside [0, nlist) left out."""
import numpy as np

from oracle import dense as odense

ASSIGN_N = (1, 127, 128, 129, 255, 256, 257, 513)
ASSIGN_NLIST = (1, 2, 63, 64, 65, 100, 127, 128, 129, 257)
ASSIGN_DIM = (4, 28, 36, 64)

LISTS_N = (1, 2, 1023, 1024, 1025, 65535, 65536, 65537, 300000)
LISTS_NLIST = (1, 2, 100, 1024, 1025, 4096, 262144)
LISTS_PATTERNS = ("first", "last", "round_robin", "empty_runs", "skewed", "out_of_range")


def nearest(x, centroids):
    """(list_of i32 [n], best_score f32 [n]) of the oracle."""
    s, i = odense.ip_topk_exact(x, centroids, 1)
    return i[:, 0].astype(np.int32), np.ascontiguousarray(s[:, 0])


def normal(seed, n, dim):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


# (c, c', ...): centroid c is copied to the later indices; each group is the winner of the rows aimed at it
TIE_GROUPS = ((3, 17),            # inside one 32-column accumulator
              (5, 37),            # the two 32-column sub-tiles (NI) of one wave
              (7, 71),            # the two column waves
              (9, 137),           # the next centroid tile (c + 128)
              (11, 267),          # two tiles on (c + 256)
              (13, 141, 269))     # c, c + 128, c + 256: the same lane and register in three tiles
TIE_NLIST = 300


def tie_case(n, dim=32, seed=11):
    """(x, centroids, winner): row r is aimed at group r % len(TIE_GROUPS), whose copies all attain its maximum; rows of
    zeros (every score +0: list 0 wins) are mixed in every 7th row (winner 0)."""
    cent = normal(seed, TIE_NLIST, dim)
    for group in TIE_GROUPS:
        for other in group[1:]:
            cent[other] = cent[group[0]]
    rng = np.random.default_rng(seed + 1)
    aim = np.arange(n) % len(TIE_GROUPS)
    first = np.array([g[0] for g in TIE_GROUPS])[aim]
    x = (3.0 * cent[first] + 0.05 * rng.standard_normal((n, dim))).astype(np.float32)
    zero = np.arange(n) % 7 == 6
    x[zero] = 0.0
    return x, cent, np.where(zero, 0, first).astype(np.int32)


def range_cases():
    """name -> (x, centroids): all scores negative; scores near +-3e38; the winner in the last real column next to the
    padded ones (the padded columns of a tile repeat the last centroid)."""
    rng = np.random.default_rng(21)
    out = {}
    x = np.abs(normal(22, 300, 36)) + 0.1
    out["all_negative"] = (x, -(np.abs(normal(23, 130, 36)) + 0.1))
    # one live coordinate: score = +-x0 * c0, |score| up to 3e38, every product and sum finite
    x = np.zeros((300, 8), np.float32)
    x[:, 0] = np.where(np.arange(300) % 2 == 0, 1.0, -1.0)
    c = np.zeros((200, 8), np.float32)
    c[:, 0] = (rng.random(200, dtype=np.float32) * 2 - 1) * np.float32(3e38)
    out["near_float_max"] = (x, c)
    c = np.zeros((150, 8), np.float32)
    c[:, 0] = -(rng.random(150, dtype=np.float32) * 0.5 + 0.5) * np.float32(3e38)     # every score of the even rows below -1.5e38
    out["all_near_minus_float_max"] = (np.ascontiguousarray(x[::2]), c)
    for nlist in (100, 130, 257):
        c = normal(24 + nlist, nlist, 32)
        x = (3.0 * c[np.full(200, nlist - 1)] + 0.05 * rng.standard_normal((200, 32))).astype(np.float32)
        out[f"last_column_{nlist}"] = (x, c)
    return out


def labels(pattern, n, nlist, seed=0):
    rng = np.random.default_rng(seed + n + 7 * nlist)
    if pattern == "first":
        return np.zeros(n, np.int32)
    if pattern == "last":
        return np.full(n, nlist - 1, np.int32)
    if pattern == "round_robin":
        return (np.arange(n) % nlist).astype(np.int32)
    if pattern == "empty_runs":                     # lists 5..9 of every 10 stay empty, and so does the tail
        live = np.flatnonzero((np.arange(nlist) % 10 < 5) & (np.arange(nlist) < max(1, nlist - 3)))
        return live[rng.integers(0, len(live), size=n)].astype(np.int32)
    if pattern == "skewed":
        return np.minimum(nlist - 1, (nlist * rng.random(n) ** 4).astype(np.int64)).astype(np.int32)
    if pattern == "out_of_range":
        lab = rng.integers(0, nlist, size=n).astype(np.int64)
        bad = rng.random(n) < 0.2
        lab[bad] = rng.choice(np.array([-1, nlist, 2 ** 31 - 1, -2 ** 31, nlist + 1]), size=int(bad.sum()))
        return lab.astype(np.int32)
    raise ValueError(pattern)


def lists(lab, nlist):
    """(list_offsets i64 [nlist + 1], row_ids i64 [listed rows], max_list_len) of the labels."""
    lab = lab.astype(np.int64)
    ok = (lab >= 0) & (lab < nlist)
    rows = np.flatnonzero(ok)
    order = rows[np.argsort(lab[rows], kind="stable")]
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(lab[rows], minlength=nlist))
    return offsets, order.astype(np.int64), int((offsets[1:] - offsets[:-1]).max())
