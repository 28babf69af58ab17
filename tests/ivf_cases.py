"""Inputs, expected values and geometry of the IVF scan's edge cases (tests/test_ivf_cases_cpu.py proves from the geometry that
every case reaches the path it is named for; tests/test_ivf_scan_edges_gpu.py runs them through mevi_ivf_scan_topk_f32).

A case is `Case(q, d, list_of, probe, nlist, max_list_len, k, row_ids)` in numpy: `d` in the caller's row order, `list_of[j]` the
list of row j, `max_list_len` the bound handed to the kernel (it may exceed the longest list), `row_ids[j]` the id of row j
(None: the id is j).  Builders are cached and their arrays are read-only: every test shares one copy.

Expected values are the oracle's selection for a given probe table: per query the rows of its valid, de-duplicated lists in
ascending id order, scored and ranked by oracle.dense.ip_topk_exact on that subset (the pinned fmaf chain; lowest row on ties =
lowest id), padded with -FLT_MAX / -1.  Queries that probe the same set of lists share one oracle call.  No number in these
files is a tolerance: the bar is bit equality throughout."""
import functools
from typing import NamedTuple, Optional

import numpy as np

from oracle import dense as odense

PAIR_TILE, ROW_BLOCK = 64, 128          # MEVI_IVF_SCAN_PAIR_TILE / MEVI_IVF_SCAN_ROW_BLOCK (test_ivf_cases_cpu checks them)
MAX_QUERY_TILE = 4096                   # ivf_scan.hip: IVF_MAX_QT
CAND_CAP = 2 << 30                      # ivf_scan.hip: IVF_CAND_CAP
SCAN_GRID = 768                         # the scan kernel's largest grid
PLAN_CHUNK = 1024                       # lists per chunk of ivf_plan_kernel's scan


class Case(NamedTuple):
    q: np.ndarray
    d: np.ndarray
    list_of: np.ndarray
    probe: np.ndarray
    nlist: int
    max_list_len: int
    k: int
    row_ids: Optional[np.ndarray]


def _frozen(case):
    for a in case:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def _case(q, d, list_of, probe, nlist, k, max_list_len=None, row_ids=None):
    list_of = np.asarray(list_of, np.int64)
    longest = int(np.bincount(list_of, minlength=nlist).max()) if len(list_of) else 0
    return _frozen(Case(np.ascontiguousarray(q, np.float32), np.ascontiguousarray(d, np.float32), list_of,
                        np.ascontiguousarray(probe, np.int32), int(nlist), longest if max_list_len is None else int(max_list_len),
                        int(k), None if row_ids is None else np.asarray(row_ids, np.int64)))


def list_lengths(case):
    return np.bincount(case.list_of, minlength=case.nlist)


def list_major(case):
    """(docs list by list, offsets i64 [nlist + 1], ids of the list-major rows i64): what the kernel is handed.  Inside a list the
    caller's rows keep their order."""
    order = np.argsort(case.list_of, kind="stable")
    off = np.zeros(case.nlist + 1, np.int64)
    off[1:] = np.cumsum(list_lengths(case))
    ids = order.astype(np.int64) if case.row_ids is None else case.row_ids[order]
    return np.ascontiguousarray(case.d[order]), off, np.ascontiguousarray(ids)


def clean_probe(probe, nlist):
    """ivf_mark_kernel's table: entries outside [0, nlist) and every repeat of a list after its first slot become -1."""
    p = np.asarray(probe, np.int64)
    order = np.argsort(p, axis=1, kind="stable")
    sp = np.take_along_axis(p, order, 1)
    first_sorted = np.ones(sp.shape, bool)
    first_sorted[:, 1:] = sp[:, 1:] != sp[:, :-1]
    first = np.empty(sp.shape, bool)
    np.put_along_axis(first, order, first_sorted, 1)
    return np.where((p >= 0) & (p < nlist) & first, p, -1)


# ---- expected values ---------------------------------------------------------------------------------------------------
def _groups(case):
    """{sorted tuple of a query's valid lists: [queries]} and rows_of(list) in ascending row order."""
    order = np.argsort(case.list_of, kind="stable")
    off = np.concatenate([[0], np.cumsum(list_lengths(case))])
    groups = {}
    for i, row in enumerate(clean_probe(case.probe, case.nlist)):
        groups.setdefault(tuple(sorted(row[row >= 0].tolist())), []).append(i)
    return groups, lambda l: order[off[l]:off[l + 1]]


def expected(case):
    """(scores f32 [nq, k], ids i64 [nq, k]) of the oracle for the case's probe table."""
    nq, k = len(case.q), case.k
    out_s = np.full((nq, k), -odense.FLT_MAX, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    groups, rows_of = _groups(case)
    for lists, queries in groups.items():
        rows = np.sort(np.concatenate([rows_of(l) for l in lists])) if lists else np.zeros(0, np.int64)
        if rows.size == 0:
            continue
        qs, sub = case.q[queries], case.d[rows]
        if case.row_ids is None:                      # rows ascend = ids ascend: the oracle's tie order is the kernel's
            s, local = odense.ip_topk_exact(qs, sub, k)
            out_s[queries] = s
            out_i[queries] = np.where(local >= 0, rows[np.maximum(local, 0)], -1)
            continue
        s, local = odense.ip_topk_exact(qs, sub, len(rows))        # every score of the subset, then the caller's ids decide ties
        assert (local >= 0).all()
        for j, i in enumerate(queries):
            ids = case.row_ids[rows[local[j]]]
            best = np.lexsort((ids, -s[j]))[:k]
            out_s[i, :len(best)], out_i[i, :len(best)] = s[j][best], ids[best]
    out_s.setflags(write=False)
    out_i.setflags(write=False)
    return out_s, out_i


def expected_by_pair_dot(case):
    """The second route: one oracle_dot_f32 per row, then (score desc, id asc) by np.lexsort.  Slow; for small cases."""
    nq, k = len(case.q), case.k
    out_s = np.full((nq, k), -odense.FLT_MAX, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    ids_of = np.arange(len(case.d), dtype=np.int64) if case.row_ids is None else case.row_ids
    for i in range(nq):
        lists = [l for l in case.probe[i] if 0 <= l < case.nlist]
        rows = np.flatnonzero(np.isin(case.list_of, lists))
        if rows.size == 0:
            continue
        s = odense.pair_dot(case.q[i], case.d[rows])
        ids = ids_of[rows]
        best = np.lexsort((ids, -s))[:k]
        out_s[i, :len(best)], out_i[i, :len(best)] = s[best], ids[best]
    return out_s, out_i


# ---- geometry ----------------------------------------------------------------------------------------------------------
class Geometry(NamedTuple):
    tile: int              # queries per tile (ivf_plan: qt)
    tiles: list            # queries of every tile
    pairs: np.ndarray      # [tiles, nlist] surviving (query, slot) pairs per list
    items: np.ndarray      # [tiles, nlist] work items per list: ceil(pairs / 64) * ceil(min(len, max_len) / 128)
    grids: list            # the scan kernel's grid of every tile

    @property
    def item_totals(self):
        return self.items.sum(1)


def plan_geometry(probe, lens, nlist, max_list_len, nq, nprobe):
    """The host's tiling (ivf_plan, the loop of mevi_ivf_scan_topk_f32) and ivf_plan_kernel's counts, restated."""
    probe, lens = np.asarray(probe), np.asarray(lens, np.int64)
    assert probe.shape == (nq, nprobe) and lens.shape == (nlist,)
    ld = (max(1, max_list_len) + 3) & ~3
    per_q = nprobe * ld * 4
    assert per_q <= CAND_CAP
    tile = min(CAND_CAP // per_q, min(nq, MAX_QUERY_TILE))
    row_blocks = max(1, -(-max_list_len // ROW_BLOCK))
    clamped = np.minimum(lens, max_list_len)
    tiles, pairs, items, grids = [], [], [], []
    for q0 in range(0, nq, tile):
        clean = clean_probe(probe[q0:q0 + tile], nlist)
        cnt = np.bincount(clean[clean >= 0], minlength=nlist)
        tiles.append(len(clean))
        pairs.append(cnt)
        items.append(np.where((cnt > 0) & (clamped > 0), -(-cnt // PAIR_TILE) * -(-clamped // ROW_BLOCK), 0))
        grids.append(min(len(clean) * nprobe * row_blocks, SCAN_GRID))
    return Geometry(tile, tiles, np.array(pairs), np.array(items), grids)


def geometry(case):
    return plan_geometry(case.probe, list_lengths(case), case.nlist, case.max_list_len, len(case.q), case.probe.shape[1])


def walk_ranges(items, grid):
    """Per workgroup of one tile's scan: (lo, hi, list of item lo, list of item hi - 1); workgroups without items are left out."""
    off = np.concatenate([[0], np.cumsum(items)])
    total = int(off[-1])
    out = []
    for b in range(grid):
        lo, hi = total * b // grid, total * (b + 1) // grid
        if hi > lo:
            out.append((lo, hi, int(np.searchsorted(off, lo, "right")) - 1, int(np.searchsorted(off, hi - 1, "right")) - 1))
    return out


def linear_bins(scores):
    """ivf_select_kernel's first histogram in float32: (width, bin of every score)."""
    s = np.asarray(scores, np.float32)
    lo, hi = s.min(), s.max()
    with np.errstate(over="ignore", invalid="ignore"):
        width = np.float32(hi - lo)
        inv = np.float32(2047.0) / width if 0 < width < odense.FLT_MAX else np.float32(0)
        bins = np.nan_to_num((s - lo) * inv, nan=0.0, posinf=2047.0).astype(np.int64)
    return width, np.clip(bins, 0, 2047)


def probed_scores(case, query):
    """Every score of one query over its probed rows, descending (ids do not matter here)."""
    one = case._replace(q=case.q[query:query + 1], probe=case.probe[query:query + 1], k=1, row_ids=None)
    groups, rows_of = _groups(one)
    (lists,) = groups
    rows = np.sort(np.concatenate([rows_of(l) for l in lists]))
    return odense.ip_topk_exact(one.q, case.d[rows], len(rows))[0][0]


# ---- cases -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiles_by_query_count():
    """4096 + 65 queries: two tiles, the second 65 wide (2 bitmap words per list instead of 64); the queries on either side of
    the seam probe different lists.  1100 lists also put the plan kernel's carry under every tile."""
    rng = np.random.default_rng(101)
    nq, nd, nlist = 4096 + 65, 3000, 1100
    probe = rng.integers(0, nlist, size=(nq, 2))
    probe[4094], probe[4095], probe[4096], probe[4097] = (5, 1099), (1030, 17), (700, 3), (1023, 1024)
    return _case(rng.standard_normal((nq, 4)), rng.standard_normal((nd, 4)), rng.integers(0, nlist, size=nd), probe, nlist, 10)


@functools.lru_cache(maxsize=None)
def tiles_by_candidate_cap():
    """nprobe 256 with max_list_len = nd = 262144 as the bound: 256 * 262144 * 4 bytes = 256 MiB of candidates a query, 8 queries a
    tile, 20 queries = tiles of 8, 8, 4.  300 lists of 300..1500 rows, k 4096."""
    rng = np.random.default_rng(102)
    nq, nd, nlist, nprobe = 20, 262144, 300, 256
    lens = rng.integers(300, 1449, size=nlist)
    while lens.sum() != nd:                                       # nudge single lists until the rows add up
        l = rng.integers(0, nlist)
        step = int(np.clip(nd - lens.sum(), 300 - lens[l], 1500 - lens[l]))
        lens[l] += step
    list_of = rng.permutation(np.repeat(np.arange(nlist), lens))
    probe = np.stack([rng.choice(nlist, size=nprobe, replace=False) for _ in range(nq)])
    for i in range(1, nq):                                        # query 0 keeps its 256 distinct lists
        slots = rng.choice(nprobe, size=6, replace=False)
        probe[i, slots[:3]] = -1
        probe[i, slots[3:]] = probe[i, (slots[3:] + 7) % nprobe]  # a list named twice
    return _case(rng.standard_normal((nq, 4)), rng.standard_normal((nd, 4)), list_of, probe, nlist, 4096, max_list_len=nd)


@functools.lru_cache(maxsize=None)
def item_walk_many_lists():
    """1100 lists of 1..200 rows, one in five empty and three runs of twenty empty ones; 1500 queries at nprobe 1 reach every
    list: more than 768 lists have items, so workgroups cross from list to list and over the empty ones."""
    rng = np.random.default_rng(103)
    nlist, nq = 1100, 1500
    lens = rng.integers(1, 201, size=nlist)
    lens[np.arange(nlist) % 5 == 2] = 0
    for first in (300, 600, 900):
        lens[first:first + 20] = 0
    list_of = rng.permutation(np.repeat(np.arange(nlist), lens))
    probe = (np.arange(nq) * 7 % nlist)[:, None]
    return _case(rng.standard_normal((nq, 4)), rng.standard_normal((len(list_of), 4)), list_of, probe, nlist, 10)


@functools.lru_cache(maxsize=None)
def item_walk_centroids():
    """40 unit centroids on a circle of the first two axes (the other two are zero)."""
    theta = 2 * np.pi * np.arange(40) / 40
    c = np.zeros((40, 4), np.float32)
    c[:, 0], c[:, 1] = np.cos(theta), np.sin(theta)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def item_walk_long_lists():
    """40 lists of 1409..1536 rows (12 row blocks) with 65..130 queries each (2 or 3 pair tiles): more than 900 items, so
    every workgroup walks several items of one list.  Rows and queries sit within 0.4 of the centroid spacing of their
    centroid's angle, so the lists also follow from item_walk_centroids() by the index's own assignment."""
    rng = np.random.default_rng(104)
    cent = item_walk_centroids()
    nlist = len(cent)
    lens = rng.integers(1409, 1537, size=nlist)
    aims = rng.integers(65, 131, size=nlist)
    aims[:3] = 65, 128, 130

    def around(labels):
        angle = 2 * np.pi * (labels + rng.uniform(-0.4, 0.4, size=len(labels))) / nlist
        x = rng.standard_normal((len(labels), 4))
        radius = rng.uniform(0.5, 2.0, size=len(labels))
        x[:, 0], x[:, 1] = radius * np.cos(angle), radius * np.sin(angle)
        return x.astype(np.float32)

    d = around(rng.permutation(np.repeat(np.arange(nlist), lens)))
    q = around(rng.permutation(np.repeat(np.arange(nlist), aims)))
    list_of = odense.ip_topk_exact(d, cent, 1)[1][:, 0]
    probe = odense.ip_topk_exact(q, cent, 1)[1]
    return _case(q, d, list_of, probe, nlist, 100)


@functools.lru_cache(maxsize=None)
def plan_carry(nlist):
    """Lists of 0..3 rows, 150 rows in the lists around 1024 and 2048; probes (nprobe 2) concentrated on 1020..1030 and
    2040..2048, pairs of lists on either side of a boundary among them.  Lists at or past `nlist` are empty probes."""
    rng = np.random.default_rng(105)
    lens = rng.integers(0, 4, size=nlist)
    hot = np.array([l for l in list(range(1020, 1031)) + list(range(2040, 2049)) if l < nlist])
    lens[hot] = 150
    list_of = rng.permutation(np.repeat(np.arange(nlist), lens))
    seams = [(1023, 1024), (1024, 1023), (1022, 1025), (2047, 2048), (2048, 2047), (1023, 2048), (0, 1024), (nlist - 1, 0)]
    probe = np.concatenate([np.array(seams), rng.choice(np.concatenate([hot, [1030, 2048]]), size=(150, 2)),
                            rng.integers(0, nlist, size=(60, 2))])
    return _case(rng.standard_normal((len(probe), 4)), rng.standard_normal((len(list_of), 4)), list_of, probe, nlist, 20)


EDGE_LENS = (0, 1, 2, 3, 4, 5, 31, 32, 33, 127, 128, 129, 255, 256, 257, 600)
EDGE_PAIR_COUNTS = (31, 32, 33, 63, 64, 65, 127, 128, 129)
EDGE_DIMS = (4, 28, 36)


@functools.lru_cache(maxsize=None)
def pair_and_row_edges(c):
    """`c` queries that all probe all 16 lists of EDGE_LENS (each in its own slot order): every list has exactly `c` pairs.
    The dim follows from c's place in EDGE_PAIR_COUNTS: 4 (the minimum), 28 (tail loop only), 36 (one chunk of 32 + a tail)."""
    dim = EDGE_DIMS[EDGE_PAIR_COUNTS.index(c) % 3]
    rng = np.random.default_rng(106 + c)
    nlist = len(EDGE_LENS)
    list_of = rng.permutation(np.repeat(np.arange(nlist), EDGE_LENS))
    probe = np.stack([rng.permutation(nlist) for _ in range(c)])
    return _case(rng.standard_normal((c, dim)), rng.standard_normal((len(list_of), dim)), list_of, probe, nlist, 50)


SELECT_TOTAL = 4000
SELECT_KS = (1, 2, 3, 5, SELECT_TOTAL - 1, SELECT_TOTAL, SELECT_TOTAL + 1)


def _five_lists(rng, nd=5000):
    return rng.permutation(np.repeat(np.arange(5), [1000, 900, 1100, 1000, nd - 4000]))


@functools.lru_cache(maxsize=None)
def select_k(k):
    """5000 rows in five lists; both queries probe four lists of 4000 rows in all: k around that total and the smallest ks."""
    rng = np.random.default_rng(107)
    return _case(rng.standard_normal((2, 4)), rng.standard_normal((5000, 4)), _five_lists(rng), [[0, 1, 2, 3], [4, 2, 1, 0]], 5, k)


@functools.lru_cache(maxsize=None)
def select_overflow(k):
    """Queries +-1e19 e_0, first column of the rows spread over +-3e19: scores reach +-3e38, stay finite, and hi - lo is inf in
    float32.  k = 100 ends among the positive scores, k = 2600 among the negative ones."""
    rng = np.random.default_rng(108)
    d = rng.standard_normal((5000, 4)).astype(np.float32)
    d[:, 0] = rng.uniform(-3e19, 3e19, size=5000).astype(np.float32)
    q = np.zeros((2, 4), np.float32)
    q[0, 0], q[1, 0] = 1e19, -1e19
    return _case(q, d, _five_lists(rng), [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]], 5, k)


@functools.lru_cache(maxsize=None)
def select_crowded_top():
    """3000 of 5000 scores are 1 - j * 2^-24, j = 0..3 (four values within three ulp of the maximum), the others lie in
    [-1, 0.5): the top linear bin alone holds more than k = 100 entries and the k-th place cuts the run of the maximum."""
    rng = np.random.default_rng(109)
    d = rng.standard_normal((5000, 4)).astype(np.float32)
    d[:, 0] = rng.uniform(-1.0, 0.5, size=5000).astype(np.float32)
    top = rng.choice(5000, size=3000, replace=False)
    d[top, 0] = (1.0 - rng.integers(0, 4, size=3000) * 2.0 ** -24).astype(np.float32)
    q = np.zeros((1, 4), np.float32)
    q[0, 0] = 1.0
    return _case(q, d, _five_lists(rng), [[3, 1, 4, 0, 2]], 5, 100)


def _tie_ids(rng, n_run, n_all):
    """Unique ids in [0, 2^32): the run of equals gets the corner values, ids that differ only above bit 21 (the id radix's
    first pass) and ids that differ only in bits 10..20 (its second); everything else is random."""
    corners = [0, 1, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 2, (1 << 32) - 1]
    high = [0x155555 | (j << 21) for j in range(1, 60)]
    middle = [(0x5A5 << 21) | (j << 10) | 0x2AA for j in range(1, 60)]
    run = np.array(corners + high + middle, np.int64)
    assert len(run) == n_run == len(set(run.tolist()))
    rest = np.zeros(0, np.int64)
    while len(rest) < n_all - n_run:
        rest = np.setdiff1d(np.union1d(rest, rng.integers(0, 1 << 32, size=n_all - n_run - len(rest))), run)
    return rng.permutation(run), rng.permutation(rest)


TIE_RUN = 128
TIE_PLACES = ("last", "one before last", "first")


@functools.lru_cache(maxsize=None)
def _tie_corpus(given_ids):
    rng = np.random.default_rng(110)
    nd = 2000
    d = rng.standard_normal((nd, 4)).astype(np.float32)
    v = rng.standard_normal(4).astype(np.float32)
    copies = rng.choice(nd, size=TIE_RUN + 5, replace=False)
    d[copies[:TIE_RUN]] = v
    d[copies[TIE_RUN:]] = 1.5 * v
    list_of = np.sort(rng.integers(0, 3, size=nd))                # list-major already: with row_ids = None the id is the row
    row_ids = None
    if given_ids:
        run, rest = _tie_ids(rng, TIE_RUN, nd)
        row_ids = np.empty(nd, np.int64)
        row_ids[copies[:TIE_RUN]] = run
        row_ids[np.setdiff1d(np.arange(nd), copies[:TIE_RUN])] = rest
    q = (4 * v)[None, :]
    scores = odense.ip_topk_exact(q, d, nd)[0][0]
    tie = odense.pair_dot(q[0], v[None, :])[0]
    assert (scores == tie).sum() == TIE_RUN
    return q, d, list_of, row_ids, int((scores > tie).sum()), copies[:TIE_RUN]


def tie_layout(given_ids=True):
    """(rows scoring above the run of equals, rows of the run)."""
    return _tie_corpus(given_ids)[4:]


@functools.lru_cache(maxsize=None)
def ties(place, given_ids=True):
    """128 bit-identical rows over three lists under one query; k puts the k-th place on the run's last row (the run is taken
    whole: need == n_eq, no cut), on the one before it (need == n_eq - 1) or on its first (need == 1)."""
    q, d, list_of, row_ids, above, _ = _tie_corpus(given_ids)
    need = {"last": TIE_RUN, "one before last": TIE_RUN - 1, "first": 1}[place]
    return _case(q, d, list_of, [[2, 0, 1]], 3, above + need, row_ids=row_ids)


NOTHING_LENS = (0, 50, 0, 200, 0, 30)


@functools.lru_cache(maxsize=None)
def nothing_to_scan(kind):
    """70 queries, nprobe 3 over six lists, three of them empty: a table of -1 ("no probes"), a table that names only the empty
    lists ("empty lists"), and a table over every list ("normal") for the call that follows on the same workspace."""
    rng = np.random.default_rng(111)
    nlist, nq = len(NOTHING_LENS), 70
    list_of = rng.permutation(np.repeat(np.arange(nlist), NOTHING_LENS))
    q, d = rng.standard_normal((nq, 8)), rng.standard_normal((len(list_of), 8))
    normal = rng.integers(0, nlist, size=(nq, 3))
    probe = {"no probes": np.full((nq, 3), -1), "empty lists": rng.choice([0, 2, 4], size=(nq, 3)), "normal": normal}[kind]
    return _case(q, d, list_of, probe, nlist, 40)


@functools.lru_cache(maxsize=None)
def small_for_both_routes():
    """A few hundred rows with ties, padding, empty and repeated probes: small enough for one oracle_dot_f32 per row."""
    rng = np.random.default_rng(112)
    d = rng.standard_normal((400, 8)).astype(np.float32)
    d[rng.choice(400, size=60, replace=False)] = d[0]
    probe = rng.integers(-1, 7, size=(12, 3))
    probe[3] = -1
    probe[4] = 2
    return _case(rng.standard_normal((12, 8)), d, rng.integers(0, 6, size=400), probe, 6, 150)


@functools.lru_cache(maxsize=None)
def expected_of(builder, *args):
    """`expected` of a cached case, computed once per process."""
    return expected(builder(*args))
