"""Expected values of the upper levels of the neighbour-graph index (include/mevi_hip_graph_levels.h, mevi_amd/hnsw.py) and the
generators their tests share; tests/graph_cases.py holds the level-0 half and is imported, not changed.  No number here is a
tolerance: the bar of the GPU tests is bit equality (scores as uint32, ids equal).

`level_sizes` / `level_maps` restate the arithmetic of the index.  `descend_expected` restates the header: per level one
gc.search_expected over the columns of gc.all_scores that the level's `rows` name, holes masked out, its best entries renamed
by `down` into the seeds of the level below."""
import numpy as np

import graph_cases as gc
from oracle import dense as odense

FLT_MAX = np.float32(odense.FLT_MAX)


def level_sizes(nd, M, entry_rows=4096):
    """[n_0 .. n_T]: n_0 = nd, n_l = n_{l-1} // M, up to the first level of at most `entry_rows` nodes."""
    sizes = [int(nd)]
    while True:
        sizes.append(sizes[-1] // M)
        if sizes[-1] <= entry_rows:
            return sizes


def walked_levels(nd, M, entry_rows=4096, limit=8):
    """U = T - 1 when an index of this shape has walked levels, else 0 (it is the strided index)."""
    sizes = level_sizes(nd, M, entry_rows)
    U = len(sizes) - 2
    return U if 1 <= U <= limit and sizes[-1] >= 1 else 0


def level_maps(sizes):
    """(down, rows), entry l - 1 = level l: down_l[j] = (j * n_{l-1}) // n_l, rows_l = the composition down to level 0."""
    down, rows = [], []
    for l in range(1, len(sizes)):
        d = (np.arange(sizes[l], dtype=np.int64) * sizes[l - 1]) // max(sizes[l], 1)
        down.append(d)
        rows.append(d if l == 1 else rows[-1][d])
    return down, rows


def top_seeds_expected(scores, top_rows, top_ids, nseed):
    """(seed i64 [nq, n], seed_score f32 [nq, n]), n = min(nseed, n_T): the best rows of the top level by (score descending, item
    id ascending), named by their item ids (`down` of the top level: local ids of the level below)."""
    nq = scores.shape[0]
    n = min(nseed, len(top_rows))
    seed = np.empty((nq, n), np.int64)
    score = np.empty((nq, n), np.float32)
    for i in range(nq):
        s = scores[i, top_rows]
        best = np.lexsort((top_ids, -s.astype(np.float64)))[:n]
        seed[i], score[i] = top_ids[best], s[best]
    return seed, score


def descend_expected(scores, nd, graphs, rows, down, seed, seed_score, ef, width=1, max_steps=None, nseed_out=None, visited=False):
    """(out_seed i32 [nq, nseed_out], out_score f32, steps i32 [nq] summed over the levels, rows scored [nq] without the carried
    seeds -- with `visited` the rows an exact visited set scores, a lower bound of what a lossy table scores).
    scores f32 [nq, nd] = gc.all_scores; graphs / rows / down: one array per walked level, level 1 first; seed i64 [nq, nseed_in]
    local ids of the last level with their scores."""
    U = len(graphs)
    nq = scores.shape[0]
    if max_steps is None:
        max_steps = 4 * ef
    if nseed_out is None:
        nseed_out = min(ef, 32)
    seed = np.asarray(seed, np.int64)
    seed_score = np.asarray(seed_score, np.float32)
    steps = np.zeros(nq, np.int64)
    scored = np.zeros(nq, np.int64)
    for l in range(U, 0, -1):
        r = np.asarray(rows[l - 1], np.int64)
        g = np.asarray(graphs[l - 1], np.int64).copy()
        n = len(r)
        node = (r >= 0) & (r < nd)                                      # the others are holes
        sc = np.ascontiguousarray(scores[:, np.where(node, r, 0)])
        inside = (g >= 0) & (g < n)
        g[inside & ~node[np.clip(g, 0, n - 1)]] = -1                    # a link to a hole is a hole
        s_in = (seed >= 0) & (seed < n)
        seed = np.where(s_in & node[np.clip(seed, 0, n - 1)], seed, -1)
        out_s, out_i, st, rows_scored = gc.search_expected(sc, g, seed, nseed_out, ef, width, max_steps, visited=visited,
                                                           seed_score=seed_score)
        steps += st
        for q in range(nq):                                             # search_expected counts the seeds it takes as scored
            first, L = [], set()
            for v in seed[q].tolist():
                if v >= 0 and v not in L:
                    first.append(v)
                    L.add(v)
            scored[q] += rows_scored[q] - (len(first) if visited else _seed_takes(sc[q], seed[q], ef))
        d = np.where(out_i >= 0, np.asarray(down[l - 1], np.int64)[np.clip(out_i, 0, n - 1)], -1)
        below = nd if l == 1 else len(rows[l - 2])
        seed = np.where((d >= 0) & (d < below), d, -1)
        seed_score = out_s
    out_score = np.where(seed >= 0, seed_score, -FLT_MAX).astype(np.float32)
    return seed.astype(np.int32), out_score, steps.astype(np.int32), scored


def _seed_takes(sc, seed, ef):
    """How many of its seeds gc.search_expected (no visited set) counts as scored: every seed that is not in the list when its
    turn comes -- a repeat of a seed the full list has refused or evicted is counted again."""
    import bisect

    L, inside, count = [], set(), 0
    for v in seed.tolist():
        if v < 0 or v in inside:
            continue
        count += 1
        key = (-float(sc[v]), v)
        if len(L) == ef and key > L[-1]:
            continue
        bisect.insort(L, key)
        inside.add(v)
        if len(L) > ef:
            inside.discard(L.pop()[1])
    return count


def random_levels(rng, nd, sizes, degree, holes=0.1, bad=0.05):
    """(graphs, rows, down) of walked levels of the given sizes (level 1 first) with RANDOM consistent maps: down_l draws nodes of
    the level below with repeats and in no order, rows_l = rows_{l-1}[down_l] (a node stands for one row on every level, as the
    header demands), rows_1 random rows.  Then a share `bad` of every level's `down` and, independently, of its `rows` is put
    outside its range (negative, or past the end): nodes that are walked but dropped on the way down, and holes -- also holes
    under a node that is none on the level above."""
    graphs, rows, down = [], [], []
    clean = None
    for l, n in enumerate(sizes, start=1):
        if l == 1:
            r = rng.integers(0, nd, n)
            d = r.copy()
        else:
            d = rng.integers(0, sizes[l - 2], n)
            r = clean[d]
        clean = r
        d, r = d.copy(), r.copy()
        limit = nd if l == 1 else sizes[l - 2]
        if bad and n > 4:
            at = rng.random(n) < bad
            d[at] = np.where(rng.random(at.sum()) < 0.5, -1 - rng.integers(0, 5, at.sum()), limit + rng.integers(0, 7, at.sum()))
            at = rng.random(n) < bad
            r[at] = np.where(rng.random(at.sum()) < 0.5, -1 - rng.integers(0, 5, at.sum()), nd + rng.integers(0, 7, at.sum()))
        g = gc.random_graph(rng, n, degree, holes)
        g[::7, 0] = np.arange(n)[::7]                                  # self loops
        if degree > 2:
            g[::5, 1] = g[::5, 2]                                      # repeats inside a row
        g[::11, degree - 1] = n + 3                                    # past the level's end: the next level's rows in the array
        graphs.append(g.astype(np.int32))
        rows.append(r.astype(np.int32))
        down.append(d.astype(np.int32))
    return graphs, rows, down
