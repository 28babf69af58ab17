"""Expected values of the neighbour-graph index (include/mevi_hip_graph.h) and the small generators its tests share.  No number
here is a tolerance: the bar of the GPU tests is bit equality (scores as uint32, ids equal).

`link_expected` and `search_expected` restate the header in Python.  Scores come from `all_scores`: one
oracle.dense.ip_topk_exact(q, docs, nd) call returns every row's pinned fmaf chain, sorted; they are scattered back by id (the
same chain as oracle.dense.pair_dot; tests/test_hnsw_cpu.py holds the two equal on one case).  Everything else is numpy and
Python.  `search_expected` keeps no visited set unless asked to: the header says the result cannot depend on one."""
import bisect

import numpy as np

from oracle import dense as odense


def all_scores(q, docs):
    """f32 [nq, nd]: score(v) of every row for every query, -0 folded onto +0 as the keys of the search do."""
    q = np.ascontiguousarray(q, np.float32)
    docs = np.ascontiguousarray(docs, np.float32)
    nd = len(docs)
    out = np.empty((len(q), nd), np.float32)
    if nd == 0:
        return out
    s, i = odense.ip_topk_exact(q, docs, nd)
    assert (np.sort(i, axis=1) == np.arange(nd)).all()
    np.put_along_axis(out, i, s, axis=1)
    return out + np.float32(0.0)


def forward_links(knn, M):
    """[list] per row: the first M distinct entries of the row's list that are rows and not the row itself."""
    knn = np.asarray(knn, np.int64)
    nd = len(knn)
    out = []
    for v in range(nd):
        f = []
        for u in knn[v].tolist():
            if 0 <= u < nd and u != v and u not in f:
                f.append(u)
                if len(f) == M:
                    break
        out.append(f)
    return out


def link_expected(knn, M):
    """graph i32 [nd, 2 * M]: forward links, then the reverse candidates outside them in ascending (rank, source) order, -1."""
    fwd = forward_links(knn, M)
    nd, D = len(fwd), 2 * M
    cand = [[] for _ in range(nd)]
    for u, f in enumerate(fwd):
        for r, v in enumerate(f):
            cand[v].append((r, u))
    graph = np.full((nd, D), -1, np.int32)
    for v in range(nd):
        row = list(fwd[v])
        mine = set(row)
        for r, u in sorted(cand[v]):
            if len(row) == D:
                break
            if u not in mine:
                row.append(u)
        graph[v, :len(row)] = row
    return graph


def search_expected(scores, graph, seed, k, ef, width=1, max_steps=None, visited=False, seed_score=None):
    """(scores f32 [nq, k], ids i64 [nq, k], steps i32 [nq], rows scored [nq]).  scores f32 [nq, nd] = all_scores; graph
    [nd, degree]; seed [nq, nseed].  `visited`: keep an exact visited set (a node is scored once) -- the output must not change."""
    scores = np.asarray(scores, np.float32)
    graph = np.asarray(graph)
    nq, nd = scores.shape
    if max_steps is None:
        max_steps = 4 * ef
    out_s = np.full((nq, k), -odense.FLT_MAX, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    out_steps = np.zeros(nq, np.int32)
    out_rows = np.zeros(nq, np.int64)
    for n in range(nq):
        sc = scores[n]
        keys = (-sc.astype(np.float64)).tolist()          # exact: the order of f32 scores, as Python floats
        L, U = [], []                                     # (-score, id) ascending: the list, and its unexpanded entries
        inside, seen = set(), set()

        def take(nodes):
            for v in nodes:
                if v in inside or (visited and v in seen):
                    continue
                seen.add(v)
                out_rows[n] += 1
                key = (keys[v], v)
                if len(L) == ef and key > L[-1]:
                    continue
                bisect.insort(L, key)
                bisect.insort(U, key)
                inside.add(v)
                if len(L) > ef:
                    gone = L.pop()
                    inside.discard(gone[1])
                    at = bisect.bisect_left(U, gone)
                    if at < len(U) and U[at] == gone:
                        del U[at]                         # an evicted node's flag is gone with it

        first = []
        for j, v in enumerate(np.asarray(seed[n]).tolist()):
            if 0 <= v < nd:
                if seed_score is not None:
                    assert np.float32(seed_score[n][j]).view(np.uint32) == sc[v].view(np.uint32)
                first.append(v)
        take(first)
        steps = 0
        while steps < max_steps and U:
            todo, U[:width] = [v for _, v in U[:width]], []
            steps += 1
            S = []
            for v in todo:
                S += [u for u in graph[v].tolist() if 0 <= u < nd]
            take(S)
        best = [v for _, v in L[:k]]
        out_s[n, :len(best)] = sc[best]
        out_i[n, :len(best)] = best
        out_steps[n] = steps
    return out_s, out_i, out_steps, out_rows


def random_graph(rng, nd, degree, holes=0.0):
    """i32 [nd, degree]: independent draws (repeats and self loops happen), a share `holes` replaced by -1."""
    g = rng.integers(0, nd, size=(nd, degree)).astype(np.int32)
    if holes:
        g[rng.random(g.shape) < holes] = -1
    return g


def clustered(rng, nd, dim, n_clusters, spread=0.35):
    """f32 [nd, dim]: rows around `n_clusters` random centres."""
    centres = rng.standard_normal((n_clusters, dim)).astype(np.float32)
    return (centres[rng.integers(0, n_clusters, nd)] + spread * rng.standard_normal((nd, dim))).astype(np.float32)


def entry_rows(nd, limit=4096):
    """The entry rows of mevi_amd.hnsw: E = min(nd, limit) rows at a fixed stride, row floor(i * nd / E)."""
    E = min(nd, limit)
    return (np.arange(E, dtype=np.int64) * nd) // max(E, 1)


def seeds_expected(scores, nseed, limit=4096):
    """(seed i32 [nq, n], seed_score f32 [nq, n]), n = min(nseed, E): the best entry rows, score descending then id ascending."""
    nq, nd = scores.shape
    rows = entry_rows(nd, limit)
    n = min(nseed, len(rows))
    seed = np.empty((nq, n), np.int32)
    for i in range(nq):
        seed[i] = rows[np.lexsort((rows, -scores[i, rows]))[:n]]
    return seed, np.take_along_axis(scores, seed.astype(np.int64), axis=1)
