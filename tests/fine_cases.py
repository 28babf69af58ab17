"""Inputs, expected values and geometry of the device fine stage's cases (tests/test_fine_topk_cpu.py proves from host
arithmetic that every case reaches the path it is named for and that oracle.dense.fine_stage reproduces the expected lists;
tests/test_fine_topk_gpu.py runs them through mevi_fine_topk_f32).

A case is `Case(q, emb, keys, offsets, docs, beam, k, max_cand, per_beam)` in numpy: `keys` / `offsets` / `docs` are the CSR
arrays of the cluster index (keys ascending and distinct), `beam` i64 [B, R] the beam keys, `q` f32 [B, dim] or, with per_beam,
[B * R, dim] (row b * R + j scores beam j of query b), `max_cand` the bound handed to the kernel (it may exceed every walk, or
-- one case -- fall short of one).  Builders are cached and their arrays are read-only: every test shares one copy.

Expected values: per query the walk over its beam row (cluster after cluster in stored order, a repeated key again, an absent
or negative key nothing, ids outside [0, N) dropped), cut to the first max_cand entries, scored by oracle.dense.pair_dot (the
pinned fmaf chain) and ordered (score desc, id asc) by np.lexsort, padded with -FLT_MAX / -1; ndoc counts the whole walk.
No number in these files is a tolerance: the bar is bit equality throughout."""
import functools
from typing import NamedTuple

import numpy as np

from oracle import dense as odense

CAND_CAP = 1 << 30                      # fine_topk.hip: FINE_CAND_CAP (scores + ids of a tile, 8 bytes a place)
MAX_QUERY_TILE = 16384                  # fine_topk.hip: FINE_MAX_QT
SORT_MAX = 16384                        # fine_topk.hip: FINE_SORT_MAX, places the LDS sort holds
SCORE_CHUNK = 128                       # candidates a workgroup of fine_score_kernel scores per step


class Case(NamedTuple):
    q: np.ndarray
    emb: np.ndarray
    keys: np.ndarray
    offsets: np.ndarray
    docs: np.ndarray
    beam: np.ndarray
    k: int
    max_cand: int
    per_beam: bool


def csr(clusters):
    """{key: [doc ids]} -> (keys ascending, offsets, docs) as i64 arrays."""
    keys = np.array(sorted(clusters), np.int64)
    sizes = np.array([len(clusters[int(c)]) for c in keys], np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    docs = np.array([d for c in keys for d in clusters[int(c)]], np.int64)
    return keys, offsets, docs


def clusters_of(case):
    """The CSR arrays back as {key: doc id array}."""
    return {int(c): case.docs[a:b] for c, a, b in zip(case.keys, case.offsets[:-1], case.offsets[1:])}


def largest_walk(clusters, R):
    """The bound FineStage.max_candidates computes: the R largest clusters together, at least 1.  It holds for rows of distinct
    keys; the cases that repeat a key in a row name their bound themselves."""
    return max(1, int(sum(sorted((len(v) for v in clusters.values()), reverse=True)[:R])))


def _case(q, emb, clusters, beam, k, max_cand=None, per_beam=False):
    beam = np.ascontiguousarray(beam, np.int64)
    keys, offsets, docs = csr(clusters)
    case = Case(np.ascontiguousarray(q, np.float32), np.ascontiguousarray(emb, np.float32), keys, offsets, docs, beam, int(k),
                largest_walk(clusters, beam.shape[1]) if max_cand is None else int(max_cand), bool(per_beam))
    assert case.q.shape[0] == beam.shape[0] * (beam.shape[1] if per_beam else 1)
    for a in case:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def walk(case, b):
    """(document ids, beam slot of every entry) of query b's whole walk, ids outside [0, N) included."""
    cl = clusters_of(case)
    parts = [(cl[int(key)], j) for j, key in enumerate(case.beam[b]) if int(key) in cl]
    if not parts:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate([d for d, _ in parts]), np.concatenate([np.full(len(d), j, np.int64) for d, j in parts])


def expected(case):
    """(scores f32 [B, k], ids i64 [B, k], ndoc i32 [B])."""
    B, R = case.beam.shape
    n = len(case.emb)
    out_s = np.full((B, case.k), -odense.FLT_MAX, np.float32)
    out_i = np.full((B, case.k), -1, np.int64)
    ndoc = np.zeros(B, np.int32)
    for b in range(B):
        docs, slot = walk(case, b)
        ok = (docs >= 0) & (docs < n)
        ndoc[b] = ok.sum()
        keep = ok[:case.max_cand]
        docs, slot = docs[:case.max_cand][keep], slot[:case.max_cand][keep]
        if docs.size == 0:
            continue
        if case.per_beam:
            sc = np.empty(len(docs), np.float32)
            for j in np.unique(slot):
                sc[slot == j] = odense.pair_dot(case.q[b * R + j], case.emb[docs[slot == j]])
        else:
            sc = odense.pair_dot(case.q[b], case.emb[docs])
        best = np.lexsort((docs, -sc))[:case.k]
        out_s[b, :len(best)], out_i[b, :len(best)] = sc[best], docs[best]
    for a in (out_s, out_i, ndoc):
        a.setflags(write=False)
    return out_s, out_i, ndoc


@functools.lru_cache(maxsize=None)
def expected_of(builder, *args):
    """`expected` of a cached case, computed once per process."""
    return expected(builder(*args))


# ---- geometry ----------------------------------------------------------------------------------------------------------
def query_tile(nq, max_cand):
    """fine_plan's tile, restated: the queries whose places (align4(max_cand) * 8 bytes) fit the cap, at most 16384."""
    per_q = ((max_cand + 3) & ~3) * 8
    assert per_q <= CAND_CAP
    return min(CAND_CAP // per_q, nq, MAX_QUERY_TILE)


def places(case):
    """Entries of every query's walk the kernel keeps: min(whole walk, max_cand) -- what decides between the LDS sort and the
    radix selection."""
    return np.array([min(len(walk(case, b)[0]), case.max_cand) for b in range(len(case.beam))])


# ---- cases -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def minimal():
    """B = R = k = 1, one cluster of one document, dim 4."""
    return _case([[1.0, -2.0, 0.5, 3.0]], [[0.25, 1.0, -4.0, 2.0]], {7: [0]}, [[7]], 1)


@functools.lru_cache(maxsize=None)
def key_kinds():
    """Keys found, absent (below the first, between two, above the last), negative, the first and the last of cluster_keys; query
    3 finds no cluster at all, query 4 only the first key, query 5 only the last."""
    rng = np.random.default_rng(201)
    clusters = {3: [4, 9], 10: [0, 1, 2], 11: [7], 500: [3, 5, 6, 8], 1 << 40: [10, 11]}
    beam = [[10, 4, -1, 500], [1 << 40, 3, 11, 12], [2, 3, 10, (1 << 40) + 1], [-7, 0, 499, 1 << 41], [3, -1, -1, -1],
            [-1, 9, 1 << 40, 600]]
    return _case(rng.standard_normal((6, 8)), rng.standard_normal((12, 8)), clusters, beam, 5)


@functools.lru_cache(maxsize=None)
def one_cluster():
    """n_clusters = 1: the binary search over a single key, hit from one beam and missed on either side."""
    rng = np.random.default_rng(202)
    return _case(rng.standard_normal((3, 4)), rng.standard_normal((9, 4)), {42: [8, 0, 3, 5]}, [[42, 41], [43, 42], [41, 43]], 3)


@functools.lru_cache(maxsize=None)
def no_clusters():
    """n_clusters = 0: the kernel gets null CSR pointers; everything is padding."""
    rng = np.random.default_rng(203)
    return _case(rng.standard_normal((2, 4)), rng.standard_normal((5, 4)), {}, [[0, 1, 2], [5, -1, 0]], 4)


EDGE_SIZES = (1, 63, 64, 65, 129, 5000)


@functools.lru_cache(maxsize=None)
def cluster_sizes():
    """Clusters of 1, 63, 64, 65, 129 and 5000 documents (key = size) at R = 10: a wave's 64 lanes and a workgroup's 128
    candidates are met exactly, by one more and by one less; query 0 walks all six (5322 candidates, 42 chunks), the others
    walk one size alone or pairs whose seam falls inside a wave."""
    rng = np.random.default_rng(204)
    n = sum(EDGE_SIZES)
    ids = rng.permutation(n)
    clusters, at = {}, 0
    for s in EDGE_SIZES:
        clusters[s] = np.sort(ids[at:at + s]).tolist()
        at += s
    pad = [-1] * 10
    beam = [[5000, 1, 65, 7, 63, 129, 64, -1, 2, 66]] + [([s] + pad)[:10] for s in EDGE_SIZES[:5]] + \
           [([63, 1] + pad)[:10], ([1, 63, 64, 65] + pad)[:10], ([129, 129, 65] + pad)[:10]]
    return _case(rng.standard_normal((len(beam), 8)), rng.standard_normal((n, 8)), clusters, beam, 50)


@functools.lru_cache(maxsize=None)
def many_beams():
    """R = 128 with one-document clusters; a few beams are absent and the last beam counts."""
    rng = np.random.default_rng(205)
    clusters = {c: [c] for c in range(300)}
    beam = np.stack([rng.choice(300, size=128, replace=False) for _ in range(3)])
    beam[1, [0, 17, 127]] = (-1, 300, 1000)
    return _case(rng.standard_normal((3, 4)), rng.standard_normal((300, 4)), clusters, beam, 128)


DIMS = (4, 36, 768)


@functools.lru_cache(maxsize=None)
def dims(dim, per_beam=False):
    """dim 4 (one float4), 36 (one 32-slab and a tail of 4) and 768 (24 slabs): 5 queries, R = 4, clusters of 0..40."""
    rng = np.random.default_rng(206 + dim)
    sizes = rng.integers(1, 41, size=30)
    ids = rng.permutation(int(sizes.sum()))
    off = np.concatenate([[0], np.cumsum(sizes)])
    clusters = {int(c) * 3: ids[off[c]:off[c + 1]].tolist() for c in range(30)}
    beam = rng.integers(0, 30, size=(5, 4)) * 3
    beam[2, 1] = 4                                                   # absent
    return _case(rng.standard_normal((5 * (4 if per_beam else 1), dim)), rng.standard_normal((len(ids), dim)), clusters, beam, 20,
                 max_cand=160, per_beam=per_beam)


@functools.lru_cache(maxsize=None)
def k_edges(which):
    """One query of 37 + 5 candidates: k one below, at and one above the count (the last with padding), and k = 4096 over it."""
    rng = np.random.default_rng(207)
    clusters = {1: list(range(37)), 2: list(range(40, 45))}
    k = {"below": 41, "equal": 42, "above": 43, "far above": 4096}[which]
    return _case(rng.standard_normal((1, 8)), rng.standard_normal((45, 8)), clusters, [[2, 1]], k)


@functools.lru_cache(maxsize=None)
def k4096_of_5000():
    """k = 4096 of one cluster of 5000: the LDS sort over 8192 keys, half of them written out."""
    rng = np.random.default_rng(208)
    return _case(rng.standard_normal((1, 4)), rng.standard_normal((5000, 4)), {9: rng.permutation(5000).tolist()}, [[9, 8]], 4096)


@functools.lru_cache(maxsize=None)
def above_lds_sort(k):
    """Query 0: 3 x 6000 = 18000 candidates, more than the LDS sort holds: the radix selection.  Query 1 walks one of the
    clusters (6000: the sort) under the same launch."""
    rng = np.random.default_rng(209)
    ids = rng.permutation(18000)
    clusters = {c: ids[6000 * c:6000 * (c + 1)].tolist() for c in range(3)}
    return _case(rng.standard_normal((2, 4)), rng.standard_normal((18000, 4)), clusters, [[2, 0, 1], [1, -1, 5]], k)


TIE_RUN = 96


@functools.lru_cache(maxsize=None)
def ties(large):
    """TIE_RUN bit-identical embedding rows (scattered ids) whose score is cut by the k-th place after a third of the run: the
    lowest ids win.  small: 400 candidates (LDS sort); large: 18000 (radix selection, id pass at the cut)."""
    rng = np.random.default_rng(210 + large)
    n = 18000 if large else 400
    emb = rng.standard_normal((n, 4)).astype(np.float32)
    v = rng.standard_normal(4).astype(np.float32)
    run = rng.choice(n, size=TIE_RUN, replace=False)
    emb[run] = v
    q = (2 * v)[None, :]
    scores = odense.pair_dot(q[0], emb)
    tie = odense.pair_dot(q[0], v[None, :])[0]
    assert (scores == tie).sum() == TIE_RUN
    ids = rng.permutation(n)
    third = n // 3
    clusters = {c: ids[third * c:third * (c + 1)].tolist() for c in range(2)}
    clusters[2] = ids[2 * third:].tolist()
    return _case(q, emb, clusters, [[1, 2, 0]], int((scores > tie).sum()) + TIE_RUN // 3)


def tie_run_ids(large):
    """Ids of the run of equal scores, ascending."""
    case = ties(large)
    s = odense.pair_dot(case.q[0], case.emb)
    values, counts = np.unique(s, return_counts=True)
    return np.flatnonzero(s == values[np.argmax(counts)])


@functools.lru_cache(maxsize=None)
def zero_query(large):
    """An all-zero query: every score is +0 and the ids alone decide (hi == lo in the selection's first histogram)."""
    rng = np.random.default_rng(212)
    n = 17000 if large else 300
    ids = rng.permutation(n)
    clusters = {5: ids[:n // 2].tolist(), 6: ids[n // 2:].tolist()}
    return _case(np.zeros((1, 4)), rng.standard_normal((n, 4)), clusters, [[6, 5]], 40)


@functools.lru_cache(maxsize=None)
def repeated_key(per_beam):
    """A key twice (query 0) and three times (query 1) in a beam row: its documents are listed and scored again.  With one
    embedding per query the repeats are identical (score, id) entries; with per-beam embeddings the same id carries one score
    per beam.  k = 25 cuts query 1's triples after the first entry of one of them."""
    rng = np.random.default_rng(213)
    clusters = {1: list(range(0, 12)), 2: list(range(12, 30)), 3: list(range(30, 33))}
    beam = [[1, 2, 1, 3], [2, 2, -1, 2], [3, 1, 2, 0]]
    return _case(rng.standard_normal((3 * (4 if per_beam else 1), 8)), rng.standard_normal((33, 8)), clusters, beam, 25,
                 max_cand=60, per_beam=per_beam)


@functools.lru_cache(maxsize=None)
def repeated_key_large():
    """One cluster of 6000 named three times: 18000 candidates in identical triples through the radix selection; k = 100 ends
    on the first entry of the 34th triple, so of three entries equal in score AND id exactly one belongs to the list."""
    rng = np.random.default_rng(214)
    return _case(rng.standard_normal((1, 4)), rng.standard_normal((6000, 4)), {4: rng.permutation(6000).tolist()}, [[4, 4, 4]], 100,
                 max_cand=18000)


TILE_MAX_CAND = 2_000_000


@functools.lru_cache(maxsize=None)
def query_tiles():
    """B = 70, R = 10 with a bound of 2 000 000 candidates a query (16 MB of places each): 67 queries fit the cap, so the call
    walks a tile of 67 and a ragged one of 3, while the data stay tiny (clusters of 0..6 documents)."""
    rng = np.random.default_rng(215)
    sizes = rng.integers(0, 7, size=200)
    ids = rng.permutation(int(sizes.sum()))
    off = np.concatenate([[0], np.cumsum(sizes)])
    clusters = {c: ids[off[c]:off[c + 1]].tolist() for c in range(200)}
    return _case(rng.standard_normal((70, 8)), rng.standard_normal((len(ids), 8)), clusters, rng.integers(0, 220, size=(70, 10)), 10,
                 max_cand=TILE_MAX_CAND)


@functools.lru_cache(maxsize=None)
def short_bound(per_beam=False):
    """max_cand = 100 against walks of 30 + 80 + 45 (query 0: cut inside its second cluster, the third dropped whole), 80 + 30
    (query 1: cut inside its second), 45 + 30 (query 2: untouched) and 100 exactly (query 3).  Keys are distinct inside a row."""
    rng = np.random.default_rng(216)
    ids = rng.permutation(175)
    clusters = {1: ids[:30].tolist(), 2: ids[30:110].tolist(), 3: ids[110:155].tolist(), 4: ids[155:175].tolist()}
    beam = [[1, 2, 3], [2, 1, -1], [3, 9, 1], [2, 4, 0]]
    return _case(rng.standard_normal((4 * (3 if per_beam else 1), 8)), rng.standard_normal((175, 8)), clusters, beam, 60,
                 max_cand=100, per_beam=per_beam)


@functools.lru_cache(maxsize=None)
def bad_ids():
    """Document ids outside [0, N) in the index (-3, N, N + 9): skipped, not scored and not counted."""
    rng = np.random.default_rng(217)
    clusters = {1: [0, -3, 4, 20], 2: [29, 7, 3], 3: [-1, 20, 29]}
    return _case(rng.standard_normal((2, 4)), rng.standard_normal((20, 4)), clusters, [[1, 2, 3], [3, 3, 0]], 6)


ALL = [(minimal, ()), (key_kinds, ()), (one_cluster, ()), (no_clusters, ()), (cluster_sizes, ()), (many_beams, ())] + \
      [(dims, (d, p)) for d in DIMS for p in (False, True)] + \
      [(k_edges, (w,)) for w in ("below", "equal", "above", "far above")] + \
      [(k4096_of_5000, ()), (above_lds_sort, (100,)), (above_lds_sort, (4096,)), (ties, (False,)), (ties, (True,)),
       (zero_query, (False,)), (zero_query, (True,)), (repeated_key, (False,)), (repeated_key, (True,)), (repeated_key_large, ()),
       (query_tiles, ()), (short_bound, (False,)), (short_bound, (True,)), (bad_ids, ())]


def case_id(entry):
    builder, args = entry
    return builder.__name__ + "".join(f"-{a}" for a in args)
