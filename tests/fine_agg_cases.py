"""Inputs and expected values of the device fine stage's merge and weight modes (mevi_fine_topk_agg_f32): tests/
test_fine_agg_cpu.py proves from host arithmetic that every case reaches the path it is named for, tests/test_fine_agg_gpu.py
runs them through the call and against FineStage.rerank.

A case is `AggCase(base, aggregate, weights, doc_proba, ratio, rerank)`: `base` a fine_cases.Case (index, beam keys, query rows,
k, max_cand), `aggregate` None | 'add' | 'max', `weights` f32 [B, R] or None, `doc_proba` f32 [N] or None with `ratio`, and
`rerank`: whether FineStage.rerank models the case (it has no max_cand cut and reads every id as a row of the matrix).

Expected values restate the header's rules in numpy f32: the walk and q.d of fine_cases.expected (oracle.dense.pair_dot, the
pinned fmaf chain), cut to the first max_cand entries; the blend ratio * doc_proba[d] + (1 - ratio) * s and the weight
w[b, j] * s as separately rounded np.float32 operations; the fold of one id's entries in walk order, one f32 operation per
occurrence from +0 ('add') or -inf ('max'); -0 folded onto +0 as the sort keys do; np.lexsort by (score desc, id asc);
padding -FLT_MAX / -1 after the unique count.  No number here is a tolerance: the bar is bit equality."""
import functools
from typing import NamedTuple, Optional

import numpy as np

import fine_cases as fc
from oracle import dense as odense

SORT_MAX = fc.SORT_MAX                  # places the merge holds: FINE_SORT_MAX
SMALL_MAX = 2048                        # fine_topk.hip: FINE_SMALL_MAX, places of a query the 256-thread selection takes
AGG = {None: 0, "add": 1, "max": 2}


class AggCase(NamedTuple):
    base: fc.Case
    aggregate: Optional[str]
    weights: Optional[np.ndarray]
    doc_proba: Optional[np.ndarray]
    ratio: float
    rerank: bool


def _agg(base, aggregate=None, weights=None, doc_proba=None, ratio=0.0, rerank=True):
    def ro(a, shape):
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.float32)
        assert a.shape == shape, (a.shape, shape)
        a.setflags(write=False)
        return a

    assert aggregate in AGG and (doc_proba is None or weights is not None)
    return AggCase(base, aggregate, ro(weights, base.beam.shape), ro(doc_proba, (len(base.emb),)), float(ratio), bool(rerank))


def blend_terms(case):
    """(f32 ratio, f32 1 - ratio) as the host hands them over: the subtraction in double, then one rounding."""
    return np.float32(case.ratio), np.float32(1.0 - case.ratio)


def occurrences(case, b):
    """(document ids, beam slots, scores f32) of the entries of query b that compete, in walk order: the walk cut to max_cand
    places, ids outside [0, N) dropped, every score with its blend and weight applied; and the whole walk's count."""
    base = case.base
    R = base.beam.shape[1]
    docs, slot = fc.walk(base, b)
    ok = (docs >= 0) & (docs < len(base.emb))
    keep = ok[:base.max_cand]
    docs, slot = docs[:base.max_cand][keep], slot[:base.max_cand][keep]
    sc = np.zeros(len(docs), np.float32)
    if docs.size:
        if base.per_beam:
            for j in np.unique(slot):
                sc[slot == j] = odense.pair_dot(base.q[b * R + j], base.emb[docs[slot == j]])
        else:
            sc = odense.pair_dot(base.q[b], base.emb[docs])
    if case.weights is not None:
        if case.doc_proba is not None and case.ratio:
            r, omr = blend_terms(case)
            sc = (r * case.doc_proba[docs]).astype(np.float32) + (omr * sc).astype(np.float32)
        sc = (case.weights[b, slot] * sc).astype(np.float32)
    assert sc.dtype == np.float32
    return docs, slot, sc, int(ok.sum())


def fold(docs, sc, aggregate, reverse=False):
    """(unique ids ascending, folded scores): every id's entries in walk order (reverse: in the opposite order), one f32
    operation per occurrence."""
    order = np.lexsort((np.arange(len(docs)), docs))               # (id, place)
    ids, first, count = np.unique(docs[order], return_index=True, return_counts=True)
    acc = np.full(len(ids), 0.0 if aggregate == "add" else -np.inf, np.float32)
    for t in range(int(count.max()) if len(ids) else 0):
        has = count > t
        at = first[has] + (count[has] - 1 - t if reverse else t)
        s = sc[order][at]
        acc[has] = (acc[has] + s).astype(np.float32) if aggregate == "add" else np.fmax(acc[has], s)
    return ids, acc


def expected(case):
    """(scores f32 [B, k], ids i64 [B, k], ndoc i32 [B], nuniq i32 [B] or None without a merge)."""
    base = case.base
    B, k = base.beam.shape[0], base.k
    out_s = np.full((B, k), -odense.FLT_MAX, np.float32)
    out_i = np.full((B, k), -1, np.int64)
    ndoc = np.zeros(B, np.int32)
    nuniq = np.zeros(B, np.int32) if case.aggregate else None
    for b in range(B):
        docs, _, sc, ndoc[b] = occurrences(case, b)
        if case.aggregate:
            docs, sc = fold(docs, sc, case.aggregate)
            nuniq[b] = len(docs)
        sc = sc + np.float32(0.0)                                   # the keys fold -0 onto +0
        best = np.lexsort((docs, -sc))[:k]
        out_s[b, :len(best)], out_i[b, :len(best)] = sc[best], docs[best]
    for a in (out_s, out_i, ndoc, nuniq):
        if a is not None:
            a.setflags(write=False)
    return out_s, out_i, ndoc, nuniq


@functools.lru_cache(maxsize=None)
def expected_of(builder, *args):
    """`expected` of a cached case, computed once per process."""
    return expected(builder(*args))


def sorted_ids(case, b):
    """Ids of query b's competing entries in the merge's first order, (id, place)."""
    docs = occurrences(case, b)[0]
    return docs[np.lexsort((np.arange(len(docs)), docs))]


# ---- cases -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def minimal(mode):
    """One document in two beam clusters: B = 1, R = 2, dim 4; k = 2 shows the padding after the one unique entry."""
    base = fc._case([[1.0, -2.0, 0.5, 3.0]], [[0.25, 1.0, -4.0, 2.0]], {7: [0], 9: [0]}, [[9, 7]], 2)
    return _agg(base, mode)


RUN_SEED = 403                          # a seed for which adding in the reversed order changes the bits (test_fine_agg_cpu.py)


@functools.lru_cache(maxsize=None)
def longest_run(mode):
    """Document 0 in all of R = 128 clusters of one to three documents, a query row and a weight per beam: 128 different scores
    fold into one entry, so the order of the adds shows in the bits."""
    rng = np.random.default_rng(RUN_SEED)
    n, R = 200, 128
    clusters = {c: [0] + rng.choice(np.arange(1, n), size=int(rng.integers(0, 3)), replace=False).tolist() for c in range(R)}
    beam = rng.permutation(R)[None, :]
    base = fc._case(rng.standard_normal((R, 8)), rng.standard_normal((n, 8)), clusters, beam, 50, per_beam=True)
    return _agg(base, mode, weights=-rng.random((1, R)) - 0.1)


SEAMS = {False: (64, 256), True: (64, 256, 1024, 2048)}


@functools.lru_cache(maxsize=None)
def seams(wide, mode="add"):
    """Runs of four equal ids that straddle places 64 and 256 of the (id, place) order (a wave's and a 256-thread pass's
    seam; wide: also 1024 and 2048, the 1024-thread launch's), and a run of three that ends at the last place.  Cluster 1
    holds every id once; clusters 2..4 repeat the run ids, each beam under its own weight."""
    rng = np.random.default_rng(403 + wide)
    runs, pos, next_id = [], 0, 0
    for seam in SEAMS[wide]:
        next_id += seam - 2 - pos                                   # single ids up to two places before the seam
        runs.append(next_id)
        pos, next_id = seam + 2, next_id + 1
    last = next_id + 30
    clusters = {1: rng.permutation(last + 1).tolist(), 2: runs + [last], 3: [last] + runs[::-1], 4: runs}
    base = fc._case(rng.standard_normal((1, 8)), rng.standard_normal((last + 1, 8)), clusters, [[3, 1, 4, 2]], 40)
    return _agg(base, mode, weights=rng.standard_normal((1, 4)))


K_EDGE_UNIQUE = 45


@functools.lru_cache(maxsize=None)
def k_edges(which, mode="add"):
    """55 places of 45 unique documents: k one below, at and one above the unique count, and k = 4096."""
    rng = np.random.default_rng(404)
    clusters = {1: list(range(30)), 2: list(range(20, 45))}
    k = {"below": K_EDGE_UNIQUE - 1, "equal": K_EDGE_UNIQUE, "above": K_EDGE_UNIQUE + 1, "far above": 4096}[which]
    base = fc._case(rng.standard_normal((1, 8)), rng.standard_normal((45, 8)), clusters, [[2, 1]], k)
    return _agg(base, mode)


@functools.lru_cache(maxsize=None)
def full_sort(mode):
    """Exactly 16384 places: two clusters of 8192 sharing 4096 ids (12288 unique), weighted."""
    rng = np.random.default_rng(405)
    clusters = {0: rng.permutation(np.arange(0, 8192)).tolist(), 1: rng.permutation(np.arange(4096, 12288)).tolist()}
    base = fc._case(rng.standard_normal((1, 4)), rng.standard_normal((12288, 4)), clusters, [[1, 0]], 1000)
    return _agg(base, mode, weights=[[0.75, -1.5]])


TIE_IDS = (3, 7)


@functools.lru_cache(maxsize=None)
def ties(mode):
    """Documents 3 and 7 have bit-identical rows and sit in the same two clusters: their merged scores are equal bit for bit
    and the lower id comes first."""
    rng = np.random.default_rng(406)
    emb = rng.standard_normal((10, 8)).astype(np.float32)
    emb[TIE_IDS[1]] = emb[TIE_IDS[0]]
    clusters = {1: [7, 3, 1, 0], 2: [2, 3, 7, 9]}
    base = fc._case(rng.standard_normal((1, 8)), emb, clusters, [[1, 2]], 6)
    return _agg(base, mode, weights=[[0.5, 1.25]])


@functools.lru_cache(maxsize=None)
def negative_max():
    """Every score negative under 'max': the fold has to start from -inf, not from 0."""
    rng = np.random.default_rng(407)
    emb = -np.abs(rng.standard_normal((12, 4))) - 0.1
    clusters = {1: [0, 1, 2, 3, 4, 5], 2: [4, 5, 6, 7], 3: [5, 0, 8]}
    base = fc._case(np.abs(rng.standard_normal((1, 4))) + 0.1, emb, clusters, [[1, 2, 3]], 9)
    return _agg(base, "max", weights=[[1.0, 2.0, 0.5]])


@functools.lru_cache(maxsize=None)
def minus_zero_add():
    """Document 2 has a zero row and one occurrence under a negative weight: its score is -0, and 0 + -0 = +0."""
    rng = np.random.default_rng(408)
    emb = rng.standard_normal((6, 4)).astype(np.float32)
    emb[2] = 0.0
    clusters = {1: [0, 1, 2], 2: [0, 3]}
    base = fc._case(rng.standard_normal((1, 4)), emb, clusters, [[1, 2]], 5)
    return _agg(base, "add", weights=[[-1.0, -2.0]])


@functools.lru_cache(maxsize=None)
def repeated_key(mode):
    """A key twice (query 0) and three times (query 1) in a beam row with a merge: the repeats fold like any other."""
    rng = np.random.default_rng(409)
    base = fc.repeated_key(False)
    return _agg(base, mode, weights=rng.standard_normal(base.beam.shape))


@functools.lru_cache(maxsize=None)
def cut_between(mode):
    """max_cand = 13 against a walk of 10 + 5: document 3's two occurrences (places 3 and 10) both compete, document 5's second
    one (place 13) is cut off, so only its first folds."""
    rng = np.random.default_rng(410)
    clusters = {1: list(range(10)), 2: [3, 20, 21, 5, 6]}
    base = fc._case(rng.standard_normal((1, 8)), rng.standard_normal((22, 8)), clusters, [[1, 2]], 15, max_cand=13)
    return _agg(base, mode, weights=[[1.0, 3.0]], rerank=False)


@functools.lru_cache(maxsize=None)
def bad_ids(mode):
    """Ids outside [0, N) (-3, -1, 20, 29) inside clusters that overlap in documents 0, 3 and 4."""
    rng = np.random.default_rng(411)
    clusters = {1: [0, -3, 4, 20], 2: [29, 4, 3, 0], 3: [-1, 20, 4, 3]}
    base = fc._case(rng.standard_normal((2, 4)), rng.standard_normal((20, 4)), clusters, [[1, 2, 3], [3, 3, 1]], 6)
    return _agg(base, mode, rerank=False)


@functools.lru_cache(maxsize=None)
def weights_above_lds_sort():
    """Weights without a merge over 18000 places (the radix selection); the weights are log-probabilities, so negative."""
    rng = np.random.default_rng(412)
    base = fc.above_lds_sort(100)
    return _agg(base, None, weights=np.log(rng.random(base.beam.shape) * 0.9 + 0.05))


@functools.lru_cache(maxsize=None)
def blend(mode):
    """doc_proba with ratio 0.3 under beam weights, with and without a merge."""
    rng = np.random.default_rng(413)
    sizes = rng.integers(1, 30, size=12)
    clusters = {c: rng.choice(150, size=int(s), replace=False).tolist() for c, s in enumerate(sizes)}
    base = fc._case(rng.standard_normal((3, 36)), rng.standard_normal((150, 36)), clusters, rng.integers(0, 13, size=(3, 5)), 40,
                    max_cand=150)
    return _agg(base, mode, weights=np.log(rng.random((3, 5)) * 0.9 + 0.05), doc_proba=rng.random(150), ratio=0.3)


TILE_MAX_CAND = SORT_MAX
TILE_QUERIES = fc.CAND_CAP // (TILE_MAX_CAND * 8) + 3


@functools.lru_cache(maxsize=None)
def query_tiles(mode="add"):
    """The largest bound a merge takes, 16384 places a query (128 KiB each): 8192 queries fit the cap, so 8195 queries are a
    full tile and a ragged one of 3; the data stay tiny (R = 2, eight clusters of one to three documents)."""
    rng = np.random.default_rng(414)
    clusters = {c: rng.choice(12, size=int(rng.integers(1, 4)), replace=False).tolist() for c in range(8)}
    B = TILE_QUERIES
    base = fc._case(rng.standard_normal((B, 4)), rng.standard_normal((12, 4)), clusters, rng.integers(0, 9, size=(B, 2)), 4,
                    max_cand=TILE_MAX_CAND)
    return _agg(base, mode, weights=rng.standard_normal((B, 2)))


MODES = ("add", "max")
ALL = [(minimal, (m,)) for m in MODES] + [(longest_run, (m,)) for m in MODES] + \
      [(seams, (w, m)) for w in (False, True) for m in MODES] + \
      [(k_edges, (w,)) for w in ("below", "equal", "above", "far above")] + \
      [(full_sort, (m,)) for m in MODES] + [(ties, (m,)) for m in MODES] + [(negative_max, ()), (minus_zero_add, ())] + \
      [(repeated_key, (m,)) for m in MODES] + [(cut_between, (m,)) for m in MODES] + [(bad_ids, (m,)) for m in MODES] + \
      [(weights_above_lds_sort, ())] + [(blend, (m,)) for m in (None, "add", "max")] + [(query_tiles, ())]


def case_id(entry):
    builder, args = entry
    return builder.__name__ + "".join(f"-{a}" for a in args)
