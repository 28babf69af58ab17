"""mevi_graph_search_topk_f32 (csrc/graph_search.hip) against tests/graph_cases.py: search_expected, the header restated in
Python over oracle scores.  Bar: bit equality -- scores as uint32, ids, steps."""
import numpy as np
import pytest
import torch

import graph_cases as gc
from mevi_amd import dense, hip

pytestmark = pytest.mark.gpu
FLT_MAX = np.finfo(np.float32).max


def _make(seed, nd, dim, degree, nq, nseed, holes=0.1, dup_rows=0):
    rng = np.random.default_rng(seed)
    docs = rng.standard_normal((nd, dim)).astype(np.float32)
    if dup_rows:                                                       # only `dup_rows` distinct rows: ties everywhere
        docs = docs[rng.integers(0, dup_rows, nd)]
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    g = gc.random_graph(rng, nd, degree, holes)
    g[::7, 0] = np.arange(nd)[::7]                                     # self loops
    g[::5, 1] = g[::5, 2]                                              # repeats inside a row
    g[1::2, 3] = g[0:nd - 1:2, 3][:len(g[1::2])]                       # rows 2i and 2i + 1 share a neighbour
    seed_ids = rng.integers(0, nd, size=(nq, nseed)).astype(np.int32)
    return rng, docs, q, g, seed_ids


def _run(cuda, docs, q, g, seed, k, ef, width=1, max_steps=None, with_score=True, sc=None, workspace=None):
    sc = gc.all_scores(q, docs) if sc is None else sc
    nd = len(docs)
    seed_score = None
    if with_score:                                                     # the chain's score where the seed is a row, junk elsewhere
        ok = (seed >= 0) & (seed < nd)
        seed_score = np.where(ok, np.take_along_axis(sc, np.clip(seed, 0, max(nd - 1, 0)).astype(np.int64), axis=1), np.float32(7e30))
        seed_score = seed_score.astype(np.float32)
    want = gc.search_expected(sc, g, seed, k, ef, width, max_steps, seed_score=None)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    steps = torch.full((len(q),), -5, dtype=torch.int32, device=cuda)
    s, i = dense.graph_search_topk(t(q), t(docs), t(g), t(seed), None if seed_score is None else t(seed_score), k, ef, width, max_steps,
                                   steps=steps, workspace=workspace)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(i.cpu().numpy(), want[1])
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    np.testing.assert_array_equal(steps.cpu().numpy(), want[2])
    return want


#  nd, dim, degree, nq, nseed, k, ef, width, max_steps
SHAPES = {
    "dim4_degree4_ef1": (500, 4, 4, 3, 1, 1, 1, 1, None),
    "dim4_degree4_width512": (3000, 4, 4, 3, 32, 16, 16, 512, None),
    "dim36_degree64_k_below_ef": (700, 36, 64, 3, 32, 5, 16, 1, None),
    "dim36_degree64_width2": (700, 36, 64, 3, 32, 16, 16, 2, None),
    "dim36_degree64_width32": (2500, 36, 64, 1, 32, 100, 100, 32, None),
    "dim768_degree512_width4": (900, 768, 512, 3, 256, 100, 1000, 4, None),
    "dim768_degree64": (600, 768, 64, 3, 32, 10, 16, 1, None),
    "ef1000_k_is_ef": (5000, 32, 64, 3, 32, 1000, 1000, 1, None),
    "ef4096_k_is_ef": (9000, 32, 64, 1, 32, 4096, 4096, 2, None),
    "ef4096_k10": (9000, 32, 8, 3, 256, 10, 4096, 1, None),
    "max_steps_reached": (4000, 32, 64, 3, 32, 10, 64, 1, 3),
    "nq300": (2000, 36, 8, 300, 32, 10, 16, 1, None),
    "nq300_ef100": (2000, 36, 8, 300, 32, 10, 100, 1, None),         # past 256 queries the visited table is the small one
}


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("with_score", [True, False], ids=["seed_score", "scored"])
def test_walk_equals_the_reference(cuda, name, with_score):
    nd, dim, degree, nq, nseed, k, ef, width, max_steps = SHAPES[name]
    rng, docs, q, g, seed = _make(len(name), nd, dim, degree, nq, nseed)
    if nseed > 2:                                                      # a repeat, -1 and rows past the end among the seeds
        seed[:, 1] = seed[:, 0]
        seed[:, 2] = -1
        seed[0, nseed - 1] = nd
        seed[-1, nseed - 1] = nd + 12345
    want = _run(cuda, docs, q, g, seed, k, ef, width, max_steps, with_score)
    if max_steps is not None:
        assert (want[2] == max_steps).all()
    assert (want[2] > 0).all()


def test_duplicate_rows_tie_by_id_inside_the_list_and_at_the_eviction_boundary(cuda):
    """12 distinct rows among 800: every score is shared by ~66 ids, so a list of 16 or 40 entries ends inside a run of equal
    scores and the entry that stays is the one with the lower id."""
    rng, docs, q, g, seed = _make(77, 800, 36, 16, 4, 8, dup_rows=12)
    sc = gc.all_scores(q, docs)
    for k, ef, width in ((16, 16, 1), (7, 40, 3)):
        want = _run(cuda, docs, q, g, seed, k, ef, width, None, sc=sc)
        for n in range(len(q)):
            assert len(np.unique(want[0][n])) < k                      # ties inside the result
            last = want[0][n, k - 1]
            assert (sc[n] == last).sum() > (want[0][n] == last).sum()  # ... and the run continues past the boundary


def test_fewer_reachable_nodes_than_k(cuda):
    rng, docs, q, g, seed = _make(5, 400, 16, 8, 3, 4, holes=0.0)
    g[:10] = rng.integers(0, 10, size=(10, 8))                         # a closed component of 10 nodes
    seed[:] = rng.integers(0, 10, size=seed.shape)
    want = _run(cuda, docs, q, g, seed, 50, 64)
    assert (want[1][:, 10:] == -1).all() and (want[0][:, 10:] == -FLT_MAX).all() and (want[1][:, :3] >= 0).all()


def test_all_seeds_invalid_then_a_normal_call_on_the_same_workspace(cuda):
    rng, docs, q, g, seed = _make(6, 900, 36, 8, 3, 5)
    ws = torch.empty(dense.graph_search_workspace_bytes(3, 36, 8, 5, 10, 16, 1, 64), dtype=torch.uint8, device=cuda)
    bad = np.full_like(seed, -1)
    bad[:, 1] = 900
    bad[:, 2] = 2 ** 31 - 1
    for with_score in (True, False):
        want = _run(cuda, docs, q, g, bad, 10, 16, with_score=with_score, workspace=ws)
        assert (want[1] == -1).all() and (want[0] == -FLT_MAX).all() and (want[2] == 0).all()
        assert (ws[:12].view(torch.int32).cpu().numpy() == 0).all()    # rows scored
    want = _run(cuda, docs, q, g, seed, 10, 16, workspace=ws)
    assert (want[1] >= 0).all()


def test_rows_scored_are_counted_in_the_workspace(cuda):
    """The u32 per query the call leaves in its workspace: at least the rows an exact visited set scores (the table forgets, it
    never invents), at most the ids the steps read."""
    rng, docs, q, g, seed = _make(8, 3000, 32, 16, 5, 8)
    sc = gc.all_scores(q, docs)
    ws = torch.empty(dense.graph_search_workspace_bytes(5, 32, 16, 8, 10, 64, 1, 256), dtype=torch.uint8, device=cuda)
    want = _run(cuda, docs, q, g, seed, 10, 64, with_score=False, sc=sc, workspace=ws)
    exact = gc.search_expected(sc, g, seed, 10, 64, visited=True)
    got = ws[:20].view(torch.int32).cpu().numpy()
    assert (got >= exact[3]).all() and (got <= 8 + want[2].astype(np.int64) * 16).all()


def test_a_walk_that_scores_more_rows_than_the_visited_table_holds(cuda):
    """50 000 rows, a random graph of degree 64, ef 4096: the walk expands thousands of nodes and reads hundreds of thousands of
    ids, far more than any table in LDS remembers; the list is what decides."""
    rng = np.random.default_rng(50)
    nd, dim, nq = 50000, 32, 2
    docs = rng.standard_normal((nd, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    g = gc.random_graph(rng, nd, 64)
    seed = rng.integers(0, nd, size=(nq, 32)).astype(np.int32)
    sc = gc.all_scores(q, docs)
    want = _run(cuda, docs, q, g, seed, 100, 4096, 1, None, sc=sc)
    assert (want[2] >= 4096).all() and (want[3] > 16384).all()


def test_replayed_call_equals_eager(cuda):
    rng, docs, q, g, seed = _make(9, 2000, 36, 16, 3, 8)
    sc = gc.all_scores(q, docs)
    want = gc.search_expected(sc, g, seed, 10, 32)
    t = lambda a: torch.from_numpy(a).to(cuda)
    args = (t(q), t(docs), t(g), t(seed), None, 10, 32, 1, 128)
    out = (torch.empty((3, 10), dtype=torch.float32, device=cuda), torch.empty((3, 10), dtype=torch.int64, device=cuda))
    ws = torch.empty(dense.graph_search_workspace_bytes(3, 36, 16, 8, 10, 32, 1, 128), dtype=torch.uint8, device=cuda)
    dense.graph_search_topk(*args, out=out, workspace=ws)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dense.graph_search_topk(*args, out=out, workspace=ws)
    out[0].zero_()
    out[1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out[1].cpu().numpy(), want[1])
    np.testing.assert_array_equal(out[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32))


def test_refusals_arrive_before_a_launch(cuda):
    """With real buffers: a refused call leaves the outputs untouched and the device idle and healthy."""
    rng, docs, q, g, seed = _make(10, 500, 36, 8, 3, 4)
    t = lambda a: torch.from_numpy(a).to(cuda)
    tq, td, tg, ts = t(q), t(docs), t(g), t(seed)
    out = (torch.full((3, 10), 5.0, dtype=torch.float32, device=cuda), torch.full((3, 10), 5, dtype=torch.int64, device=cuda))
    for kw in (dict(k=10, ef=5), dict(k=10, ef=4097), dict(k=10, ef=16, width=300), dict(k=10, ef=16, max_steps=0),
               dict(k=10, ef=16, max_steps=70000)):
        with pytest.raises(hip.MeviHipError, match="graph_search"):
            dense.graph_search_topk(tq, td, tg, ts, None, kw["k"], kw["ef"], kw.get("width", 1), kw.get("max_steps", 64), out=out,
                                    workspace=torch.empty(256, dtype=torch.uint8, device=cuda))
    with pytest.raises(hip.MeviHipError, match="workspace"):
        dense.graph_search_topk(tq, td, tg, ts, None, 10, 16, 1, 64, out=out, workspace=torch.empty(0, dtype=torch.uint8, device=cuda))
    torch.cuda.synchronize()
    assert (out[0] == 5.0).all() and (out[1] == 5).all()
