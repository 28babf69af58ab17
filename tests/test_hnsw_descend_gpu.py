"""mevi_graph_descend_f32 (csrc/graph_descend.hip) against tests/graph_level_cases.py: descend_expected, the header restated in
Python over oracle scores, on random graphs with holes and RANDOM consistent maps (repeats, no order, entries outside their
range).  Bar: bit equality -- seeds, scores as uint32, steps."""
import numpy as np
import pytest
import torch

import graph_cases as gc
import graph_level_cases as glc
from mevi_amd import dense, hip

pytestmark = pytest.mark.gpu
FLT_MAX = np.finfo(np.float32).max


def _make(seed, nd, dim, degree, sizes, nq, nseed_in, holes=0.1, bad=0.05, dup_rows=0):
    rng = np.random.default_rng(seed)
    docs = rng.standard_normal((nd, dim)).astype(np.float32)
    if dup_rows:                                                       # only `dup_rows` distinct rows: ties everywhere
        docs = docs[rng.integers(0, dup_rows, nd)]
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    graphs, rows, down = glc.random_levels(rng, nd, sizes, degree, holes, bad)
    top = rng.integers(0, sizes[-1], size=(nq, nseed_in)).astype(np.int64)
    return rng, docs, q, graphs, rows, down, top


def _top_score(sc, rows, top, nd):
    """The chain's score where the seed is a node of the last level that is no hole, junk elsewhere."""
    r = rows[-1].astype(np.int64)
    ok = (top >= 0) & (top < len(r))
    row = r[np.clip(top, 0, len(r) - 1)]
    ok &= (row >= 0) & (row < nd)
    return np.where(ok, np.take_along_axis(sc, np.clip(row, 0, nd - 1), axis=1), np.float32(7e30)).astype(np.float32)


def _run(cuda, docs, q, graphs, rows, down, top, ef, width=1, max_steps=None, nseed_out=None, sc=None, workspace=None):
    sc = gc.all_scores(q, docs) if sc is None else sc
    nd = len(docs)
    score = _top_score(sc, rows, top, nd)
    want = glc.descend_expected(sc, nd, graphs, rows, down, top, score, ef, width, max_steps, nseed_out)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    steps = torch.full((len(q),), -5, dtype=torch.int32, device=cuda)
    i, s = dense.graph_descend(t(q), t(docs), t(np.concatenate(graphs)), t(np.concatenate(rows)), t(np.concatenate(down)),
                               [len(r) for r in rows], t(top), t(score), ef, width, max_steps, nseed_out, steps=steps, workspace=workspace)
    torch.cuda.synchronize()
    assert i.dtype == torch.int32 and s.dtype == torch.float32 and i.shape == want[0].shape
    np.testing.assert_array_equal(i.cpu().numpy(), want[0])
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    np.testing.assert_array_equal(steps.cpu().numpy(), want[2])
    return want


#  nd, dim, degree, level sizes (level 1 first), nq, nseed_in, ef, width, max_steps, nseed_out
SHAPES = {
    "dim4_degree4_one_level_ef1": (500, 4, 4, [200], 3, 1, 1, 1, None, 1),
    "dim4_degree4_width512": (3000, 4, 4, [2500, 600], 3, 32, 16, 512, None, 16),
    "dim36_degree64_two_levels": (2000, 36, 64, [700, 150], 3, 32, 8, 1, None, 8),
    "dim36_degree64_width2": (2000, 36, 64, [700, 150], 3, 32, 32, 2, None, 32),
    "dim36_degree64_width32": (3000, 36, 64, [2500, 300], 1, 32, 32, 32, None, 32),
    "dim768_degree512_width4_ef256": (900, 768, 512, [800, 300], 2, 256, 256, 4, None, 32),
    "dim768_degree64": (600, 768, 64, [500, 90], 3, 32, 16, 1, None, 16),
    "eight_levels": (3000, 36, 8, [1500, 900, 500, 300, 200, 100, 50, 20], 3, 8, 8, 1, None, 4),
    "ef256_out1": (2000, 32, 8, [1500, 400], 2, 64, 256, 1, None, 1),
    "a_level_of_one_node": (1000, 36, 8, [400, 1, 50], 3, 8, 8, 1, None, 8),
    "the_last_level_is_one_node": (1000, 36, 8, [400, 1], 3, 8, 8, 1, None, 8),
    "max_steps_1": (2000, 32, 16, [1500, 400], 3, 32, 16, 1, 1, 16),
    "nq300": (2000, 36, 8, [600, 100], 300, 32, 8, 1, None, 8),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_descent_equals_the_reference(cuda, name):
    nd, dim, degree, sizes, nq, nseed_in, ef, width, max_steps, nseed_out = SHAPES[name]
    bad = 0.0 if min(sizes) == 1 else 0.05                             # a level of one node that is a hole ends every descent
    rng, docs, q, graphs, rows, down, top = _make(len(name), nd, dim, degree, sizes, nq, nseed_in, bad=bad)
    if nseed_in > 2:                                                   # a repeat, -1 and nodes past the level's end among the seeds
        top[:, 1] = top[:, 0]
        top[:, 2] = -1
        top[0, nseed_in - 1] = sizes[-1]
        top[-1, nseed_in - 1] = 2 ** 40 + 5                            # an i64 whose low 32 bits would name a node
    want = _run(cuda, docs, q, graphs, rows, down, top, ef, width, max_steps, nseed_out)
    if max_steps is not None:
        assert (want[2] == max_steps * len(sizes)).all()
    assert (want[2] >= len(sizes)).any() and (want[0][:, 0] >= 0).any()


def test_maps_and_rows_out_of_range_are_holes_and_drops(cuda):
    """A third of every level's `down` and a third of its `rows` lie outside their ranges, some by a wide margin: the descent still
    equals the reference, and every query loses seeds on the way (fewer than nseed_out come out)."""
    rng, docs, q, graphs, rows, down, top = _make(31, 1500, 36, 16, [900, 300, 80], 6, 16, holes=0.3, bad=0.33)
    for a in rows + down:
        a[::17] = 2 ** 31 - 1
        a[5::19] = -2 ** 31
    want = _run(cuda, docs, q, graphs, rows, down, top, 16, 2, None, 16)
    assert (want[0] == -1).any() and (want[0] >= 0).any()
    assert ((want[0] == -1) == (want[1] == -FLT_MAX)).all()


def test_nseed_out_above_the_nodes_a_level_reaches_is_padded(cuda):
    rng, docs, q, graphs, rows, down, top = _make(5, 400, 16, 8, [300, 60], 3, 4, holes=0.0, bad=0.0)
    graphs[0][:10] = rng.integers(0, 10, size=(10, 8))                 # level 1: a closed component of 10 nodes ...
    down[1][:] = rng.integers(0, 10, size=60)                          # ... which is all that level 2 leads to
    rows[1][:] = rows[0][down[1]]
    want = _run(cuda, docs, q, graphs, rows, down, top, 64, 1, None, 32)
    assert (want[0][:, 10:] == -1).all() and (want[1][:, 10:] == -FLT_MAX).all() and (want[0][:, :3] >= 0).all()


def test_all_seeds_invalid_then_a_normal_call_on_the_same_workspace(cuda):
    rng, docs, q, graphs, rows, down, top = _make(6, 900, 36, 8, [500, 120], 3, 5)
    ws = torch.empty(dense.graph_descend_workspace_bytes(3, 36, 8, 2, 5, 8, 16, 1, 64), dtype=torch.uint8, device=cuda)
    bad = np.full_like(top, -1)
    bad[:, 1] = 120
    bad[:, 2] = 2 ** 31 - 1
    bad[:, 3] = -2 ** 33
    want = _run(cuda, docs, q, graphs, rows, down, bad, 16, 1, None, 8, workspace=ws)
    assert (want[0] == -1).all() and (want[1] == -FLT_MAX).all() and (want[2] == 0).all()
    assert (ws[:12].view(torch.int32).cpu().numpy() == 0).all()        # rows scored
    want = _run(cuda, docs, q, graphs, rows, down, top, 16, 1, None, 8, workspace=ws)
    assert (want[0] >= 0).any()


def test_duplicate_rows_tie_by_local_id_at_the_eviction_boundary(cuda):
    """12 distinct rows among 800: every score is shared by dozens of nodes, so a list of 16 entries ends inside a run of equal
    scores and the node that stays -- and goes down -- is the one with the lower LOCAL id, whatever its row."""
    rng, docs, q, graphs, rows, down, top = _make(77, 800, 36, 16, [600, 200], 4, 8, dup_rows=12, bad=0.0)
    sc = gc.all_scores(q, docs)
    for ef, width, nseed_out in ((16, 1, 16), (40, 3, 7)):
        want = _run(cuda, docs, q, graphs, rows, down, top, ef, width, None, nseed_out, sc=sc)
        for n in range(len(q)):
            assert len(np.unique(want[1][n])) < nseed_out              # ties inside the result
            last = want[1][n, nseed_out - 1]
            assert (sc[n] == last).sum() > (want[1][n] == last).sum()  # ... and the run continues past the boundary


def test_steps_and_rows_scored_are_counted(cuda):
    """out_steps is the sum over the levels; the u32 per query in the workspace counts the rows the descent scored, carried seeds
    excluded: at least the rows an exact visited set scores (the table forgets, it never invents), at most the ids the steps read."""
    rng, docs, q, graphs, rows, down, top = _make(8, 3000, 32, 16, [2000, 500], 5, 8)
    sc = gc.all_scores(q, docs)
    ws = torch.empty(dense.graph_descend_workspace_bytes(5, 32, 16, 2, 8, 16, 64, 1, 256), dtype=torch.uint8, device=cuda)
    want = _run(cuda, docs, q, graphs, rows, down, top, 64, 1, None, 16, sc=sc, workspace=ws)
    exact = glc.descend_expected(sc, 3000, graphs, rows, down, top, _top_score(sc, rows, top, 3000), 64, 1, None, 16, visited=True)
    got = ws[:20].view(torch.int32).cpu().numpy()
    assert np.array_equal(exact[0], want[0]) and np.array_equal(exact[2], want[2])
    assert (got >= exact[3]).all() and (got <= want[2].astype(np.int64) * 16).all() and (got > 0).all()
    assert (want[2] > 0).all() and (want[2] <= 2 * 256).all()


def test_output_seeds_the_level0_search(cuda):
    """The descent's output handed to mevi_graph_search_topk_f32 as seed / seed_score equals gc.search_expected with those
    seeds -- whose check that every seed score is the row's score holds the carried bits to the pinned chain."""
    rng, docs, q, graphs, rows, down, top = _make(12, 2500, 36, 16, [1200, 300], 4, 16)
    sc = gc.all_scores(q, docs)
    want = _run(cuda, docs, q, graphs, rows, down, top, 32, 1, None, 32, sc=sc)
    g0 = gc.random_graph(rng, 2500, 16, 0.1)
    walk = gc.search_expected(sc, g0, want[0], 10, 16, seed_score=want[1])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    tq, td = t(q), t(docs)
    i, s = dense.graph_descend(tq, td, t(np.concatenate(graphs)), t(np.concatenate(rows)), t(np.concatenate(down)), [1200, 300],
                               t(top), t(_top_score(sc, rows, top, 2500)), 32, 1, None, 32)
    out_s, out_i = dense.graph_search_topk(tq, td, t(g0), i, s, 10, 16)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out_i.cpu().numpy(), walk[1])
    np.testing.assert_array_equal(out_s.cpu().numpy().view(np.uint32), walk[0].view(np.uint32))


def test_refusals_arrive_before_a_launch(cuda):
    """With real buffers: a refused call leaves the outputs untouched and the device idle and healthy."""
    rng, docs, q, graphs, rows, down, top = _make(10, 500, 36, 8, [300, 60], 3, 4)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    args = (t(q), t(docs), t(np.concatenate(graphs)), t(np.concatenate(rows)), t(np.concatenate(down)))
    seed, score = t(top), torch.zeros((3, 4), dtype=torch.float32, device=cuda)
    out = (torch.full((3, 8), 5, dtype=torch.int32, device=cuda), torch.full((3, 8), 5.0, dtype=torch.float32, device=cuda))
    small = torch.empty(256, dtype=torch.uint8, device=cuda)
    for kw in (dict(ef=4), dict(ef=257), dict(width=300), dict(max_steps=0), dict(max_steps=70000)):
        with pytest.raises(hip.MeviHipError, match="graph_descend"):
            dense.graph_descend(*args, [300, 60], seed, score, kw.get("ef", 16), kw.get("width", 1), kw.get("max_steps", 64), 8, out=out,
                                workspace=small)
    with pytest.raises(hip.MeviHipError, match="workspace"):
        dense.graph_descend(*args, [300, 60], seed, score, 16, 1, 64, 8, out=out, workspace=torch.empty(0, dtype=torch.uint8, device=cuda))
    torch.cuda.synchronize()
    assert (out[0] == 5).all() and (out[1] == 5.0).all()
