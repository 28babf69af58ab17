"""Host side of the neighbour-graph index (mevi_amd/hnsw.py, include/mevi_hip_graph.h) without a GPU: the factory strings, the
header and its bindings, the sizing functions (monotone, 0 just outside every bound), every documented refusal before anything
is launched (the pointers handed over are null or fake), the routing envelope, and the references of the GPU tests
(tests/graph_cases.py) against their own definitions: visited-set independence, exactness at ef >= nd, the link invariants and
the recall the reference search reaches over the reference graph."""
import os
import re

import numpy as np
import pytest

import graph_cases as gc
from oracle import dense as odense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def test_parse_factory_table():
    from mevi_amd import hnsw, ivf, ivfpq

    table = {"HNSW256": 256, "HNSW32": 32, "HNSW8,Flat": 8, " HNSW16 , Flat ": 16, "HNSW2": 2, "HNSW1000": 1000}
    for text, want in table.items():
        assert hnsw.parse_factory(text) == want, text
    for text in ("HNSW", "HNSW32_PQ8", "HNSW32_SQ8", "HNSW32_Flat", "HNSW32,PQ8", "HNSW32,SQ8", "HNSW32_2x8", "IVF100_HNSW32,Flat",
                 "IVF8,Flat", "Flat", "PQ8", "OPQ16,HNSW32", "HNSW32,Flat,RFlat", "HNSW-3", "HNSW3.5", "hnsw32", "HNSW32x", "NSG32", ""):
        assert hnsw.parse_factory(text) is None, text
    assert ivf.parse_factory("HNSW32,Flat") is None and ivfpq.parse_factory("HNSW32") is None


def test_header_is_included_exported_and_bound(L):
    from mevi_amd import dense, hip

    assert '#include "mevi_hip_graph.h"' in open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    raw = open(os.path.join(ROOT, "include", "mevi_hip_graph.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mevi_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["mevi_graph_link", "mevi_graph_link_workspace_bytes", "mevi_graph_search_topk_f32",
                        "mevi_graph_search_workspace_bytes"]
    assert hip.exported_symbols("mevi_hip_graph.h") == declared and not set(declared) & set(hip.exported_symbols())
    assert all(callable(getattr(L, n)) for n in declared)
    for name, value in (("MEVI_GRAPH_MAX_EF", dense.GRAPH_MAX_EF), ("MEVI_GRAPH_MAX_BATCH", dense.GRAPH_MAX_BATCH),
                        ("MEVI_GRAPH_LINK_MIN_ROWS", dense.GRAPH_LINK_MIN_ROWS)):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == value
    for name in ("graph_link", "graph_link_workspace_bytes", "graph_search_topk", "graph_search_workspace_bytes"):
        assert callable(getattr(dense, name))
    # the header states the property the kernel's lossy visited table rests on, and what the index is not
    assert "does NOT depend on whether a node is scored more than once" in raw and "shrink_neighbor_list" in raw


#        nq, dim, degree, nseed, k, ef, width, max_steps
INSIDE = (8, 32, 64, 32, 10, 16, 1, 64)


def test_search_size_is_host_arithmetic_monotone_and_zero_just_outside(L):
    f = L.mevi_graph_search_workspace_bytes
    assert f(*INSIDE) > 0
    grids = {0: [1, 2, 63, 64, 65, 300, 6980, 1 << 20], 1: [4, 36, 768, 4096], 2: [4, 8, 64, 512], 3: [1, 32, 256], 4: [1, 10, 16],
             5: [16, 17, 1000, 4096], 6: [1, 2, 32], 7: [1, 64, 65536]}
    for axis, values in grids.items():
        sizes = []
        for v in values:
            shape = list(INSIDE)
            shape[axis] = v
            sizes.append(f(*shape))
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (axis, sizes)
    edges = {"nq 0": (0, 32, 64, 32, 10, 16, 1, 64), "dim 0": (8, 0, 64, 32, 10, 16, 1, 64), "dim 34": (8, 34, 64, 32, 10, 16, 1, 64),
             "degree 0": (8, 32, 0, 32, 10, 16, 1, 64), "degree 2": (8, 32, 2, 32, 10, 16, 1, 64), "degree 6": (8, 32, 6, 32, 10, 16, 1, 64),
             "degree 516": (8, 32, 516, 32, 10, 16, 1, 64), "nseed 0": (8, 32, 64, 0, 10, 16, 1, 64),
             "nseed 257": (8, 32, 64, 257, 10, 16, 1, 64), "k 0": (8, 32, 64, 32, 0, 16, 1, 64), "k > ef": (8, 32, 64, 32, 17, 16, 1, 64),
             "ef 4097": (8, 32, 64, 32, 10, 4097, 1, 64), "width 0": (8, 32, 64, 32, 10, 16, 0, 64),
             "width * degree": (8, 32, 64, 32, 10, 16, 33, 64), "max_steps 0": (8, 32, 64, 32, 10, 16, 1, 0),
             "max_steps 65537": (8, 32, 64, 32, 10, 16, 1, 65537)}
    for name, shape in edges.items():
        assert f(*shape) == 0, name
    for shape in [(1, 4, 4, 1, 1, 1, 1, 1), (1 << 20, 4096, 512, 256, 4096, 4096, 4, 65536), (8, 32, 64, 32, 16, 16, 32, 64),
                  (8, 32, 4, 32, 16, 16, 512, 64)]:
        assert f(*shape) > 0, shape


def test_link_size_is_host_arithmetic_monotone_and_zero_just_outside(L):
    from mevi_amd import dense

    f = L.mevi_graph_link_workspace_bytes
    assert f(100, 17, 16) == 100 * 32 * 8 + (-100 * 32 * 8) % 256
    assert f(8841823, 257, 256) == dense.GRAPH_LINK_MIN_ROWS * 512 * 8 <= dense.IVF_WORKSPACE_CAP      # C2 size, M = 256
    for axis, values in {0: [1, 2, 4095, 4096, 4097, 8841823, (1 << 31) - 1], 2: [1, 2, 16, 255, 256]}.items():
        sizes = []
        for v in values:
            shape = [5000, 17, 16]
            shape[axis] = v
            sizes.append(f(*shape))
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (axis, sizes)
    assert len({f(5000, c, 16) for c in (1, 16, 17, 4096)}) == 1
    for name, shape in {"nd 0": (0, 17, 16), "nd 2^31": (1 << 31, 17, 16), "C 0": (5000, 0, 16), "C 4097": (5000, 4097, 16),
                        "M 0": (5000, 17, 0), "M 257": (5000, 17, 257)}.items():
        assert f(*shape) == 0, name


def test_refusals_come_before_any_launch(L):
    from mevi_amd import hip

    A = 1 << 20                                    # a fake, well-aligned device address: nothing may dereference it

    def call(q=A, nq=8, dim=32, docs=A, nd=5000, graph=A, degree=64, seed=A, score=A, nseed=32, k=10, ef=16, width=1, steps=64,
             out_s=A, out_i=A, out_steps=A, ws=A, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.mevi_graph_search_workspace_bytes(nq, dim, degree, nseed, k, ef, width, steps)
        st = L.mevi_graph_search_topk_f32(q, nq, dim, docs, nd, graph, degree, seed, score, nseed, k, ef, width, steps, out_s, out_i,
                                          out_steps, ws, ws_bytes, None)
        return st, L.mevi_last_error().decode()

    def refused(code, word, **kw):
        st, msg = call(**kw)
        assert st == code and word in msg and msg.startswith("graph_search:"), (kw, st, msg)
        with pytest.raises(hip.MeviHipError, match="graph_search"):
            hip.check(st, "mevi_graph_search_topk_f32")

    refused(UNSUPPORTED, "dim=34", dim=34)
    refused(UNSUPPORTED, "dim=0", dim=0)
    refused(UNSUPPORTED, "degree=2", degree=2)
    refused(UNSUPPORTED, "degree=6", degree=6)
    refused(UNSUPPORTED, "degree=516", degree=516)
    refused(UNSUPPORTED, "ef=0", ef=0, k=0)
    refused(UNSUPPORTED, "ef=4097", ef=4097)
    refused(UNSUPPORTED, "k=0", k=0)
    refused(UNSUPPORTED, "k=17", k=17)
    refused(UNSUPPORTED, "nseed=0", nseed=0)
    refused(UNSUPPORTED, "nseed=257", nseed=257)
    refused(UNSUPPORTED, "width=0", width=0)
    refused(UNSUPPORTED, "width=33", width=33)
    refused(UNSUPPORTED, "max_steps=0", steps=0)
    refused(UNSUPPORTED, "max_steps=65537", steps=65537)
    refused(UNSUPPORTED, "31 bits", nd=1 << 31)
    for name in ("q", "docs", "graph", "seed", "out_s", "out_i", "ws"):
        refused(INVALID, "null", **{name: None})
    for name, step in (("q", 8), ("docs", 4), ("graph", 2), ("seed", 2), ("score", 2), ("out_s", 2), ("out_i", 4), ("out_steps", 2),
                       ("ws", 128)):
        refused(INVALID, "align", **{name: A + step})
    refused(INVALID, "nq=-1", nq=-1, ws_bytes=0)
    refused(INVALID, "nd=-1", nd=-1)
    need = L.mevi_graph_search_workspace_bytes(8, 32, 64, 32, 10, 16, 1, 64)
    refused(WORKSPACE, str(need), ws_bytes=need - 1)
    refused(WORKSPACE, str(need), ws_bytes=0)
    assert call(nq=0, q=None, ws=None, ws_bytes=0, score=None, out_steps=None)[0] == 0      # no queries: nothing to do

    def link(knn=A, nd=5000, C=17, M=16, graph=A, ws=A, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.mevi_graph_link_workspace_bytes(nd, C, M)
        return L.mevi_graph_link(knn, nd, C, M, graph, ws, ws_bytes, None), L.mevi_last_error().decode()

    for code, word, kw in ((UNSUPPORTED, "M=0", dict(M=0)), (UNSUPPORTED, "M=257", dict(M=257)), (UNSUPPORTED, "C=0", dict(C=0)),
                           (UNSUPPORTED, "C=4097", dict(C=4097)), (UNSUPPORTED, "31 bits", dict(nd=1 << 31)),
                           (INVALID, "nd=-1", dict(nd=-1)), (INVALID, "null", dict(knn=None)), (INVALID, "null", dict(graph=None)),
                           (INVALID, "null", dict(ws=None)), (INVALID, "align", dict(knn=A + 4)), (INVALID, "align", dict(graph=A + 2)),
                           (INVALID, "align", dict(ws=A + 128)),
                           (WORKSPACE, str(L.mevi_graph_link_workspace_bytes(5000, 17, 16)), dict(ws_bytes=4096 * 32 * 8 - 1))):
        st, msg = link(**kw)
        assert st == code and word in msg and msg.startswith("graph_link:"), (kw, st, msg)
    assert link(nd=0, knn=None, graph=None, ws=None, ws_bytes=0)[0] == 0


def test_routing_envelope_of_dense_search(L, monkeypatch):
    """`hnsw.wanted`: which (string, shape) pairs dense.search serves with the index; the others keep the exact search."""
    from mevi_amd import hnsw

    monkeypatch.delenv("MEVI_HNSW", raising=False)
    assert hnsw.wanted("HNSW256", 8841823, 768, 1000) == 256 and hnsw.wanted("HNSW32,Flat", 8841823, 768, 10) == 32
    assert hnsw.wanted("HNSW8", 1024, 32, 100) == 8 and hnsw.wanted("HNSW8", 1023, 32, 100) is None        # nd >= 64 * 2M
    assert hnsw.wanted("HNSW256", 2600, 32, 100) is None                # the end-to-end test's shape: exact lists
    assert hnsw.wanted("HNSW256", 32768, 32, 100) == 256 and hnsw.wanted("HNSW256", 32767, 32, 100) is None
    assert hnsw.wanted("HNSW32", 100000, 34, 10) is None                # dim % 4 != 0
    assert hnsw.wanted("HNSW32", 100000, 32, 4096) == 32 and hnsw.wanted("HNSW32", 100000, 32, 4097) is None
    assert hnsw.wanted("HNSW1", 100000, 32, 10) is None and hnsw.wanted("HNSW2", 100000, 32, 10) == 2
    assert hnsw.wanted("HNSW257", 10 ** 6, 32, 10) is None
    for text in ("HNSW32_PQ8", "HNSW32,SQ8", "IVF100_HNSW32,Flat", "IVF8,Flat", "Flat", "PQ8"):
        assert hnsw.wanted(text, 100000, 32, 10) is None, text
    monkeypatch.setenv("MEVI_HNSW", "exact")
    assert hnsw.wanted("HNSW32", 100000, 32, 10) is None
    monkeypatch.delenv("MEVI_HNSW")
    monkeypatch.setenv("MEVI_HNSW_EFSEARCH", "64")
    monkeypatch.setenv("MEVI_HNSW_WIDTH", "100")
    assert hnsw.default_ef_search() == 64 and hnsw.default_width(32) == 32 and hnsw.default_width(256) == 4


def test_all_scores_are_pair_dot_bit_for_bit():
    """The scores of the reference (one ip_topk_exact call, scattered back by id) are the pinned chain of oracle.dense.pair_dot,
    with a zero row, a repeated row and a ragged last slab."""
    rng = np.random.default_rng(3)
    for nd, dim in ((50, 36), (9, 4), (20, 768)):
        docs = rng.standard_normal((nd, dim)).astype(np.float32)
        docs[3] = 0.0
        docs[5] = docs[1]
        q = rng.standard_normal((3, dim)).astype(np.float32)
        s = gc.all_scores(q, docs)
        for i in range(3):
            want = odense.pair_dot(q[i], docs) + np.float32(0.0)
            assert np.array_equal(s[i].view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), (nd, dim, i)


def test_search_expected_does_not_depend_on_a_visited_set():
    """The property the header states: scoring a node again cannot change L, so the reference with an exact visited set and the
    one without give identical output -- on graphs with holes, self loops and repeats, at every width, with small and large ef."""
    rng = np.random.default_rng(11)
    nd, dim, nq = 600, 16, 6
    docs = gc.clustered(rng, nd, dim, 8)
    docs[100:110] = docs[90:100]                                       # duplicate rows: ties by id
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    sc = gc.all_scores(q, docs)
    rescored = 0
    for degree, ef, k, width, steps in ((8, 16, 10, 1, None), (8, 64, 64, 2, None), (16, 5, 3, 3, 2), (4, 300, 100, 4, None), (8, 1, 1, 1, None)):
        g = gc.random_graph(rng, nd, degree, holes=0.2)
        g[::7, 0] = np.arange(nd)[::7]                                 # self loops
        g[::5, 1] = g[::5, 2]                                          # repeats inside a row
        seed = rng.integers(-2, nd + 3, size=(nq, 5)).astype(np.int32)
        a = gc.search_expected(sc, g, seed, k, ef, width, steps, visited=False)
        b = gc.search_expected(sc, g, seed, k, ef, width, steps, visited=True)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert (a[3] >= b[3]).all()
        rescored += int((a[3] - b[3]).sum())
        if steps is not None:
            assert (a[2] <= steps).all() and (a[2] == steps).any()
    assert rescored > 0                                                # the two references did differ in what they scored


def test_search_expected_is_exact_when_the_list_holds_every_row():
    """ef >= nd on a graph whose every node is reachable from the seeds (a ring plus random links): nothing is ever evicted, so
    the result is the oracle's exact top-k."""
    rng = np.random.default_rng(5)
    nd, dim, nq, k = 300, 12, 4, 40
    docs = rng.standard_normal((nd, dim)).astype(np.float32)
    docs[7] = docs[3]
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    g = gc.random_graph(rng, nd, 4)
    g[:, 0] = (np.arange(nd) + 1) % nd
    seed = rng.integers(0, nd, size=(nq, 2)).astype(np.int32)
    sc = gc.all_scores(q, docs)
    want_s, want_i = odense.ip_topk_exact(q, docs, k)
    for width in (1, 3):
        s, i, steps, rows = gc.search_expected(sc, g, seed, k, nd + 5, width, 4 * nd)
        assert np.array_equal(s.view(np.uint32), (want_s + np.float32(0.0)).view(np.uint32)) and np.array_equal(i, want_i)
        assert (steps <= nd).all()


def test_link_expected_invariants():
    rng = np.random.default_rng(2)
    nd, C, M = 200, 12, 6
    knn = rng.integers(-1, nd, size=(nd, C))
    knn[:, 0] = np.arange(nd)                                          # the row itself comes first, as a search returns it
    knn[::3, 4] = knn[::3, 2]                                          # repeats
    knn[1:, 1] = 0                                                     # a hub
    g = gc.link_expected(knn, M)
    fwd = gc.forward_links(knn, M)
    assert g.shape == (nd, 2 * M) and g.dtype == np.int32
    for v in range(nd):
        row = g[v][g[v] >= 0].tolist()
        assert g[v, :len(row)].tolist() == row                         # -1 only at the end
        assert row[:len(fwd[v])] == fwd[v] and v not in row and len(set(row)) == len(row)
        rev = row[len(fwd[v]):]
        ranks = [(fwd[u].index(v), u) for u in rev]                    # every reverse link names v as a forward neighbour
        assert ranks == sorted(ranks)
        every = sorted((fwd[u].index(v), u) for u in range(nd) if v in fwd[u] and u not in fwd[v])
        assert ranks == every[:2 * M - len(fwd[v])]
    assert (g[0] >= 0).all() and g[0, M:].tolist() == [u for u in range(1, nd) if u not in fwd[0]][:M]      # the hub: rank 0, lowest rows
    short = gc.link_expected(knn[:, :4], M)                            # C < M: fewer forward links, reverse links follow them at once
    for v in range(nd):
        f = gc.forward_links(knn[:, :4], M)[v]
        assert len(f) <= 3 and short[v, :len(f)].tolist() == f


def test_reference_search_over_reference_graph_recall():
    """The recall condition: a fixed-seed clustered corpus (3000 x 32, 48 clusters), M = 16, k = 10, efSearch = 64, 4096 entry
    rows (all of them here), 32 seeds: the REFERENCE search over the REFERENCE graph reaches recall@10 >= 0.90.  Measured here:
    recall@10 1.0000, 61.1 steps on average (printed).  The device equals the reference bit for bit (tests/test_hnsw_index_gpu.py), so this bounds the device."""
    rng = np.random.default_rng(1234)
    nd, dim, M, k, ef, nq = 3000, 32, 16, 10, 64, 50
    docs = gc.clustered(rng, nd, dim, 48)
    q = (docs[rng.integers(0, nd, nq)] + 0.3 * rng.standard_normal((nq, dim))).astype(np.float32)
    knn = odense.ip_topk_exact(docs, docs, M + 1)[1]
    g = gc.link_expected(knn, M)
    sc = gc.all_scores(q, docs)
    seed, seed_score = gc.seeds_expected(sc, 32)
    s, i, steps, rows = gc.search_expected(sc, g, seed, k, ef, 1, 4 * ef, seed_score=seed_score)
    exact = odense.ip_topk_exact(q, docs, k)[1]
    recall = np.mean([len(set(i[n].tolist()) & set(exact[n].tolist())) / k for n in range(nq)])
    print(f"recall@10 {recall:.4f}, steps mean {steps.mean():.1f} max {steps.max()}, rows scored mean {rows.mean():.0f}")
    assert recall >= 0.90
    assert (i[:, 0] == exact[:, 0]).all()                              # nd <= ENTRY_ROWS: the best row is a seed and is never evicted
