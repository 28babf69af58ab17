"""Host side of the upper levels of the neighbour-graph index (mevi_amd/hnsw.py, include/mevi_hip_graph_levels.h) without a GPU:
the header and its bindings, the sizing function (monotone, 0 just outside every bound), every documented refusal before
anything is launched (the device pointers handed over are null or fake), the level arithmetic and its fallbacks, the
environment, and the recall condition on the references of the GPU tests alone (tests/graph_level_cases.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import graph_cases as gc
import graph_level_cases as glc
from oracle import dense as odense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def test_header_is_included_exported_and_bound(L):
    from mevi_amd import dense, hip

    assert '#include "mevi_hip_graph_levels.h"' in open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    raw = open(os.path.join(ROOT, "include", "mevi_hip_graph_levels.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mevi_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["mevi_graph_descend_f32", "mevi_graph_descend_workspace_bytes"]
    assert hip.exported_symbols("mevi_hip_graph_levels.h") == declared
    assert not set(declared) & set(hip.exported_symbols()) and not set(declared) & set(hip.exported_symbols("mevi_hip_graph.h"))
    assert all(callable(getattr(L, n)) for n in declared)
    for name, value in (("MEVI_GRAPH_MAX_LEVELS", dense.GRAPH_MAX_LEVELS), ("MEVI_GRAPH_DESCEND_MAX_EF", dense.GRAPH_DESCEND_MAX_EF)):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == value
    assert callable(dense.graph_descend) and callable(dense.graph_descend_workspace_bytes)
    # the header pins what the carried scores rest on, and what the levels are not
    assert "LOCAL id ascending" in raw and "never scored again" in raw and "random levels" in raw


#        nq, dim, degree, n_levels, nseed_in, nseed_out, ef, width, max_steps
INSIDE = (8, 32, 64, 2, 32, 32, 32, 1, 128)


def test_size_is_host_arithmetic_monotone_and_zero_just_outside(L):
    f = L.mevi_graph_descend_workspace_bytes
    assert f(*INSIDE) == 256 and f(300, 32, 64, 2, 32, 32, 32, 1, 128) == 1280
    grids = {0: [1, 2, 63, 64, 65, 300, 6980, 1 << 20], 1: [4, 36, 768, 4096], 2: [4, 8, 64, 512], 3: [1, 2, 8], 4: [1, 32, 256],
             5: [1, 8, 32], 6: [32, 33, 256], 7: [1, 2, 32], 8: [1, 64, 65536]}
    for axis, values in grids.items():
        sizes = []
        for v in values:
            shape = list(INSIDE)
            shape[axis] = v
            sizes.append(f(*shape))
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (axis, sizes)

    def at(**kw):
        shape = dict(zip(("nq", "dim", "degree", "n_levels", "nseed_in", "nseed_out", "ef", "width", "max_steps"), INSIDE))
        shape.update(kw)
        return f(*shape.values())

    for kw in (dict(nq=0), dict(dim=0), dict(dim=34), dict(degree=0), dict(degree=2), dict(degree=6), dict(degree=516), dict(n_levels=0),
               dict(n_levels=9), dict(nseed_in=0), dict(nseed_in=257), dict(nseed_out=0), dict(nseed_out=33), dict(ef=0, nseed_out=0),
               dict(ef=257), dict(width=0), dict(width=33), dict(max_steps=0), dict(max_steps=65537)):
        assert at(**kw) == 0, kw
    for kw in (dict(nq=1, dim=4, degree=4, n_levels=1, nseed_in=1, nseed_out=1, ef=1, width=1, max_steps=1),
               dict(nq=1 << 20, dim=4096, degree=512, n_levels=8, nseed_in=256, nseed_out=256, ef=256, width=4, max_steps=65536),
               dict(width=32), dict(degree=4, width=512)):
        assert at(**kw) > 0, kw


def test_refusals_come_before_any_launch(L):
    from mevi_amd import hip

    A = 1 << 20                                    # a fake, well-aligned device address: nothing may dereference it
    sizes = (ctypes.c_int64 * 8)(5000, 1200, 300, 75, 20, 5, 2, 1)
    host = ctypes.addressof(sizes)

    def call(q=A, nq=8, dim=32, docs=A, nd=20000, graphs=A, degree=64, rows=A, down=A, level_n=host, n_levels=2, seed=A, score=A,
             nseed_in=32, ef=32, width=1, steps=128, nseed_out=32, out_i=A, out_s=A, out_steps=A, ws=A, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.mevi_graph_descend_workspace_bytes(nq, dim, degree, n_levels, nseed_in, nseed_out, ef, width, steps)
        st = L.mevi_graph_descend_f32(q, nq, dim, docs, nd, graphs, degree, rows, down, level_n, n_levels, seed, score, nseed_in, ef,
                                      width, steps, nseed_out, out_i, out_s, out_steps, ws, ws_bytes, None)
        return st, L.mevi_last_error().decode()

    def refused(code, word, **kw):
        st, msg = call(**kw)
        assert st == code and word in msg and msg.startswith("graph_descend:"), (kw, st, msg)
        with pytest.raises(hip.MeviHipError, match="graph_descend"):
            hip.check(st, "mevi_graph_descend_f32")

    refused(UNSUPPORTED, "dim=34", dim=34)
    refused(UNSUPPORTED, "dim=0", dim=0)
    refused(UNSUPPORTED, "degree=2", degree=2)
    refused(UNSUPPORTED, "degree=6", degree=6)
    refused(UNSUPPORTED, "degree=516", degree=516)
    refused(UNSUPPORTED, "n_levels=0", n_levels=0)
    refused(UNSUPPORTED, "n_levels=9", n_levels=9)
    refused(UNSUPPORTED, "nseed_in=0", nseed_in=0)
    refused(UNSUPPORTED, "nseed_in=257", nseed_in=257)
    refused(UNSUPPORTED, "ef=0", ef=0, nseed_out=0)
    refused(UNSUPPORTED, "ef=257", ef=257)
    refused(UNSUPPORTED, "nseed_out=0", nseed_out=0)
    refused(UNSUPPORTED, "nseed_out=33", nseed_out=33)
    refused(UNSUPPORTED, "width=0", width=0)
    refused(UNSUPPORTED, "width=33", width=33)
    refused(UNSUPPORTED, "max_steps=0", steps=0)
    refused(UNSUPPORTED, "max_steps=65537", steps=65537)
    refused(UNSUPPORTED, "31 bits", nd=1 << 31)
    for at, value in ((0, 0), (1, -3), (7, 1 << 31)):                   # every level's size is read, and only the first n_levels
        bad = (ctypes.c_int64 * 8)(*sizes)
        bad[at] = value
        refused(UNSUPPORTED, f"level_n[{at}]={value}", level_n=ctypes.addressof(bad), n_levels=8)
        if at >= 2:
            assert call(level_n=ctypes.addressof(bad), nq=0)[0] == 0
    for name in ("q", "docs", "graphs", "rows", "down", "level_n", "seed", "score", "out_i", "out_s", "ws"):
        refused(INVALID, "null", **{name: None})
    for name, step in (("q", 8), ("docs", 4), ("graphs", 2), ("rows", 2), ("down", 2), ("seed", 4), ("score", 2), ("out_i", 2), ("out_s", 2),
                       ("out_steps", 2), ("ws", 128)):
        refused(INVALID, "align", **{name: A + step})
    refused(INVALID, "nq=-1", nq=-1, ws_bytes=0)
    refused(INVALID, "nd=-1", nd=-1)
    need = L.mevi_graph_descend_workspace_bytes(8, 32, 64, 2, 32, 32, 32, 1, 128)
    refused(WORKSPACE, str(need), ws_bytes=need - 1)
    refused(WORKSPACE, str(need), ws_bytes=0)
    assert call(nq=0, q=None, ws=None, ws_bytes=0, out_steps=None)[0] == 0      # no queries: nothing to do
    assert call(nq=0, out_steps=None, nd=0, docs=None)[0] == 0


def test_level_sizes_maps_and_fallbacks():
    from mevi_amd import dense, hnsw

    assert hnsw.level_sizes(8841823, 32, 4096) == [8841823, 276306, 8634, 269] == glc.level_sizes(8841823, 32, 4096)
    assert hnsw.walked_levels(8841823, 32) == 2 == glc.walked_levels(8841823, 32)
    assert hnsw.level_sizes(6000, 4, 64) == [6000, 1500, 375, 93, 23] and hnsw.walked_levels(6000, 4, 64) == 3
    assert hnsw.level_sizes(20000, 4) == [20000, 5000, 1250] and hnsw.walked_levels(20000, 4) == 1
    # U = 0: level 1 is already within the entry rows, the strided rows are at least as dense
    assert hnsw.level_sizes(4096, 8) == [4096, 512] and hnsw.walked_levels(4096, 8) == 0
    assert hnsw.walked_levels(4096 * 8 + 7, 8) == 0 and hnsw.walked_levels(4097 * 8, 8) == 1
    assert hnsw.walked_levels(100, 4) == 0 and hnsw.walked_levels(3, 4) == 0
    # U > 8: 2 ** 20 rows halved down to 2 rows are 18 walked levels; 9 is the first count refused
    assert dense.GRAPH_MAX_LEVELS == 8
    assert len(hnsw.level_sizes(1 << 20, 2, 2)) - 2 == 18 and hnsw.walked_levels(1 << 20, 2, 2) == 0
    assert len(hnsw.level_sizes(1 << 20, 2, 1 << 10)) - 2 == 9 and hnsw.walked_levels(1 << 20, 2, 1 << 10) == 0
    assert hnsw.walked_levels(1 << 20, 2, 1 << 11) == 8
    # an empty top level (fewer nodes than M on the level before it) is no top level
    assert hnsw.level_sizes(7, 4, 1) == [7, 1] and hnsw.level_sizes(11, 4, 1) == [11, 2, 0] and hnsw.walked_levels(11, 4, 1) == 0
    for nd, M, limit in ((8841823, 32, 4096), (6000, 4, 64), (20000, 4, 4096), (1 << 20, 2, 1 << 11), (12345, 3, 10)):
        sizes = hnsw.level_sizes(nd, M, limit)
        assert sizes == glc.level_sizes(nd, M, limit)
        assert all(sizes[l] == sizes[l - 1] // M for l in range(1, len(sizes))) and sizes[-1] <= limit < sizes[-2]
        down, rows = hnsw.level_maps(sizes)
        wdown, wrows = glc.level_maps(sizes)
        for l in range(1, len(sizes)):
            d, r = down[l - 1].numpy(), rows[l - 1].numpy()
            assert np.array_equal(d, wdown[l - 1]) and np.array_equal(r, wrows[l - 1]) and len(d) == sizes[l]
            assert (np.diff(d) > 0).all() and (np.diff(r) > 0).all()    # strictly ascending: the order by local id is the order by row
            assert d[0] == 0 and d[-1] < sizes[l - 1] and r[-1] < nd and d.max() < 2 ** 31
            below = np.arange(nd) if l == 1 else rows[l - 2].numpy()
            assert np.array_equal(r, below[d])                          # nested: a node of level l is a node of level l - 1
    assert dense.graph_descend_workspace_bytes(1, 768, 64, 2, 32, 32, 32, 1, 128) > 0


def test_environment(monkeypatch):
    from mevi_amd import hnsw

    for name in ("MEVI_HNSW_ENTRY", "MEVI_HNSW_EF_UPPER", "MEVI_HNSW_WIDTH_UPPER"):
        monkeypatch.delenv(name, raising=False)
    assert hnsw.default_entry() == "strided" and hnsw.default_ef_upper() == hnsw.N_SEEDS == 32
    # the width's default is 4, not the level-0 walk's 1: measured at C2 size; degree 1024 would leave room for 2 only
    assert hnsw.default_width_upper(32) == hnsw.WIDTH_UPPER == 4 and hnsw.default_width_upper(256) == 4
    for text, want in (("levels", "levels"), (" Levels ", "levels"), ("strided", "strided"), ("", "strided")):
        monkeypatch.setenv("MEVI_HNSW_ENTRY", text)
        assert hnsw.default_entry() == want
    monkeypatch.setenv("MEVI_HNSW_ENTRY", "random")
    with pytest.raises(ValueError, match="MEVI_HNSW_ENTRY"):
        hnsw.default_entry()
    monkeypatch.setenv("MEVI_HNSW_EF_UPPER", "8")
    monkeypatch.setenv("MEVI_HNSW_WIDTH_UPPER", "100")
    assert hnsw.default_ef_upper() == 8 and hnsw.default_width_upper(32) == 32 and hnsw.default_width_upper(256) == 4
    monkeypatch.setenv("MEVI_HNSW_EF_UPPER", "1000")
    assert hnsw.default_ef_upper() == 256
    monkeypatch.setenv("MEVI_HNSW_EF_UPPER", "0")
    assert hnsw.default_ef_upper() == 1


def _reference_recall(seed, nd, n_clusters, M, limit, nseed, ef_upper, k=10, ef=16, nq=100):
    """(recall@k with the strided entry, with levels, rows scored per query of either) of the REFERENCE search over REFERENCE
    graphs, oracle scores throughout."""
    rng = np.random.default_rng(seed)
    docs = gc.clustered(rng, nd, 32, n_clusters)
    q = (docs[rng.integers(0, nd, nq)] + 0.1 * rng.standard_normal((nq, 32))).astype(np.float32)
    sc = gc.all_scores(q, docs)
    exact = odense.ip_topk_exact(q, docs, k)[1]
    g0 = gc.link_expected(odense.ip_topk_exact(docs, docs, M + 1)[1], M)

    def recall(ids):
        return float(np.mean([len(set(ids[n].tolist()) & set(exact[n].tolist())) / k for n in range(nq)]))

    seed0, score0 = gc.seeds_expected(sc, nseed, limit)
    strided = gc.search_expected(sc, g0, seed0, k, ef, 1, 4 * ef, seed_score=score0)
    sizes = glc.level_sizes(nd, M, limit)
    down, rows = glc.level_maps(sizes)
    U = len(sizes) - 2
    graphs = []
    for l in range(1, U + 1):
        level_docs = np.ascontiguousarray(docs[rows[l - 1]])
        graphs.append(gc.link_expected(odense.ip_topk_exact(level_docs, level_docs, min(M + 1, sizes[l]))[1], M))
    top, top_score = glc.top_seeds_expected(sc, rows[U], down[U], nseed)
    seed1, score1, steps, scored = glc.descend_expected(sc, nd, graphs, rows[:U], down[:U], top, top_score, ef_upper, 1, 4 * ef_upper,
                                                        min(nseed, ef_upper))
    levels = gc.search_expected(sc, g0, seed1, k, ef, 1, 4 * ef, seed_score=score1)
    rows_strided = len(gc.entry_rows(nd, limit)) + strided[3].mean() - seed0.shape[1]
    rows_levels = sizes[-1] + scored.mean() + levels[3].mean() - (seed1 >= 0).sum(1).mean()
    return recall(strided[1]), recall(levels[1]), rows_strided, rows_levels


def test_reference_descent_recall_on_an_island_corpus():
    """The recall condition, on the references alone: 6000 x 32 rows around 300 centres (gc.clustered, seed 0), M = 4, 64 entry
    rows, 8 seeds, upper ef 16, 100 queries (rows + 0.1 noise), k = 10, ef = 16.  The level-0 graph falls into per-cluster
    islands and 64 strided rows reach a fifth of the clusters; levels 1500 / 375 / 93 walked and 23 scanned reach them.
    Bar: levels recall@10 >= 0.7 and >= 2 x the strided recall@10.  Measured with the oracle's scores (printed): strided 0.2320,
    levels 0.9400 -- the values a float32-matmul prototype of the same walk gave, so seed 0 stays --, for 101 against 213 rows
    scored per query (entry scan, descent and walk; carried seeds not counted).
    The device equals these references bit for bit (tests/test_hnsw_levels_index_gpu.py), so this bounds the device."""
    strided, levels, rows_strided, rows_levels = _reference_recall(0, 6000, 300, 4, 64, 8, 16)
    print(f"recall@10 strided {strided:.4f} levels {levels:.4f}; rows scored per query strided {rows_strided:.0f} levels {rows_levels:.0f}")
    assert levels >= 0.7 and levels >= 2 * strided
