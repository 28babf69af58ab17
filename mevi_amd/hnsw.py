"""A neighbour-graph index behind `faiss_search.py --param HNSW<M>` (the reference README's own ANN command uses HNSW256).

faiss builds `IndexHNSWFlat(dim, M, METRIC_INNER_PRODUCT)`: M links per node on the upper levels, 2M on level 0, built by
sequential insertion (efConstruction 40) with random levels and diversity pruning, searched with a candidate list of
max(efSearch, k) entries (efSearch 16).  Its insertion order and RNG cannot be reproduced, so neither can its graph; what this
index keeps is HNSW's level-0 structure and its search, with the two serial parts replaced by brute force:
  * graph : i32 [nd, 2M].  Slots [0, M) of row v = v's M nearest other rows by exact inner product (one exact search of the rows
    against themselves, in chunks); the remaining slots = reverse links: the rows u that name v as their forward neighbour of
    rank r, outside v's own forward links, in ascending (r, u) order until the row is full (mevi_graph_link).  There is NO
    diversity pruning (faiss's shrink_neighbor_list).
  * entry : by default, instead of the upper levels' descent, ENTRY_ROWS = min(nd, 4096) rows at a fixed stride (row floor(i * nd / E)) are
    scored per query with mevi_ivf_scan_topk_f32 as one list; the best N_SEEDS = 32 seed the walk, scores included.
  * search: best-first over the graph with ef = max(efSearch, k) entries, `width` entries expanded per step, at most 4 * ef steps
    (mevi_graph_search_topk_f32, csrc/graph_search.hip; the semantics are pinned in include/mevi_hip_graph.h).
Every returned score is the exact search's score for that id, bit for bit; which ids are found is approximate.  Given the graph
and the seeds the result is defined exactly and tested bit for bit (tests/graph_cases.py).  `search` also runs the exact search
and reports recall on stderr.

`HNSWIndex.search` is two stream-ordered device calls (entry scan, walk; three with levels, below); nothing is copied to the host, so up to
GRAPH_MAX_QUERIES queries can be captured and replayed (`search_graph`).

Upper levels (opt-in: `HNSWIndex(..., entry="levels")` or MEVI_HNSW_ENTRY=levels; the default, "strided", is the entry scan
above and every result of it is unchanged).  The strided rows are the only way into the graph, and on a clustered corpus the
exact-kNN graph falls into per-cluster islands: a query whose cluster holds no entry row walks the wrong island however long
its list is.  With levels the seeds of the walk come from a hierarchy instead:
  * levels: n_0 = nd, n_l = n_{l-1} // M, up to the first level T with n_T <= entry_rows (`level_sizes`).  Membership is nested
    and arithmetic, not random: local id j of level l is local id (j * n_{l-1}) // n_l of level l - 1 (`down`), and `rows` is
    the composition down to the rows of the corpus.  Levels 1 .. U = T - 1 each get a graph i32 [n_l, 2M] in local ids, built
    by the same two calls as level 0 (exact kNN of the level's rows among themselves, mevi_graph_link): still no pruning.
  * search: the top level's rows are scanned exhaustively (the call that scans the strided rows, with `down` of level T as item
    ids), one kernel descends levels U .. 1 (mevi_graph_descend_f32, csrc/graph_descend.hip; semantics pinned in
    include/mevi_hip_graph_levels.h: per level the walk of level 0 with ef = MEVI_HNSW_EF_UPPER, the best N_SEEDS go down with
    their scores), and its output seeds the unchanged level-0 walk: three stream-ordered calls, replayable as before.
When U would be 0 (nd // M <= entry_rows: the strided rows are at least as dense as level 1) or above 8 the index is the
strided one; `index.entry` says which it is.

Environment: MEVI_HNSW_EFSEARCH (default 16), MEVI_HNSW_WIDTH (default 1), MEVI_HNSW_ENTRY (strided | levels, default strided),
MEVI_HNSW_EF_UPPER (default 32) and MEVI_HNSW_WIDTH_UPPER (default 4) for the upper levels' walks, MEVI_HNSW=exact answers the
string with the exact search, as before this index existed.
"""
import os
import re
import sys

import torch

from . import dense, hip, ivf

ENTRY_ROWS = 4096                 # rows scored per query in place of the upper levels
N_SEEDS = 32                      # ... the best of which seed the walk
GRAPH_MAX_QUERIES = ivf.GRAPH_MAX_QUERIES
KNN_CHUNK = 8192                  # rows per exact search while the kNN lists are built
MIN_ROWS_PER_DEGREE = 64          # `wanted`: nd >= 64 * 2M, below that the graph is close to complete and exact search wins
MAX_M = 256
ENTRIES = ("strided", "levels")   # how the level-0 walk finds its seeds
WIDTH_UPPER = 4                   # entries an upper level's walk expands per step: at C2 size faster than 1 at every batch and
                                  # list size, with equal or higher recall; the level-0 walk keeps 1


def parse_factory(param):
    """M of 'HNSW<M>' and 'HNSW<M>,Flat', else None: 'HNSW<M>_PQ8', 'HNSW<M>,SQ8', 'IVF..._HNSW32,...' keep the exact search."""
    g = re.fullmatch(r"\s*HNSW(\d+)\s*(?:,\s*Flat\s*)?", str(param))
    return int(g.group(1)) if g else None


def default_ef_search():
    return max(1, int(os.environ.get("MEVI_HNSW_EFSEARCH", "16")))


def default_width(M):
    return max(1, min(int(os.environ.get("MEVI_HNSW_WIDTH", "1")), dense.GRAPH_MAX_BATCH // (2 * M)))


def default_entry():
    """'strided' or 'levels' from MEVI_HNSW_ENTRY (unset or empty: 'strided'); any other value is an error."""
    entry = os.environ.get("MEVI_HNSW_ENTRY", "").strip().lower() or "strided"
    if entry not in ENTRIES:
        raise ValueError(f"MEVI_HNSW_ENTRY={entry!r}: expected one of {ENTRIES}")
    return entry


def default_ef_upper():
    return max(1, min(int(os.environ.get("MEVI_HNSW_EF_UPPER", str(N_SEEDS))), dense.GRAPH_DESCEND_MAX_EF))


def default_width_upper(M):
    return max(1, min(int(os.environ.get("MEVI_HNSW_WIDTH_UPPER", str(WIDTH_UPPER))), dense.GRAPH_MAX_BATCH // (2 * M)))


def level_sizes(nd, M, entry_rows=ENTRY_ROWS):
    """[n_0 .. n_T]: n_0 = nd, n_l = n_{l-1} // M, ending with the first level of at most `entry_rows` nodes (the top level T,
    scanned exhaustively; levels 1 .. T - 1 are walked)."""
    assert M >= 2
    sizes = [int(nd)]
    while True:
        sizes.append(sizes[-1] // M)
        if sizes[-1] <= entry_rows:
            return sizes


def walked_levels(nd, M, entry_rows=ENTRY_ROWS):
    """U = T - 1 when the index of this shape descends levels, else 0 (the strided index): U < 1 -- level 1 would already be
    the scanned one, and the strided rows are at least as dense --, U above the descent's limit, or an empty top level."""
    sizes = level_sizes(nd, M, entry_rows)
    U = len(sizes) - 2
    return U if 1 <= U <= dense.GRAPH_MAX_LEVELS and sizes[-1] >= 1 else 0


def level_maps(sizes, device="cpu"):
    """(down, rows): per level l = 1 .. T, down_l i64 [n_l] = local id on level l - 1, (j * n_{l-1}) // n_l, and rows_l i64 [n_l] =
    row of the corpus.  Both strictly ascending; entry l - 1 of each list is level l."""
    down, rows = [], []
    for l in range(1, len(sizes)):
        d = (torch.arange(sizes[l], dtype=torch.int64, device=device) * sizes[l - 1]) // max(sizes[l], 1)
        down.append(d)
        rows.append(d if l == 1 else rows[-1][d])
    return down, rows


def supported(nd, dim, topk, M):
    """True when an index of this shape is inside the envelope of the link and of the walk (host arithmetic)."""
    if not 2 <= M <= MAX_M or nd < 1 or topk < 1:
        return False
    return (dense.graph_link_workspace_bytes(nd, M + 1, M) > 0 and
            dense.graph_search_workspace_bytes(1, dim, 2 * M, min(N_SEEDS, nd), topk, max(topk, 1), 1, 4 * topk) > 0)


def wanted(param, nd, dim, topk):
    """M when `dense.search` / `dense.profile` serve `param` with an HNSWIndex: the string parses, dim % 4 == 0, 2 <= M <= 256,
    topk <= 4096, nd >= 64 * 2M (a graph of degree 2M over fewer rows is close to complete: exact search is faster and exact)
    and MEVI_HNSW is not 'exact'; else None."""
    M = parse_factory(param)
    if M is None or os.environ.get("MEVI_HNSW", "index") == "exact" or not 2 <= M <= MAX_M:
        return None
    if dim % 4 != 0 or topk > dense.GRAPH_MAX_EF or nd < MIN_ROWS_PER_DEGREE * 2 * M or not supported(nd, dim, topk, M):
        return None
    return M


def knn_lists(docs, C, chunk=KNN_CHUNK, index=None):
    """i64 [nd, C]: the exact top-C of every row against all rows (the row itself is usually first), `chunk` rows a search."""
    index = index or dense.DenseIndex(docs)
    nd = docs.shape[0]
    out = torch.empty((nd, C), dtype=torch.int64, device=docs.device)
    for a in range(0, nd, chunk):
        out[a:a + chunk] = index.search(docs[a:a + chunk], C)[1]
    return out


def entry_rows(nd, device, limit=ENTRY_ROWS):
    E = min(nd, limit)
    return (torch.arange(E, dtype=torch.int64, device=device) * nd) // max(E, 1)


strided_rows = entry_rows         # for HNSWIndex.__init__, whose `entry_rows` argument is the limit


class HNSWIndex:
    """`index.add(doc)` of 'HNSW<M>': kNN lists, links, entry rows.  `knn` / `graph` given: taken instead of built.
    `entry`: 'strided' or 'levels' (None: MEVI_HNSW_ENTRY); `self.entry` is what the index is -- 'strided' also when levels
    were asked for on a shape without walked levels (`walked_levels`).  `entry_rows`: the most rows the entry scan reads."""

    def __init__(self, docs, M, knn=None, graph=None, timing=None, entry=None, entry_rows=ENTRY_ROWS, ef_upper=None, width_upper=None):
        import time

        hip.require_gpu()
        assert docs.is_cuda and docs.dtype == torch.float32 and docs.dim() == 2
        self.docs = docs.contiguous()
        nd, dim = self.docs.shape
        self.M, self.dim, self.degree = M, dim, 2 * M
        entry = default_entry() if entry is None else entry
        if entry not in ENTRIES:
            raise ValueError(f"HNSWIndex: entry={entry!r}: expected one of {ENTRIES}")
        self.entry = "levels" if entry == "levels" and walked_levels(nd, M, entry_rows) else "strided"

        def lap(name, t0):
            if timing is not None:
                torch.cuda.synchronize()
                timing[name] = time.perf_counter() - t0
            return time.perf_counter()

        t = time.perf_counter()
        if graph is None:
            self.knn = knn_lists(self.docs, min(M + 1, nd)) if knn is None else knn.contiguous()
            t = lap("knn_s", t)
            self.graph = dense.graph_link(self.knn, M)
            t = lap("link_s", t)
        else:
            self.knn, self.graph = knn, graph.contiguous()
        self.level_n = [nd]
        if self.entry == "levels":
            t = self.build_levels(entry_rows, lap, t)
        else:
            self.entry_ids = self.top_rows = strided_rows(nd, docs.device, entry_rows)
        self.entry_docs = self.docs[self.top_rows].contiguous()      # the scan's one list; entry_ids are its item ids
        self.entry_offsets = torch.tensor([0, self.entry_ids.numel()], dtype=torch.int64, device=docs.device)
        self.nseed = min(N_SEEDS, self.entry_ids.numel())
        self.set_upper(ef_upper, width_upper)
        lap("entry_s", t)

    def build_levels(self, entry_rows, lap, t):
        """The walked levels' graphs and maps, and the top level as the entry scan's list: its item ids are `down` of level T,
        so the scan returns local ids of level U."""
        M, dev = self.M, self.docs.device
        self.level_n = level_sizes(self.docs.shape[0], M, entry_rows)
        down, rows = level_maps(self.level_n, dev)
        U = len(self.level_n) - 2
        self.level_knn, graphs = [], []
        for l in range(1, U + 1):
            level_docs = self.docs[rows[l - 1]].contiguous()           # a temporary: the descent gathers through `rows`
            self.level_knn.append(knn_lists(level_docs, min(M + 1, self.level_n[l])))
            graphs.append(dense.graph_link(self.level_knn[-1], M))
            del level_docs
        self.level_graphs = torch.cat(graphs).contiguous()
        self.level_rows = torch.cat(rows[:U]).to(torch.int32)
        self.level_down = torch.cat(down[:U]).to(torch.int32)
        self.entry_ids = down[U].contiguous()
        self.top_rows = rows[U]
        return lap("levels_s", t)

    def set_upper(self, ef_upper=None, width_upper=None):
        """The upper levels' walks: list size (None: MEVI_HNSW_EF_UPPER), width (None: MEVI_HNSW_WIDTH_UPPER), 4 * ef steps per
        level; the best min(N_SEEDS, ef) entries of a level go down, so that many seed the level-0 walk."""
        ef = default_ef_upper() if ef_upper is None else int(ef_upper)
        self.upper = (ef, default_width_upper(self.M) if width_upper is None else int(width_upper), 4 * ef)
        self.walk_nseed = min(N_SEEDS, ef) if self.entry == "levels" else self.nseed

    def entry_name(self):
        """'strided', or 'levels(n_1/.../n_T)'."""
        return self.entry if self.entry == "strided" else "levels(" + "/".join(str(n) for n in self.level_n[1:]) + ")"

    def graph_bytes(self):
        n = self.graph.numel() * 4 + self.entry_docs.numel() * 4 + self.entry_ids.numel() * 8
        if self.entry == "levels":
            n += self.level_graphs.numel() * 4 + self.level_rows.numel() * 4 + self.level_down.numel() * 4
        return n

    def plan(self, k, ef_search=None, width=None):
        """(ef, width, max_steps) of a search."""
        ef = max(default_ef_search() if ef_search is None else int(ef_search), k)
        return ef, (default_width(self.M) if width is None else int(width)), 4 * ef

    def workspace_shapes(self, nq, k, ef, width, max_steps):
        E = self.entry_ids.numel()
        return (nq, 1, self.nseed, self.dim, 1, E), (nq, self.dim, self.degree, self.walk_nseed, k, ef, width, max_steps)

    def descend_shape(self, nq):
        """The arguments of dense.graph_descend_workspace_bytes for nq queries (levels only)."""
        ef, width, max_steps = self.upper
        return nq, self.dim, self.degree, len(self.level_n) - 2, self.nseed, self.walk_nseed, ef, width, max_steps

    def search(self, query, k, ef_search=None, width=None, steps=None, workspace=None, descent_steps=None, descent_workspace=None):
        """(scores f32 [nq, k] desc, ids i64 [nq, k]; -FLT_MAX / -1 padding when the walk reached fewer than k rows).  `steps` /
        `descent_steps` i32 [nq]: the steps of the level-0 walk / of the upper levels' descent."""
        ef, width, max_steps = self.plan(k, ef_search, width)
        return self.search_walk(query.contiguous(), k, ef, width, max_steps, steps=steps, workspace=workspace,
                                descent_steps=descent_steps, descent_workspace=descent_workspace)

    def descend(self, query, seed, seed_score, out=None, workspace=None, steps=None):
        """(seed i32 [nq, walk_nseed], score f32): the entry scan's best top-level nodes taken down to rows of the corpus."""
        ef, width, max_steps = self.upper
        return dense.graph_descend(query, self.docs, self.level_graphs, self.level_rows, self.level_down, self.level_n[1:-1], seed,
                                   seed_score, ef, width, max_steps, self.walk_nseed, out=out, workspace=workspace, steps=steps)

    def seeds(self, query, out=None, workspace=None):
        """(scores f32 [nq, nseed], ids i64 [nq, nseed]): the best entry rows of every query, by the exact scan."""
        zero = torch.zeros((query.shape[0], 1), dtype=torch.int32, device=query.device) if out is None else out[2]
        return dense.ivf_scan_topk(query, self.entry_docs, self.entry_offsets, self.entry_ids, self.entry_ids.numel(), zero, self.nseed,
                                   out=None if out is None else out[:2], workspace=workspace)

    def search_walk(self, query, k, ef, width, max_steps, buffers=None, steps=None, workspace=None, descent_steps=None,
                    descent_workspace=None):
        """The two device calls (entry scan, walk), three with levels (entry scan, descent, walk).  `buffers` (search_graph) =
        preallocated (seed scores, seed ids, zero probe, i32 seeds, out, two workspaces[, the descent's scores and workspace])."""
        if self.entry == "levels":
            if buffers is None:
                s, i = self.seeds(query)
                seed32, s = self.descend(query, i, s, workspace=descent_workspace, steps=descent_steps)
                return dense.graph_search_topk(query, self.docs, self.graph, seed32, s, k, ef, width, max_steps, steps=steps,
                                               workspace=workspace)
            seed_s, seed_i, zero, seed32, out, ws_entry, ws_walk, walk_s, ws_descend = buffers
            self.seeds(query, out=(seed_s, seed_i, zero), workspace=ws_entry)
            self.descend(query, seed_i, seed_s, out=(seed32, walk_s), workspace=ws_descend)
            return dense.graph_search_topk(query, self.docs, self.graph, seed32, walk_s, k, ef, width, max_steps, out=out, workspace=ws_walk)
        if buffers is None:
            s, i = self.seeds(query)
            return dense.graph_search_topk(query, self.docs, self.graph, i.to(torch.int32), s, k, ef, width, max_steps, steps=steps,
                                           workspace=workspace)
        seed_s, seed_i, zero, seed32, out, ws_entry, ws_walk = buffers
        self.seeds(query, out=(seed_s, seed_i, zero), workspace=ws_entry)
        seed32.copy_(seed_i)
        return dense.graph_search_topk(query, self.docs, self.graph, seed32, seed_s, k, ef, width, max_steps, out=out, workspace=ws_walk)

    def search_graph(self, nq, k, ef_search=None, width=None):
        """A captured graph of `search` for exactly nq <= GRAPH_MAX_QUERIES queries: `.run(query)` -> (scores, ids)."""
        ef, width, max_steps = self.plan(k, ef_search, width)
        entry, walk = self.workspace_shapes(nq, k, ef, width, max_steps)
        if (not 1 <= nq <= GRAPH_MAX_QUERIES or dense.graph_search_workspace_bytes(*walk) < 1 or dense.ivf_scan_workspace_bytes(*entry) < 1 or
                (self.entry == "levels" and dense.graph_descend_workspace_bytes(*self.descend_shape(nq)) < 1)):
            raise ValueError(f"search_graph: nq={nq} k={k} ef={ef} width={width} is outside the device walk (1..{GRAPH_MAX_QUERIES} queries)")
        return SearchGraph(self, nq, k, ef, width, max_steps)


class SearchGraph:
    """`HNSWIndex.search` of a fixed (nq, k, ef, width) as one replayed graph: static query, seed and output buffers and both
    workspaces are allocated here, the first search runs eagerly (it loads the kernels), the second is captured."""

    def __init__(self, index, nq, k, ef, width, max_steps):
        dev = index.docs.device
        self.query = torch.zeros((nq, index.dim), dtype=torch.float32, device=dev)

        def empty(n, dtype):
            return torch.empty((nq, n), dtype=dtype, device=dev)

        entry, walk = index.workspace_shapes(nq, k, ef, width, max_steps)
        buffers = (empty(index.nseed, torch.float32), empty(index.nseed, torch.int64), torch.zeros((nq, 1), dtype=torch.int32, device=dev),
                   empty(index.walk_nseed, torch.int32), (empty(k, torch.float32), empty(k, torch.int64)),
                   torch.empty(dense.ivf_scan_workspace_bytes(*entry), dtype=torch.uint8, device=dev),
                   torch.empty(dense.graph_search_workspace_bytes(*walk), dtype=torch.uint8, device=dev))
        if index.entry == "levels":
            buffers += (empty(index.walk_nseed, torch.float32),
                        torch.empty(dense.graph_descend_workspace_bytes(*index.descend_shape(nq)), dtype=torch.uint8, device=dev))
        index.search_walk(self.query, k, ef, width, max_steps, buffers)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = index.search_walk(self.query, k, ef, width, max_steps, buffers)
        self.index, self.buffers = index, buffers          # the graph holds their addresses

    def run(self, query):
        self.query.copy_(query)
        self.graph.replay()
        return self.out[0].clone(), self.out[1].clone()


def search(query, docs, k, M, ef_search=None, width=None, report=True):
    """faiss_search.search for 'HNSW<M>' on device tensors: add (kNN lists, links, entry rows or upper levels, by MEVI_HNSW_ENTRY)
    + search; recall vs exact, the entry, steps (with levels also the descent's) and graph size on stderr."""
    hip.require_gpu()
    index = HNSWIndex(docs, M)
    nq = query.shape[0]
    ef, width, max_steps = index.plan(k, ef_search, width)
    steps = torch.zeros(nq, dtype=torch.int32, device=query.device)
    down_steps = torch.zeros(nq, dtype=torch.int32, device=query.device) if index.entry == "levels" else None
    s, i = index.search(query, k, ef_search, width, steps=steps, descent_steps=down_steps)
    if report:
        es, ei = dense.DenseIndex(docs).search(query, k)
        rec = {}
        chunk = max(1, min(256, (1 << 28) // (k * k)))           # in chunks of queries: the comparison tensor is [chunk, k, k]
        for a in range(0, nq, chunk):
            part = ivf.recall_report(i[a:a + chunk], ei[a:a + chunk], cutoffs=tuple(sorted({1, 10, k})))
            for c, v in part.items():
                rec[c] = rec.get(c, 0.0) + v * min(chunk, nq - a)
        rec = {c: v / max(1, nq) for c, v in rec.items()}
        st = steps.float()
        print(f"[mevi_amd] HNSW{M} efSearch={ef} width={width} entry={index.entry_name()}: recall vs exact search " +
              ", ".join(f"@{c} {v:.4f}" for c, v in rec.items()) +
              (f"; steps: mean {float(st.mean()):.1f} / max {int(st.max())}, {int((steps >= max_steps).sum())} of {nq} queries hit "
               f"max_steps={max_steps}" if nq else "") +
              (f"; descent (ef {index.upper[0]}, width {index.upper[1]}) steps: mean {float(down_steps.float().mean()):.1f} / max "
               f"{int(down_steps.max())}" if nq and down_steps is not None else "") +
              f"; {index.graph_bytes()} bytes of graph and entry rows", file=sys.stderr)
    return s, i
