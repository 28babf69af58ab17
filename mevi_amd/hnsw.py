"""A neighbour-graph index behind `faiss_search.py --param HNSW<M>` (the reference README's own ANN command uses HNSW256).

faiss builds `IndexHNSWFlat(dim, M, METRIC_INNER_PRODUCT)`: M links per node on the upper levels, 2M on level 0, built by
sequential insertion (efConstruction 40) with random levels and diversity pruning, searched with a candidate list of
max(efSearch, k) entries (efSearch 16).  Its insertion order and RNG cannot be reproduced, so neither can its graph; what this
index keeps is HNSW's level-0 structure and its search, with the two serial parts replaced by brute force:
  * graph : i32 [nd, 2M].  Slots [0, M) of row v = v's M nearest other rows by exact inner product (one exact search of the rows
    against themselves, in chunks); the remaining slots = reverse links: the rows u that name v as their forward neighbour of
    rank r, outside v's own forward links, in ascending (r, u) order until the row is full (mevi_graph_link).  There is NO
    diversity pruning (faiss's shrink_neighbor_list) and there are no upper levels.
  * entry : instead of the upper levels' descent, ENTRY_ROWS = min(nd, 4096) rows at a fixed stride (row floor(i * nd / E)) are
    scored per query with mevi_ivf_scan_topk_f32 as one list; the best N_SEEDS = 32 seed the walk, scores included.
  * search: best-first over the graph with ef = max(efSearch, k) entries, `width` entries expanded per step, at most 4 * ef steps
    (mevi_graph_search_topk_f32, csrc/graph_search.hip; the semantics are pinned in include/mevi_hip_graph.h).
Every returned score is the exact search's score for that id, bit for bit; which ids are found is approximate.  Given the graph
and the seeds the result is defined exactly and tested bit for bit (tests/graph_cases.py).  `search` also runs the exact search
and reports recall on stderr.

`HNSWIndex.search` is two stream-ordered device calls (entry scan, walk); nothing is copied to the host, so up to
GRAPH_MAX_QUERIES queries can be captured and replayed (`search_graph`).

Environment: MEVI_HNSW_EFSEARCH (default 16), MEVI_HNSW_WIDTH (default 1), MEVI_HNSW=exact answers the string with the exact
search, as before this index existed.
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


def parse_factory(param):
    """M of 'HNSW<M>' and 'HNSW<M>,Flat', else None: 'HNSW<M>_PQ8', 'HNSW<M>,SQ8', 'IVF..._HNSW32,...' keep the exact search."""
    g = re.fullmatch(r"\s*HNSW(\d+)\s*(?:,\s*Flat\s*)?", str(param))
    return int(g.group(1)) if g else None


def default_ef_search():
    return max(1, int(os.environ.get("MEVI_HNSW_EFSEARCH", "16")))


def default_width(M):
    return max(1, min(int(os.environ.get("MEVI_HNSW_WIDTH", "1")), dense.GRAPH_MAX_BATCH // (2 * M)))


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


def entry_rows(nd, device):
    E = min(nd, ENTRY_ROWS)
    return (torch.arange(E, dtype=torch.int64, device=device) * nd) // max(E, 1)


class HNSWIndex:
    """`index.add(doc)` of 'HNSW<M>': kNN lists, links, entry rows.  `knn` / `graph` given: taken instead of built."""

    def __init__(self, docs, M, knn=None, graph=None, timing=None):
        import time

        hip.require_gpu()
        assert docs.is_cuda and docs.dtype == torch.float32 and docs.dim() == 2
        self.docs = docs.contiguous()
        nd, dim = self.docs.shape
        self.M, self.dim, self.degree = M, dim, 2 * M

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
        self.entry_ids = entry_rows(nd, docs.device)
        self.entry_docs = self.docs[self.entry_ids].contiguous()
        self.entry_offsets = torch.tensor([0, self.entry_ids.numel()], dtype=torch.int64, device=docs.device)
        self.nseed = min(N_SEEDS, self.entry_ids.numel())
        lap("entry_s", t)

    def graph_bytes(self):
        return self.graph.numel() * 4 + self.entry_docs.numel() * 4 + self.entry_ids.numel() * 8

    def plan(self, k, ef_search=None, width=None):
        """(ef, width, max_steps) of a search."""
        ef = max(default_ef_search() if ef_search is None else int(ef_search), k)
        return ef, (default_width(self.M) if width is None else int(width)), 4 * ef

    def workspace_shapes(self, nq, k, ef, width, max_steps):
        E = self.entry_ids.numel()
        return (nq, 1, self.nseed, self.dim, 1, E), (nq, self.dim, self.degree, self.nseed, k, ef, width, max_steps)

    def search(self, query, k, ef_search=None, width=None, steps=None, workspace=None):
        """(scores f32 [nq, k] desc, ids i64 [nq, k]; -FLT_MAX / -1 padding when the walk reached fewer than k rows)."""
        ef, width, max_steps = self.plan(k, ef_search, width)
        return self.search_walk(query.contiguous(), k, ef, width, max_steps, steps=steps, workspace=workspace)

    def seeds(self, query, out=None, workspace=None):
        """(scores f32 [nq, nseed], ids i64 [nq, nseed]): the best entry rows of every query, by the exact scan."""
        zero = torch.zeros((query.shape[0], 1), dtype=torch.int32, device=query.device) if out is None else out[2]
        return dense.ivf_scan_topk(query, self.entry_docs, self.entry_offsets, self.entry_ids, self.entry_ids.numel(), zero, self.nseed,
                                   out=None if out is None else out[:2], workspace=workspace)

    def search_walk(self, query, k, ef, width, max_steps, buffers=None, steps=None, workspace=None):
        """The two device calls.  `buffers` (search_graph) = preallocated (seed scores, seed ids, zero probe, i32 seeds, out,
        two workspaces)."""
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
        if not 1 <= nq <= GRAPH_MAX_QUERIES or dense.graph_search_workspace_bytes(*walk) < 1 or dense.ivf_scan_workspace_bytes(*entry) < 1:
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
                   empty(index.nseed, torch.int32), (empty(k, torch.float32), empty(k, torch.int64)),
                   torch.empty(dense.ivf_scan_workspace_bytes(*entry), dtype=torch.uint8, device=dev),
                   torch.empty(dense.graph_search_workspace_bytes(*walk), dtype=torch.uint8, device=dev))
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
    """faiss_search.search for 'HNSW<M>' on device tensors: add (kNN lists, links, entry rows) + search; recall vs exact, steps
    and graph size on stderr."""
    hip.require_gpu()
    index = HNSWIndex(docs, M)
    nq = query.shape[0]
    ef, width, max_steps = index.plan(k, ef_search, width)
    steps = torch.zeros(nq, dtype=torch.int32, device=query.device)
    s, i = index.search(query, k, ef_search, width, steps=steps)
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
        print(f"[mevi_amd] HNSW{M} efSearch={ef} width={width}: recall vs exact search " +
              ", ".join(f"@{c} {v:.4f}" for c, v in rec.items()) +
              (f"; steps: mean {float(st.mean()):.1f} / max {int(st.max())}, {int((steps >= max_steps).sum())} of {nq} queries hit "
               f"max_steps={max_steps}" if nq else "") +
              f"; {index.graph_bytes()} bytes of graph and entry rows", file=sys.stderr)
    return s, i
