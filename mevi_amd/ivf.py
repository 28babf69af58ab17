"""IVF-Flat behind `faiss_search.py --param IVF<n>,Flat` (the script's DEFAULT factory string, MEVI/faiss_search.py:89;
SURVEY 8(f).4).

faiss builds `IndexIVFFlat(IndexFlatIP, dim, nlist, METRIC_INNER_PRODUCT)`: a coarse quantiser of `nlist` centroids
trained by k-means on at most 256 * nlist sampled rows (25 iterations, assignment by the quantiser = largest inner
product, centroid = mean of its rows), every document stored in the inverted list of its best centroid, and a search
that scans only the `nprobe` (default 1) best lists of the query.  faiss-cpu 1.7.4 is absent from the reference tree and
its k-means is seeded from its own RNG, so list contents cannot be matched bit for bit; what IS defined -- and tested
against the oracle -- given the centroids:
  * assignment: argmax_c <d, centroid_c> (exact f32 chains, lowest list on ties),
  * search: the exact top-k (score desc, id asc, faiss padding) among the documents of the query's `nprobe` best lists.
Because the result is approximate by construction, `search` also runs the exact search and reports recall against it
(stderr, so the script's stdout stays the reference's).  `nprobe` comes from MEVI_IVF_NPROBE (faiss default: 1).

`IVFFlatIndex.search` is two stream-ordered calls of one C-ABI entry point (mevi_ivf_scan_topk_f32, csrc/ivf_scan.hip):
the coarse quantiser -- the centroids as one list every query probes, k = nprobe -- and the scan of the probed lists,
which groups the (query, slot) pairs by list on the device, shares every pass over a list's rows among the pairs that
probe it and selects each query's top-k over all its probed rows at once.  Nothing is copied to the host, so a search of
up to GRAPH_MAX_QUERIES queries can be captured and replayed as one graph (`search_graph`).  `search_lists` is the
earlier host loop (one exact search per probed list + a merge): same bits; it serves the shapes outside the scan's
envelope, the regimes where it measured faster (scan_wanted: many query tiles over few long lists) and every shape when
MEVI_IVF_SCAN=lists.

The build (`train_centroids`, `IVFFlatIndex.__init__`) labels rows with mevi_ivf_assign_f32 -- the exact GEMM's loop with a running
(best score, lowest index) per row instead of a stored score matrix -- and lays the lists out with mevi_ivf_build_lists (a stable
sort of (label, row) on the device), both in csrc/ivf_build.hip.  MEVI_IVF_BUILD=host restores the torch composition they
replaced (exact GEMM + argmax, argsort + bincount): same bits, the A/B partner of DESIGN 4.1g and the path of shapes outside the
kernels' envelope.
"""
import os
import re
import sys

import numpy as np
import torch

from . import dense, ops, rq

MAX_POINTS_PER_CENTROID = 256     # faiss ClusteringParameters defaults
NITER = 25
GRAPH_MAX_QUERIES = 32            # search_graph: the batch sizes of faiss_search.profile / latency_b1
# where `search` takes the device scan (profiles/ivf_scan_c2.json, 8.8 M x 768, k = 1000): up to SCAN_MAX_TILES query tiles it
# beat the host loop at IVF100 and IVF4096 alike (6980 queries at nprobe 1: 4 and 3 tiles); with more tiles it still did at
# IVF4096 (11 and 42 tiles: 123 vs 544 ms, 436 vs 795 ms) and lost at IVF100 (15 and 60 tiles: 232 vs 129 ms, 999 vs 255 ms)
SCAN_MAX_TILES = 4
SCAN_ANY_TILES_NLIST = 4096


def parse_factory(param):
    """nlist of an 'IVF<n>,Flat' factory string, else None (every other index type is served by exact search)."""
    m = re.fullmatch(r"\s*IVF(\d+)\s*,\s*Flat\s*", str(param))
    return int(m.group(1)) if m else None


def build_path():
    """'device' (the kernels of csrc/ivf_build.hip) or 'host' (MEVI_IVF_BUILD=host: the torch composition they replaced --
    exact GEMM + argmax, argsort + bincount -- unchanged: the A/B partner, and what shapes outside the envelope take)."""
    return "host" if os.environ.get("MEVI_IVF_BUILD", "device") == "host" else "device"


def assign_wanted(n, dim, nlist):
    """True when `assign` takes mevi_ivf_assign_f32: not MEVI_IVF_BUILD=host and the shape is inside the kernel's envelope."""
    return build_path() == "device" and n >= 1 and dense.ivf_assign_workspace_bytes(n, dim, nlist) > 0


def assign(x, centroids, chunk=1 << 18):
    """argmax_c <x, centroid_c> per row (exact f32 chains; lowest c on ties) -> i32 [n]."""
    if assign_wanted(x.shape[0], x.shape[1], centroids.shape[0]) and x.dtype == torch.float32 and centroids.dtype == torch.float32:
        out = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
        return dense.ivf_assign(x.contiguous(), centroids.contiguous(), out=(out, None))[0]
    return assign_host(x, centroids, chunk)


def assign_host(x, centroids, chunk=1 << 18):
    """`assign` as the score matrix of the exact GEMM, chunk by chunk, and its argmax."""
    out = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
    for a in range(0, x.shape[0], chunk):
        out[a:a + chunk] = torch.argmax(ops.linear(x[a:a + chunk].contiguous(), centroids), dim=1).to(torch.int32)
    return out


def lists_wanted(n, nlist):
    """True when `build_lists` takes mevi_ivf_build_lists: not MEVI_IVF_BUILD=host and the shape is inside its envelope."""
    return build_path() == "device" and n >= 1 and dense.ivf_build_lists_workspace_bytes(n, nlist) > 0


def build_lists(list_of, nlist):
    """Labels -> (offsets i64 [nlist + 1] on the CPU, the same on the device, ids i64 [n]: the rows ordered by (list, row), the
    longest list as an int).  The device path is one call; its offsets and longest list come back once (the scan's ABI wants
    the latter on the host)."""
    if lists_wanted(list_of.numel(), nlist):
        offsets_dev, order, longest = dense.ivf_build_lists(list_of, nlist)
        return offsets_dev.cpu(), offsets_dev, order, int(longest.item())
    order = torch.argsort(list_of.long(), stable=True)                    # ids ascending inside a list
    offsets = torch.zeros(nlist + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(torch.bincount(list_of.long(), minlength=nlist), 0).cpu()
    return offsets, offsets.to(list_of.device), order, (int((offsets[1:] - offsets[:-1]).max()) if nlist else 0)


def train_centroids(docs, nlist, seed=1234):
    """k-means as faiss's Clustering runs it for an inner-product IVF: sample, random distinct rows as the first
    centroids, NITER x (assign by inner product, mean); an empty list takes a row of the largest one."""
    n, dim = docs.shape
    gen = torch.Generator(device=docs.device).manual_seed(int(seed))
    perm = torch.randperm(n, generator=gen, device=docs.device)
    xs = docs[perm[:min(n, MAX_POINTS_PER_CENTROID * nlist)]].contiguous()
    cent = xs[:nlist].clone() if xs.shape[0] >= nlist else torch.cat(
        [xs, torch.zeros((nlist - xs.shape[0], dim), dtype=torch.float32, device=docs.device)])
    for _ in range(NITER):
        lab = assign(xs, cent)
        new, counts, _ = rq.cluster_means(xs, lab, nlist, old=cent)
        empty = torch.nonzero(counts == 0).flatten()
        if empty.numel():
            big = int(torch.argmax(counts).item())
            rows = torch.nonzero(lab == big).flatten()
            pick = rows[torch.randperm(rows.numel(), generator=gen, device=docs.device)[:empty.numel()]]
            new[empty[:pick.numel()]] = xs[pick]
        cent = new
    return cent.contiguous()


class IVFFlatIndex:
    """`index.train(doc); index.add(doc)` of the IVF factory string: centroids, documents stored list by list."""

    def __init__(self, docs, nlist, centroids=None, seed=1234):
        assert docs.is_cuda and docs.dtype == torch.float32 and docs.dim() == 2
        self.nlist = nlist
        self.centroids = train_centroids(docs, nlist, seed) if centroids is None else centroids.to(docs.device).contiguous()
        self.list_of = assign(docs, self.centroids)
        self.offsets, self.offsets_dev, self.ids, self.max_list_len = build_lists(self.list_of, nlist)
        self.docs = docs[self.ids].contiguous()
        self.centroid_offsets = torch.tensor([0, nlist], dtype=torch.int64, device=docs.device)   # the quantiser's one list

    def scan_wanted(self, nq, k, nprobe):
        """True when `search` takes the device scan: the shape is inside its envelope (a workspace size exists for both of its
        calls), MEVI_IVF_SCAN does not ask for the host loop, and the regime is one where the scan measured at least as fast
        (DESIGN 4.1f): the scan passes over the probed lists once per query tile, the host loop once per probed list, so many
        tiles over few lists -- thousands of queries at nprobe >= 4 on an index of a hundred long lists -- stay with the loop."""
        if os.environ.get("MEVI_IVF_SCAN", "scan") == "lists" or nq < 1 or nprobe > dense.IVF_MAX_NPROBE:
            return False
        dim = self.docs.shape[1]
        tile = dense.ivf_scan_query_tile(nq, nprobe, k, dim, self.nlist, self.max_list_len)
        if tile < 1 or dense.ivf_scan_workspace_bytes(nq, 1, nprobe, dim, 1, self.nlist) < 1:
            return False
        return -(-nq // tile) <= SCAN_MAX_TILES or self.nlist >= SCAN_ANY_TILES_NLIST

    def search(self, query, k, nprobe=1):
        """(scores f32 [nq, k] desc, ids i64 [nq, k]; -FLT_MAX / -1 padding when the probed lists hold fewer than k)."""
        nprobe = max(1, min(int(nprobe), self.nlist))
        if not self.scan_wanted(query.shape[0], k, nprobe):
            return self.search_lists(query, k, nprobe)
        return self.search_scan(query.contiguous(), k, nprobe)

    def search_scan(self, query, k, nprobe, buffers=None):
        """The two device calls.  `buffers` (search_graph) = preallocated (zero probe, coarse out, i32 probe, out, two workspaces)."""
        nq = query.shape[0]
        dev = query.device
        if buffers is None:
            zero = torch.zeros((nq, 1), dtype=torch.int32, device=dev)
            coarse = dense.ivf_scan_topk(query, self.centroids, self.centroid_offsets, None, self.nlist, zero, nprobe)
            probe = coarse[1].to(torch.int32)                              # [nq, nprobe] best lists (score desc, list asc)
            return dense.ivf_scan_topk(query, self.docs, self.offsets_dev, self.ids, self.max_list_len, probe, k)
        zero, coarse, probe, out, ws_coarse, ws_scan = buffers
        dense.ivf_scan_topk(query, self.centroids, self.centroid_offsets, None, self.nlist, zero, nprobe, out=coarse, workspace=ws_coarse)
        probe.copy_(coarse[1])
        return dense.ivf_scan_topk(query, self.docs, self.offsets_dev, self.ids, self.max_list_len, probe, k, out=out, workspace=ws_scan)

    def search_graph(self, nq, k, nprobe=1):
        """A captured graph of `search` for exactly nq <= GRAPH_MAX_QUERIES queries: `.run(query)` -> (scores, ids)."""
        nprobe = max(1, min(int(nprobe), self.nlist))
        if not 1 <= nq <= GRAPH_MAX_QUERIES or not self.scan_wanted(nq, k, nprobe):
            raise ValueError(f"search_graph: nq={nq} k={k} nprobe={nprobe} is outside the device scan (1..{GRAPH_MAX_QUERIES} queries)")
        return SearchGraph(self, nq, k, nprobe)

    def search_lists(self, query, k, nprobe=1):
        """`search` as a host loop over the probed lists: one exact search per list, then a merge.  Same result, bit for bit."""
        nq = query.shape[0]
        nprobe = max(1, min(int(nprobe), self.nlist))
        dev = query.device
        probe = dense.ip_topk(query, self.centroids, nprobe)[1]            # [nq, nprobe] best lists (score desc, list asc)
        neg = -torch.finfo(torch.float32).max
        cand_s = torch.full((nprobe, nq, k), neg, dtype=torch.float32, device=dev)
        cand_i = torch.full((nprobe, nq, k), -1, dtype=torch.int64, device=dev)
        probe_h = probe.cpu().numpy()
        off = self.offsets.numpy()
        for l in np.unique(probe_h):
            a, b = int(off[l]), int(off[l + 1])
            if a == b:
                continue
            slot, qsel = np.nonzero(probe_h.T == l)                        # which probe slot of which query
            qs = torch.from_numpy(qsel).to(dev)
            s, i = dense.ip_topk(query[qs].contiguous(), self.docs[a:b], k)
            gid = torch.where(i >= 0, self.ids[a:b][i.clamp_min(0)], i)    # list-local row -> document id
            cand_s[torch.from_numpy(slot).to(dev), qs] = s
            cand_i[torch.from_numpy(slot).to(dev), qs] = gid
        if nprobe == 1:
            out_s, out_i = cand_s[0], cand_i[0]
            # inside one list the local order is (score desc, LOCAL row asc) = (score desc, id asc): ids ascend in a list
            return out_s, out_i
        return dense.topk_merge(cand_s, cand_i, k)


class SearchGraph:
    """`IVFFlatIndex.search` of a fixed (nq, k, nprobe) as one replayed graph: static query, probe and output buffers and both
    workspaces are allocated here, the first search runs eagerly (it loads the kernels), the second is captured."""

    def __init__(self, index, nq, k, nprobe):
        dev, dim = index.docs.device, index.docs.shape[1]
        self.query = torch.zeros((nq, dim), dtype=torch.float32, device=dev)

        def empty(n, dtype):
            return torch.empty((nq, n), dtype=dtype, device=dev)

        def ws(*shape):
            return torch.empty(dense.ivf_scan_workspace_bytes(*shape), dtype=torch.uint8, device=dev)

        buffers = (torch.zeros((nq, 1), dtype=torch.int32, device=dev), (empty(nprobe, torch.float32), empty(nprobe, torch.int64)),
                   empty(nprobe, torch.int32), (empty(k, torch.float32), empty(k, torch.int64)),
                   ws(nq, 1, nprobe, dim, 1, index.nlist), ws(nq, nprobe, k, dim, index.nlist, index.max_list_len))
        index.search_scan(self.query, k, nprobe, buffers)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = index.search_scan(self.query, k, nprobe, buffers)
        self.index, self.buffers = index, buffers          # the graph holds their addresses

    def run(self, query):
        self.query.copy_(query)
        self.graph.replay()
        return self.out[0].clone(), self.out[1].clone()


def recall_report(approx_ids, exact_ids, cutoffs=(1, 10, 100, 1000)):
    """|approx top-c  ∩  exact top-c| / c averaged over queries, for every cutoff <= k."""
    out = {}
    k = exact_ids.shape[1]
    for c in cutoffs:
        if c > k:
            continue
        hit = (approx_ids[:, :c, None] == exact_ids[:, None, :c]) & (exact_ids[:, None, :c] >= 0)
        denom = (exact_ids[:, :c] >= 0).sum(1).clamp_min(1)
        out[c] = float((hit.any(1).sum(1).double() / denom.double()).mean().item())
    return out


def search(query, docs, k, nlist, nprobe=None, report=True):
    """faiss_search.search for 'IVF<n>,Flat' on device tensors: train + add + search, recall vs exact on stderr."""
    if nprobe is None:
        nprobe = int(os.environ.get("MEVI_IVF_NPROBE", "1"))
    index = IVFFlatIndex(docs, nlist)
    s, i = index.search(query, k, nprobe)
    if report:
        es, ei = dense.DenseIndex(docs).search(query, min(k, 4096))
        # in chunks of queries: the comparison tensor is [nq, c, c]
        rec = {}
        for a in range(0, query.shape[0], 256):
            part = recall_report(i[a:a + 256, :ei.shape[1]], ei[a:a + 256])
            for c, v in part.items():
                rec[c] = rec.get(c, 0.0) + v * min(256, query.shape[0] - a)
        rec = {c: v / max(1, query.shape[0]) for c, v in rec.items()}
        sizes = (index.offsets[1:] - index.offsets[:-1])
        print(f"[mevi_amd] IVF{nlist},Flat nprobe={nprobe}: recall vs exact search " +
              ", ".join(f"@{c} {v:.4f}" for c, v in rec.items()) +
              f"; lists: min {int(sizes.min())} / mean {float(sizes.float().mean()):.0f} / max {int(sizes.max())} documents",
              file=sys.stderr)
    return s, i
