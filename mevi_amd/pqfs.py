"""4-bit fast-scan PQ behind `faiss_search.py --param IVF<n>,PQ<m>x4fs` / `PQ<m>x4fs`.

faiss builds `IndexIVFPQFastScan` / `IndexPQFastScan` for these strings: product quantisers of m subspaces x 16 centroids whose
codes are stored two to a byte and scanned from small per-query tables.  Here the index is `ivfpq.IVFPQIndex` with nbits = 4 --
the same coarse quantiser, the same lists, the same codebook training (`ivfpq.train_codebook`) and the same encoder
(`ivfpq.encode`), codes of RESIDUALS x - centroid[list of x] (`by_residual`, as IVFPQIndex) -- with another storage format and
another scan:
  * a row is m / 2 bytes: byte t holds code 2t in its low nibble and code 2t + 1 in its high nibble (mevi_pq4_pack);
  * the scan (mevi_pqfs_scan_topk_f32, csrc/pqfs_scan.hip) keeps every table entry replicated in LDS so that a gather cannot meet
    a bank conflict, and returns the bits the byte scan returns for the same codebook and codes: f32 tables, lut[j][c] = the
    sequential fmaf chain <q_j, codebook[j][c]> from +0, score = ((bias + lut[0][c_0]) + lut[1][c_1]) + ... in ascending j.
What is NOT faiss's fast scan: the tables are not quantised to u8 and summed in u16 (so results equal 'PQ<m>x4', not faiss's
fast-scan approximation of it); the 32-row interleaved block layout is not reproduced (rows are stored one after the other); and
codes are of residuals, while faiss's IVF fast-scan class is believed to default to by_residual = false.

`PQFSIndex.search` is two stream-ordered device calls, as `IVFPQIndex.search`; up to GRAPH_MAX_QUERIES queries can be captured
and replayed (`search_graph`).  The result is approximate; `search` also runs the exact search and reports recall on stderr.
"""
import os
import re
import sys

import torch

from . import dense, hip, ivf, ivfpq

NBITS = 4
K = 1 << NBITS
GRAPH_MAX_QUERIES = ivf.GRAPH_MAX_QUERIES
PACK_CHUNK = ivfpq.ENCODE_CHUNK   # rows whose byte codes exist at a time during the build


def parse_factory(param):
    """(nlist or None, m) of 'IVF<n>,PQ<m>x4fs' and 'PQ<m>x4fs', else None (other widths, 'fsr', block-size suffixes, ...)."""
    g = re.fullmatch(r"\s*(?:IVF(\d+)\s*,\s*)?PQ(\d+)x4fs\s*", str(param))
    if not g:
        return None
    return (int(g.group(1)) if g.group(1) else None, int(g.group(2)))


def supported(nd, dim, topk, nlist, m):
    """True when an index of this shape is inside the envelope of the build and of the scan (host arithmetic): dim = m subspaces
    of a multiple of 4 columns, m % 8 == 0 in 8..96, at least 16 rows to train on, 0 < nlist <= nd, topk <= 4096."""
    if m < 1 or dim % m != 0 or nd < K or (nlist is not None and not 0 < nlist <= nd):
        return False
    return dense.pqfs_scan_workspace_bytes(1, 1, topk, dim, m, 1 if nlist is None else nlist, nd) > 0


def wanted(param, nd, dim, topk):
    """(nlist or None, m) when `dense.search` / `dense.profile` serve `param` with a PQFSIndex: the string parses, the shape is
    `supported` and MEVI_PQFS is not 'exact' (which restores the exact answer these strings had before); else None."""
    spec = parse_factory(param)
    if spec is None or os.environ.get("MEVI_PQFS", "index") == "exact" or not supported(nd, dim, topk, *spec):
        return None
    return spec


class PQFSIndex:
    """`index.train(doc); index.add(doc)` of 'IVF<n>,PQ<m>x4fs' (nlist=None: 'PQ<m>x4fs'): centroids, codebook, packed codes list
    by list.  `codes` is u8 [nd, m / 2]."""

    def __init__(self, docs, nlist, m, centroids=None, codebook=None, seed=1234, rotation=None):
        """rotation: None, or an orthonormal R f32 [dim, dim] (mevi_amd/opq.py), as for IVFPQIndex."""
        assert docs.is_cuda and docs.dtype == torch.float32 and docs.dim() == 2
        nd, dim = docs.shape
        assert m >= 2 and m % 2 == 0 and dim % m == 0, (dim, m)
        dev = docs.device
        self.nlist, self.m, self.nbits, self.K, self.dim = nlist, m, NBITS, K, dim
        if nlist is None:                                       # one list, no coarse quantiser, the id is the row
            self.centroids = None
            self.list_of = torch.zeros(nd, dtype=torch.int32, device=dev)
            self.offsets = torch.tensor([0, nd], dtype=torch.int64)
            self.offsets_dev = self.offsets.to(dev)
            self.ids = torch.arange(nd, dtype=torch.int64, device=dev)
            self.max_list_len = nd
        else:
            self.centroids = ivf.train_centroids(docs, nlist, seed) if centroids is None else centroids.to(dev).contiguous()
            self.list_of = ivf.assign(docs, self.centroids)
            self.offsets, self.offsets_dev, self.ids, self.max_list_len = ivf.build_lists(self.list_of, nlist)
            self.centroid_offsets = torch.tensor([0, nlist], dtype=torch.int64, device=dev)   # the quantiser's one list
        self.rotation = None if rotation is None else ivfpq.rotated_centroids(self.centroids, rotation.to(dev))
        self.codebook = (ivfpq.train_codebook(docs, self.list_of, self.centroids, m, NBITS, seed, self.rotation) if codebook is None
                         else codebook.to(dev).contiguous())
        assert self.codebook.shape == (m, K, dim // m), (self.codebook.shape, m, K, dim)
        self.codes = torch.empty((nd, m // 2), dtype=torch.uint8, device=dev)
        for a in range(0, nd, PACK_CHUNK):                      # byte codes of a chunk -> its packed rows; the bytes are dropped
            b = min(nd, a + PACK_CHUNK)
            if nlist is None:
                part = ivfpq.encode(docs[a:b], None, None, None, self.codebook, rotation=self.rotation)
            else:
                part = ivfpq.encode(docs, self.ids[a:b], self.list_of, self.centroids, self.codebook, rotation=self.rotation)
            dense.pq4_pack(part, out=self.codes[a:b])

    @property
    def n_lists(self):
        return 1 if self.nlist is None else self.nlist

    def clamp_nprobe(self, nprobe):
        return max(1, min(int(nprobe), self.n_lists))

    def workspace_shapes(self, nq, k, nprobe):
        """Argument tuples of the workspace queries of the two calls (coarse: None without a coarse quantiser)."""
        coarse = None if self.nlist is None else (nq, 1, nprobe, self.dim, 1, self.nlist)
        return coarse, (nq, nprobe, k, self.dim, self.m, self.n_lists, self.max_list_len)

    def search(self, query, k, nprobe=1):
        """(scores f32 [nq, k] desc, ids i64 [nq, k]; -FLT_MAX / -1 padding when the probed lists hold fewer than k)."""
        return self.search_scan(query.contiguous(), k, self.clamp_nprobe(nprobe))

    def search_scan(self, query, k, nprobe, buffers=None):
        """The two device calls (behind a rotation: one GEMM on the queries first).  `buffers` (search_graph) = preallocated (zero
        probe, coarse out, i32 probe, out, two workspaces, rotated queries or None)."""
        nq = query.shape[0]
        rotated = query if self.rotation is None else ivfpq.rotate_queries(query, self.rotation[0], buffers)   # what the ADC scan reads
        if buffers is None:
            zero = torch.zeros((nq, 1), dtype=torch.int32, device=query.device)
            if self.nlist is None:
                return dense.pqfs_scan_topk(rotated, self.codebook, self.codes, self.offsets_dev, None, self.max_list_len, zero, None, k)
            bias, lists = dense.ivf_scan_topk(query, self.centroids, self.centroid_offsets, None, self.nlist, zero, nprobe)
            return dense.pqfs_scan_topk(rotated, self.codebook, self.codes, self.offsets_dev, self.ids, self.max_list_len,
                                        lists.to(torch.int32), bias, k)
        zero, coarse, probe, out, ws_coarse, ws_scan = buffers[:6]
        if self.nlist is None:
            return dense.pqfs_scan_topk(rotated, self.codebook, self.codes, self.offsets_dev, None, self.max_list_len, zero, None, k,
                                        out=out, workspace=ws_scan)
        dense.ivf_scan_topk(query, self.centroids, self.centroid_offsets, None, self.nlist, zero, nprobe, out=coarse, workspace=ws_coarse)
        probe.copy_(coarse[1])
        return dense.pqfs_scan_topk(rotated, self.codebook, self.codes, self.offsets_dev, self.ids, self.max_list_len, probe, coarse[0],
                                    k, out=out, workspace=ws_scan)

    def search_graph(self, nq, k, nprobe=1):
        """A captured graph of `search` for exactly nq <= GRAPH_MAX_QUERIES queries: `.run(query)` -> (scores, ids)."""
        nprobe = self.clamp_nprobe(nprobe)
        coarse, scan = self.workspace_shapes(nq, k, nprobe)
        if not 1 <= nq <= GRAPH_MAX_QUERIES or dense.pqfs_scan_workspace_bytes(*scan) < 1 or (
                coarse is not None and dense.ivf_scan_workspace_bytes(*coarse) < 1):
            raise ValueError(f"search_graph: nq={nq} k={k} nprobe={nprobe} is outside the device scan (1..{GRAPH_MAX_QUERIES} queries)")
        return SearchGraph(self, nq, k, nprobe)


class SearchGraph:
    """`PQFSIndex.search` of a fixed (nq, k, nprobe) as one replayed graph: static query, probe and output buffers and both
    workspaces are allocated here, the first search runs eagerly (it loads the kernels), the second is captured."""

    def __init__(self, index, nq, k, nprobe):
        dev = index.codes.device
        self.query = torch.zeros((nq, index.dim), dtype=torch.float32, device=dev)

        def empty(n, dtype):
            return torch.empty((nq, n), dtype=dtype, device=dev)

        coarse, scan = index.workspace_shapes(nq, k, nprobe)
        buffers = (torch.zeros((nq, 1), dtype=torch.int32, device=dev), (empty(nprobe, torch.float32), empty(nprobe, torch.int64)),
                   empty(nprobe, torch.int32), (empty(k, torch.float32), empty(k, torch.int64)),
                   None if coarse is None else torch.empty(dense.ivf_scan_workspace_bytes(*coarse), dtype=torch.uint8, device=dev),
                   torch.empty(dense.pqfs_scan_workspace_bytes(*scan), dtype=torch.uint8, device=dev),
                   None if index.rotation is None else torch.empty_like(self.query))       # the rotated queries
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


def factory_name(nlist, m):
    return ("" if nlist is None else f"IVF{nlist},") + f"PQ{m}x4fs"


def search(query, docs, k, nlist, m, nprobe=None, report=True):
    """faiss_search.search for 'IVF<n>,PQ<m>x4fs' / 'PQ<m>x4fs' on device tensors: train + add + search, recall vs exact on stderr."""
    hip.require_gpu()
    if nprobe is None:
        nprobe = int(os.environ.get("MEVI_IVF_NPROBE", "1"))
    index = PQFSIndex(docs, nlist, m)
    s, i = index.search(query, k, nprobe)
    if report:
        es, ei = dense.DenseIndex(docs).search(query, min(k, 4096))
        rec = {}
        for a in range(0, query.shape[0], 256):                  # in chunks of queries: the comparison tensor is [nq, c, c]
            part = ivf.recall_report(i[a:a + 256, :ei.shape[1]], ei[a:a + 256])
            for c, v in part.items():
                rec[c] = rec.get(c, 0.0) + v * min(256, query.shape[0] - a)
        rec = {c: v / max(1, query.shape[0]) for c, v in rec.items()}
        sizes = (index.offsets[1:] - index.offsets[:-1])
        print(f"[mevi_amd] {factory_name(nlist, m)} nprobe={index.clamp_nprobe(nprobe)}: recall vs exact search " +
              ", ".join(f"@{c} {v:.4f}" for c, v in rec.items()) +
              f"; {index.codes.numel()} bytes of packed codes; lists: min {int(sizes.min())} / mean {float(sizes.float().mean()):.0f} / "
              f"max {int(sizes.max())} documents", file=sys.stderr)
    return s, i
