"""IVF-PQ and PQ behind `faiss_search.py --param IVF<n>,PQ<m>[x<b>]` / `PQ<m>[x<b>]`.

faiss builds `IndexIVFPQ(IndexFlatIP, dim, nlist, m, nbits, METRIC_INNER_PRODUCT)` with `by_residual = true` (`IndexPQ` for the
string without IVF): a coarse quantiser as in IVF-Flat (mevi_amd/ivf.py), a product quantiser of m subspaces x K = 2^nbits
centroids trained on the RESIDUALS x - centroid[list of x] of at most 256 * K sampled rows, every document stored as m code
bytes in the inverted list of its best centroid, and a search that scores the rows of the query's `nprobe` best lists by
asymmetric distance computation (ADC): <q, centroid> + sum_j <q_j, codebook[j][code_j]>.  k-means is seeded from our own RNG,
as for IVF-Flat, so lists and codebooks cannot be compared with faiss; what IS defined -- and tested bit for bit against the
oracle -- given the centroids and the codebook:
  * the list of a row: `ivf.assign` (largest inner product, lowest list on ties);
  * its codes: mevi_pq_encode_f32 of the f32 residual (L2 argmin per subspace, lowest index on ties), u8 [nd, m] list-major, ids
    ascending inside a list;
  * search: lut[j][c] = the sequential fmaf chain <q_j, codebook[j][c]> from +0, score = ((bias + lut[0][code_0]) + lut[1][code_1])
    + ... in ascending j with bias = the coarse score of the list (+0 without a coarse quantiser), top-k over all probed rows
    (score desc, id asc, -FLT_MAX / -1 padding).
Without IVF there is no coarse quantiser: the residual is the row itself and the index is one list.

`IVFPQIndex.search` is two stream-ordered device calls: the coarse quantiser (mevi_ivf_scan_topk_f32 on the centroids as one
list, k = nprobe) and the ADC scan (mevi_ivfpq_scan_topk_f32, csrc/ivfpq_scan.hip) with the coarse scores as the bias of every
probe slot.  Nothing is copied to the host, so up to GRAPH_MAX_QUERIES queries can be captured and replayed (`search_graph`).
The result is approximate by construction; `search` also runs the exact search and reports recall on stderr.

With `rotation=R` (mevi_amd/opq.py, 'OPQ<M>,...') the product quantiser works behind an orthonormal rotation: lists and coarse
search are unchanged, the codes are of chain(x, R) - chain(centroid, R), and the scan reads chain(q, R) -- one more GEMM a search.
"""
import os
import re
import sys

import torch

from . import dense, hip, ivf, rq

MAX_POINTS_PER_CENTROID = 256     # faiss ClusteringParameters: the PQ training sample is at most 256 * K rows
PQ_NITER = 25                     # ... and every subspace's k-means runs 25 iterations from one seeding
GRAPH_MAX_QUERIES = ivf.GRAPH_MAX_QUERIES
ENCODE_MAX_M = 32                 # subspaces of one mevi_pq_encode_f32 call
ENCODE_CHUNK = 1 << 17            # rows whose residuals exist at a time during the build


def parse_factory(param):
    """(nlist or None, m, nbits) of 'IVF<n>,PQ<m>', 'IVF<n>,PQ<m>x<b>', 'PQ<m>' and 'PQ<m>x<b>' with 1 <= b <= 8, else None."""
    g = re.fullmatch(r"\s*(?:IVF(\d+)\s*,\s*)?PQ(\d+)(?:x(\d+))?\s*", str(param))
    if not g:
        return None
    nbits = int(g.group(3)) if g.group(3) else 8
    if not 1 <= nbits <= 8:
        return None
    return (int(g.group(1)) if g.group(1) else None, int(g.group(2)), nbits)


def supported(nd, dim, topk, nlist, m, nbits):
    """True when an index of this shape is inside the envelope of the build and of the scan (host arithmetic): dim = m subspaces
    of a multiple of 4 columns, m % 4 == 0, the table within 96 KiB, at least K rows to train on, 0 < nlist <= nd, topk <= 4096."""
    K = 1 << nbits
    if m < 1 or dim % m != 0 or nd < K or (nlist is not None and not 0 < nlist <= nd):
        return False
    return dense.ivfpq_scan_workspace_bytes(1, 1, topk, dim, m, K, 1 if nlist is None else nlist, nd) > 0


def wanted(param, nd, dim, topk):
    """(nlist or None, m, nbits) when `dense.search` / `dense.profile` serve `param` with an IVFPQIndex: the string parses, the
    shape is `supported` and MEVI_IVFPQ is not 'exact' (which restores the exact answer these strings had before); else None."""
    spec = parse_factory(param)
    if spec is None or os.environ.get("MEVI_IVFPQ", "index") == "exact" or not supported(nd, dim, topk, *spec):
        return None
    return spec


def rotated_centroids(centroids, R):
    """The `rotation` pair (R, crot) of an index behind a learned rotation (mevi_amd/opq.py): crot = chain(centroids, R), one
    `ops.linear`, None without a coarse quantiser."""
    from . import ops

    R = R.contiguous()
    return R, (None if centroids is None else ops.linear(centroids, R))


def rotate_queries(query, R, buffers=None):
    """chain(q, R) of a batch of queries: one GEMM launch, into the seventh of a search graph's `buffers` when there are any."""
    from . import ops

    return ops.linear(query, R, out=None if buffers is None else buffers[6])


def train_codebook(docs, list_of, centroids, m, nbits, seed=1234, rotation=None):
    """The product quantiser: rq.train_pq_codebook on the residuals of at most 256 * K rows drawn from `seed` -> f32 [m, K, dsub].
    rotation = (R, crot): on the ROTATED residuals chain(x, R) - crot[list of x] of the same rows (dense.opq_rotate_rows)."""
    n = docs.shape[0]
    K = 1 << nbits
    gen = torch.Generator(device=docs.device).manual_seed(int(seed))
    rows = torch.randperm(n, generator=gen, device=docs.device)[:min(n, MAX_POINTS_PER_CENTROID * K)]
    if rotation is not None:
        xs = dense.opq_rotate_rows(docs, rows, None if centroids is None else list_of, rotation[1], rotation[0])
    else:
        xs = docs[rows]
        if centroids is not None:
            xs = xs - centroids[list_of[rows].long()]
    return rq.train_pq_codebook(xs.contiguous(), m, K, seed=int(seed), n_init=1, max_iter=PQ_NITER)[0].contiguous()


def encode(docs, rows, list_of, centroids, codebook, chunk=ENCODE_CHUNK, rotation=None):
    """u8 [len(rows), m]: the codes of docs[rows] in that order, residuals and codes produced `chunk` rows at a time (never a
    second f32 copy of the corpus); more than ENCODE_MAX_M subspaces are encoded in groups on contiguous column slices.
    rotation = (R, crot): the codes of the rotated residuals, a chunk of them from one dense.opq_rotate_rows call."""
    m, _, dsub = codebook.shape
    n = docs.shape[0] if rows is None else rows.numel()
    codes = torch.empty((n, m), dtype=torch.uint8, device=docs.device)
    for a in range(0, n, chunk):
        if rotation is not None:
            sel = None if centroids is None else (list_of[a:a + chunk] if rows is None else list_of)
            x = dense.opq_rotate_rows(docs[a:a + chunk] if rows is None else docs, None if rows is None else rows[a:a + chunk], sel,
                                      rotation[1], rotation[0])
        else:
            x = docs[a:a + chunk] if rows is None else docs[rows[a:a + chunk]]
            if centroids is not None:
                sel = list_of[a:a + chunk] if rows is None else list_of[rows[a:a + chunk]]
                x = x - centroids[sel.long()]                   # the f32 residual, one rounding per element
        for g in range(0, m, ENCODE_MAX_M):
            h = min(m, g + ENCODE_MAX_M)
            part = x if (g == 0 and h == m) else x[:, g * dsub:h * dsub]
            codes[a:a + chunk, g:h] = rq.pq_encode(part.contiguous(), codebook[g:h].contiguous()).to(torch.uint8)
    return codes


class IVFPQIndex:
    """`index.train(doc); index.add(doc)` of 'IVF<n>,PQ<m>x<b>' (nlist=None: 'PQ<m>x<b>'): centroids, codebook, codes list by list."""

    def __init__(self, docs, nlist, m, nbits=8, centroids=None, codebook=None, seed=1234, rotation=None):
        """rotation: None, or an orthonormal R f32 [dim, dim] (mevi_amd/opq.py) -- lists and coarse search stay those of the
        unrotated rows, the product quantiser codes chain(x, R) - chain(centroid, R) and the scan reads chain(q, R)."""
        assert docs.is_cuda and docs.dtype == torch.float32 and docs.dim() == 2
        nd, dim = docs.shape
        assert 1 <= nbits <= 8 and m >= 1 and dim % m == 0, (dim, m, nbits)
        dev = docs.device
        self.nlist, self.m, self.nbits, self.K, self.dim = nlist, m, nbits, 1 << nbits, dim
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
        self.rotation = None if rotation is None else rotated_centroids(self.centroids, rotation.to(dev))
        self.codebook = (train_codebook(docs, self.list_of, self.centroids, m, nbits, seed, self.rotation) if codebook is None
                         else codebook.to(dev).contiguous())
        assert self.codebook.shape == (m, self.K, dim // m), (self.codebook.shape, m, self.K, dim)
        self.codes = encode(docs, None if nlist is None else self.ids, self.list_of, self.centroids, self.codebook,
                            rotation=self.rotation)

    @property
    def n_lists(self):
        return 1 if self.nlist is None else self.nlist

    def clamp_nprobe(self, nprobe):
        return max(1, min(int(nprobe), self.n_lists))

    def workspace_shapes(self, nq, k, nprobe):
        """Argument tuples of the workspace queries of the two calls (coarse: None without a coarse quantiser)."""
        coarse = None if self.nlist is None else (nq, 1, nprobe, self.dim, 1, self.nlist)
        return coarse, (nq, nprobe, k, self.dim, self.m, self.K, self.n_lists, self.max_list_len)

    def search(self, query, k, nprobe=1):
        """(scores f32 [nq, k] desc, ids i64 [nq, k]; -FLT_MAX / -1 padding when the probed lists hold fewer than k)."""
        return self.search_scan(query.contiguous(), k, self.clamp_nprobe(nprobe))

    def search_scan(self, query, k, nprobe, buffers=None):
        """The two device calls (behind a rotation: one GEMM on the queries first).  `buffers` (search_graph) = preallocated (zero
        probe, coarse out, i32 probe, out, two workspaces, rotated queries or None)."""
        nq = query.shape[0]
        rotated = query if self.rotation is None else rotate_queries(query, self.rotation[0], buffers)   # what the ADC scan reads
        if buffers is None:
            zero = torch.zeros((nq, 1), dtype=torch.int32, device=query.device)
            if self.nlist is None:
                return dense.ivfpq_scan_topk(rotated, self.codebook, self.codes, self.offsets_dev, None, self.max_list_len, zero, None, k)
            bias, lists = dense.ivf_scan_topk(query, self.centroids, self.centroid_offsets, None, self.nlist, zero, nprobe)
            return dense.ivfpq_scan_topk(rotated, self.codebook, self.codes, self.offsets_dev, self.ids, self.max_list_len,
                                         lists.to(torch.int32), bias, k)
        zero, coarse, probe, out, ws_coarse, ws_scan = buffers[:6]
        if self.nlist is None:
            return dense.ivfpq_scan_topk(rotated, self.codebook, self.codes, self.offsets_dev, None, self.max_list_len, zero, None, k,
                                         out=out, workspace=ws_scan)
        dense.ivf_scan_topk(query, self.centroids, self.centroid_offsets, None, self.nlist, zero, nprobe, out=coarse, workspace=ws_coarse)
        probe.copy_(coarse[1])
        return dense.ivfpq_scan_topk(rotated, self.codebook, self.codes, self.offsets_dev, self.ids, self.max_list_len, probe, coarse[0],
                                     k, out=out, workspace=ws_scan)

    def search_graph(self, nq, k, nprobe=1):
        """A captured graph of `search` for exactly nq <= GRAPH_MAX_QUERIES queries: `.run(query)` -> (scores, ids)."""
        nprobe = self.clamp_nprobe(nprobe)
        coarse, scan = self.workspace_shapes(nq, k, nprobe)
        if not 1 <= nq <= GRAPH_MAX_QUERIES or dense.ivfpq_scan_workspace_bytes(*scan) < 1 or (
                coarse is not None and dense.ivf_scan_workspace_bytes(*coarse) < 1):
            raise ValueError(f"search_graph: nq={nq} k={k} nprobe={nprobe} is outside the device scan (1..{GRAPH_MAX_QUERIES} queries)")
        return SearchGraph(self, nq, k, nprobe)


class SearchGraph:
    """`IVFPQIndex.search` of a fixed (nq, k, nprobe) as one replayed graph: static query, probe and output buffers and both
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
                   torch.empty(dense.ivfpq_scan_workspace_bytes(*scan), dtype=torch.uint8, device=dev),
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


def factory_name(nlist, m, nbits):
    return ("" if nlist is None else f"IVF{nlist},") + f"PQ{m}" + ("" if nbits == 8 else f"x{nbits}")


def search(query, docs, k, nlist, m, nbits=8, nprobe=None, report=True):
    """faiss_search.search for 'IVF<n>,PQ<m>x<b>' / 'PQ<m>x<b>' on device tensors: train + add + search, recall vs exact on stderr."""
    hip.require_gpu()
    if nprobe is None:
        nprobe = int(os.environ.get("MEVI_IVF_NPROBE", "1"))
    index = IVFPQIndex(docs, nlist, m, nbits)
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
        print(f"[mevi_amd] {factory_name(nlist, m, nbits)} nprobe={index.clamp_nprobe(nprobe)}: recall vs exact search " +
              ", ".join(f"@{c} {v:.4f}" for c, v in rec.items()) +
              f"; {index.codes.numel()} bytes of codes; lists: min {int(sizes.min())} / mean {float(sizes.float().mean()):.0f} / "
              f"max {int(sizes.max())} documents", file=sys.stderr)
    return s, i
