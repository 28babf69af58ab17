"""Residual-quantiser indexes behind `faiss_search.py --param RQ<M>x<b>` / `IVF<n>,RQ<M>x<b>`.

faiss builds `IndexResidualQuantizer(dim, M, nbits, METRIC_INNER_PRODUCT)` / `IndexIVFResidualQuantizer(IndexFlatIP, dim, nlist, M,
nbits, METRIC_INNER_PRODUCT)` with `by_residual = true`: an ADDITIVE quantiser of M levels x K = 2^nbits centroids, every one of
them a full dim-column vector; level i is trained on what levels < i leave of at most 256 * K sampled rows (of their residuals to
the coarse centroid behind IVF), a document is stored as its M code bytes -- 64 bytes a row at 'RQ64x8', the bytes of 'PQ64' --
and a search scores the rows of the query's `nprobe` best lists by ADC: <q, centroid> + sum_j <q, codebook[j][code_j]>.  `RQ{M}x{b}`
is the string the reference's own codebook builder hands to faiss (MEVI/pq.py:183-184).

Two deliberate deviations from faiss, the first one a default only:
  * encoding and training are GREEDY by default: level i takes the nearest centroid to the residual of levels < i.  faiss keeps a
    beam (`max_beam_size` = 5) through the levels in both.  `RQIndex(..., beam=L)` / MEVI_RQINDEX_BEAM=L (1..16; faiss: 5) encodes
    with a beam of L paths ranked by reconstruction error (below); MEVI_RQINDEX_TRAIN_BEAM=L trains every level on the residuals
    of all beam entries, as faiss's trainer does.  Both default to 1, which is the greedy code path, untouched.  (The fused beam
    encoder mevi_rq_beam_encode_f32 is MEVI's cluster beam: softmax products, 8 levels -- it is not this one.);
  * k-means is seeded from our own RNG, as for every index here, so centroids and codebooks cannot be compared with faiss.
What IS defined -- and tested bit for bit against the oracle -- given the centroids and the codebook:
  * the list of a row: `ivf.assign` (largest inner product, lowest list on ties);
  * its codes: oracle.rq.rq_encode of the f32 residual over all M levels (L2 argmin per level, lowest index on ties, one rounded
    f32 subtraction per level and element), u8 [nd, M] list-major, ids ascending inside a list.  On the device: groups of at most 8
    levels through `rq.rq_encode` (the matrix-core encoder's envelope) and between two groups one mevi_rq_residual_f32 in place;
  * search: lut[j][c] = the sequential fmaf chain <q, codebook[j][c]> from +0 over all dim columns, score = ((bias + lut[0][code_0])
    + lut[1][code_1]) + ... in ascending j with bias = the coarse score of the list (+0 without a coarse quantiser), top-k over all
    probed rows (score desc, id asc, -FLT_MAX / -1 padding).
Beam encoding (beam = L > 1), defined level by level and tested bit for bit (tests/rq_errbeam_cases.py): a level takes the B residual
rows a document has (1 at level 0: the row `encode` forms today), err(b, c) = the fmaf chain of the squared differences to centroid
c (the bits of -mevi_rq_neg_dist_f32: the whole reconstruction error of that path), keeps the min(L, B * K) smallest (err, b * K + c)
in ascending order and hands on res[parent] - centroid[code]; the stored codes are the path of slot 0 after the last level.  With
L = 1 that walk IS the greedy encoder.  One mevi_rq_errbeam_step_f32 per level over ping-pong buffers, one mevi_rq_errbeam_codes_u8
per chunk; MEVI_RQINDEX_BEAM_STEP=steps (and dim > 4096) runs a level as mevi_rq_neg_dist_f32 -> torch.sort of the packed keys ->
mevi_gather_sub_f32 instead.  The search side is the same bytes, tables and scan.
`RQIndex.search` is two stream-ordered device calls, the coarse quantiser of IVF-PQ (mevi_ivf_scan_topk_f32 on the centroids as one
list) and mevi_aq_scan_topk_f32 (csrc/aq_scan.hip); up to GRAPH_MAX_QUERIES queries can be captured and replayed (`search_graph`).

Not built: norm suffixes ('RQ8x8_Nqint8', ... -- they store a norm for L2 search; inner product needs none), 'LSQ...'
and 'PRQ...' (local-search and product-residual quantisers), groups of levels of different widths ('RQ1x16-6x8'), 'OPQ...,RQ...',
a sharded form under torchrun.  Those strings keep the exact search, as do MEVI_RQINDEX=exact and shapes outside the envelope.
"""
import os
import re
import sys

import torch

from . import dense, hip, ivf, rq

MAX_POINTS_PER_CENTROID = 256     # faiss ClusteringParameters: the training sample is at most 256 * K rows
RQ_NITER = 25                     # ... and every level's k-means runs 25 iterations from one seeding
GRAPH_MAX_QUERIES = ivf.GRAPH_MAX_QUERIES
ENCODE_MAX_LEVELS = 8             # levels of one rq.rq_encode call: the matrix-core encoder's envelope
ENCODE_CHUNK = 1 << 17            # rows whose residuals exist at a time during the build


MAX_BEAM = 16                     # beams of one step call: a parent is a byte, a lane per kept slot


def env_beam(name):
    """The beam width an environment variable asks for: unset = 1 (greedy); anything but an integer in 1..MAX_BEAM is a ValueError."""
    raw = os.environ.get(name, "1")
    if not re.fullmatch(r"\s*\d+\s*", raw) or not 1 <= int(raw) <= MAX_BEAM:
        raise ValueError(f"{name}={raw!r} must be an integer in 1..{MAX_BEAM}")
    return int(raw)


def check_beam(beam, name="beam"):
    if isinstance(beam, bool) or not isinstance(beam, int) or not 1 <= beam <= MAX_BEAM:
        raise ValueError(f"{name}={beam!r} must be an integer in 1..{MAX_BEAM}")
    return beam


def parse_factory(param):
    """(nlist or None, M, nbits) of 'RQ<M>x<b>' and 'IVF<n>,RQ<M>x<b>' with 1 <= b <= 8 (<b> is mandatory, as in faiss), else None."""
    g = re.fullmatch(r"\s*(?:IVF(\d+)\s*,\s*)?RQ(\d+)x(\d+)\s*", str(param))
    if not g or not 1 <= int(g.group(3)) <= 8:
        return None
    return (int(g.group(1)) if g.group(1) else None, int(g.group(2)), int(g.group(3)))


def supported(nd, dim, topk, nlist, M, nbits):
    """True when an index of this shape is inside the envelope of the build and of the scan (host arithmetic): dim % 4 == 0,
    4 <= M <= 96 with M % 4 == 0, the table within 96 KiB, at least K rows to train on, 0 < nlist <= nd, topk <= 4096."""
    K = 1 << nbits
    if nd < K or (nlist is not None and not 0 < nlist <= nd):
        return False
    return dense.aq_scan_workspace_bytes(1, 1, topk, dim, M, K, 1 if nlist is None else nlist, nd) > 0


def wanted(param, nd, dim, topk):
    """(nlist or None, M, nbits) when `dense.search` / `dense.profile` serve `param` with an RQIndex: the string parses, the shape
    is `supported` and MEVI_RQINDEX is not 'exact' (which restores the exact answer these strings had before); else None."""
    spec = parse_factory(param)
    if spec is None or os.environ.get("MEVI_RQINDEX", "index") == "exact" or not supported(nd, dim, topk, *spec):
        return None
    return spec


def factory_name(nlist, M, nbits):
    return ("" if nlist is None else f"IVF{nlist},") + f"RQ{M}x{nbits}"


def level_errors(xs, codebook, codes):
    """[M] floats: the mean squared norm of what levels 0..j leave of the rows `xs` under `codes` i32 [n, M], j = 0..M-1 (the
    residuals are those of the encoder: one mevi_rq_residual_f32 a level)."""
    res, out = xs, []
    for j in range(codebook.shape[0]):
        res = dense.rq_residual(res, codebook[j:j + 1].contiguous(), codes[:, j:j + 1], out=None if res is xs else res)
        out.append(float((res.double() ** 2).sum(1).mean()))
    return out


def train_codebook(docs, list_of, centroids, M, nbits, seed=1234, stats=None):
    """The residual quantiser: rq.train_rq_codebook (level i = k-means on the residual of levels < i, greedy) on at most 256 * K rows
    drawn from `seed`, taken as residuals to their list's centroid when there is a coarse quantiser -> f32 [M, K, dim].  With a
    dict `stats`: 'train_rows', 'input_mse' (mean squared norm of the sample) and 'level_mse' (`level_errors` of the sample)."""
    n = docs.shape[0]
    K = 1 << nbits
    gen = torch.Generator(device=docs.device).manual_seed(int(seed))
    rows = torch.randperm(n, generator=gen, device=docs.device)[:min(n, MAX_POINTS_PER_CENTROID * K)]
    xs = docs[rows]
    if centroids is not None:
        xs = xs - centroids[list_of[rows].long()]
    xs = xs.contiguous()
    train_beam = env_beam("MEVI_RQINDEX_TRAIN_BEAM")
    if train_beam > 1:
        return train_codebook_beam(xs, M, K, int(seed), train_beam, stats)
    book, codes = rq.train_rq_codebook(xs, M, K, seed=int(seed), n_init=1, max_iter=RQ_NITER)
    book = book.contiguous()
    if stats is not None:
        stats.update(train_rows=int(rows.numel()), input_mse=float((xs.double() ** 2).sum(1).mean()),
                     level_mse=level_errors(xs, book, codes.to(torch.int32).contiguous()))
    return book


def train_codebook_beam(xs, M, K, seed, beam, stats=None):
    """faiss's default trainer (MEVI_RQINDEX_TRAIN_BEAM = beam > 1): level i's k-means (`rq.kmeans`, seed + i, as the greedy trainer)
    runs on the residual rows of ALL beam entries of the sample, [n_s * B, dim]; one step call then hands the beams on.  `stats`:
    'train_rows', 'input_mse', 'level_mse' (mean error of the best path after each level), 'train_beam', 'beam_mse' (after the last)."""
    n, dim = xs.shape
    cur, book, level_mse = xs.view(n, 1, dim), [], []
    for level in range(M):
        centers, _, _ = rq.kmeans(cur.reshape(-1, dim), K, seed=seed + level, n_init=1, max_iter=RQ_NITER)
        centers = centers.contiguous()
        book.append(centers)
        _, _, err, cur = beam_step(cur, centers, beam, want_res=level != M - 1)
        level_mse.append(float(err[:, 0].double().mean()))
    if stats is not None:
        stats.update(train_rows=int(n), input_mse=float((xs.double() ** 2).sum(1).mean()), level_mse=level_mse, train_beam=int(beam),
                     beam_mse=level_mse[-1])
    return torch.stack(book).contiguous()


def beam_step_is_fused(n, dim, K, B, L):
    """True when `beam_step` takes mevi_rq_errbeam_step_f32 (csrc/rq_errbeam.hip): not MEVI_RQINDEX_BEAM_STEP=steps and the shape is
    inside the kernel's envelope (dim <= 4096, ...); otherwise the composition `beam_step_composed` runs."""
    mode = os.environ.get("MEVI_RQINDEX_BEAM_STEP", "fused")
    if mode not in ("fused", "steps"):
        raise ValueError(f"MEVI_RQINDEX_BEAM_STEP={mode!r} must be 'fused' or 'steps'")
    return mode == "fused" and dense.rq_errbeam_step_workspace_bytes(n, dim, K, B, L) > 0


def beam_step(res_in, centroids, L, res_out=None, want_res=True, workspace=None):
    """One level of the beam encoder: `dense.rq_errbeam_step`, or the composition that states the same contract."""
    n, B, dim = res_in.shape
    if beam_step_is_fused(n, dim, centroids.shape[0], B, L):
        return dense.rq_errbeam_step(res_in, centroids, L, res_out=res_out, want_res=want_res, workspace=workspace)
    return beam_step_composed(res_in, centroids, L, res_out=res_out, want_res=want_res)


def beam_step_composed(res_in, centroids, L, res_out=None, want_res=True):
    """`dense.rq_errbeam_step` as mevi_rq_neg_dist_f32 -> torch.sort of the packed (err bits, b * K + c) keys -> mevi_gather_sub_f32
    (MEVI_RQINDEX_BEAM_STEP=steps; any dim % 4 == 0).  The same bits: err is the negated score (exact), +0 or above, so its bit
    pattern orders it, and the flat index in the low word breaks ties."""
    lib = hip.lib()
    n, B, dim = res_in.shape
    K = centroids.shape[0]
    Lo, dev = min(int(L), B * K), res_in.device
    if want_res and res_out is None:
        res_out = torch.empty((n, Lo, dim), dtype=torch.float32, device=dev)
    if n == 0:
        empty = torch.empty((0, Lo), dtype=torch.uint8, device=dev)
        return empty, empty.clone(), torch.empty((0, Lo), dtype=torch.float32, device=dev), res_out if want_res else None
    neg = torch.empty((n * B, K), dtype=torch.float32, device=dev)
    with hip.device_guard(dev):
        hip.check(lib.mevi_rq_neg_dist_f32(hip.ptr(res_in), n * B, dim, hip.ptr(centroids), K, hip.ptr(neg), hip.stream_ptr()),
                  "mevi_rq_neg_dist_f32")
        keys = ((-neg).view(torch.int32).view(n, B * K).to(torch.int64) << 32) | torch.arange(B * K, device=dev)[None]
        keys = torch.sort(keys, dim=1).values[:, :Lo]
        flat = keys & 0xFFFFFFFF
        parent, code = flat // K, flat % K
        err = (keys >> 32).to(torch.int32).view(torch.float32)
        if want_res:
            src = (torch.arange(n, device=dev)[:, None] * B + parent).reshape(-1).contiguous()
            hip.check(lib.mevi_gather_sub_f32(hip.ptr(res_in), hip.ptr(src), hip.ptr(centroids), hip.ptr(code.to(torch.int32).reshape(-1).contiguous()),
                                              n * Lo, dim, hip.ptr(res_out), hip.stream_ptr()), "mevi_gather_sub_f32")
    return parent.to(torch.uint8), code.to(torch.uint8), err.contiguous(), res_out if want_res else None


def encode_walk(docs, rows, list_of, centroids, codebook, beam, chunk=ENCODE_CHUNK, stats=None):
    """`encode` with a beam of `beam` >= 1 paths (1: the greedy codes, by the beam's own route): per chunk of chunk // beam rows the
    residual row as `encode` forms it, M step calls over two ping-pong buffers [rows, beam, dim] that write the (parent, code) traces
    u8 [M, rows, beam], one backtrack into the chunk's code rows.  `stats['code_mse']`: the mean over all rows of the kept path's
    error (the last level's err[:, 0]), summed in float64."""
    check_beam(beam)
    M, K, dim = codebook.shape
    n = docs.shape[0] if rows is None else rows.numel()
    dev = docs.device
    codes = torch.empty((n, M), dtype=torch.uint8, device=dev)
    per = max(1, chunk // beam)
    width, most = beam, min(per, max(n, 1))                      # slots of a trace row; rows of the largest chunk
    bufs = [torch.empty(most * width * dim, dtype=torch.float32, device=dev) for _ in range(2 if M > 1 else 0)]
    trace = torch.zeros((2, M * most * width), dtype=torch.uint8, device=dev)     # (slots past a level's Lo are never reached)
    ws = torch.empty(max(1, dense.rq_errbeam_step_workspace_bytes(min(per, n), dim, K, beam, beam)), dtype=torch.uint8, device=dev)
    total = torch.zeros((), dtype=torch.float64, device=dev)
    for a in range(0, n, per):
        x = docs[a:a + per] if rows is None else docs[rows[a:a + per]]
        if centroids is not None:
            sel = list_of[a:a + per] if rows is None else list_of[rows[a:a + per]]
            x = x - centroids[sel.long()]                       # the f32 residual, one rounding per element
        x = x.contiguous()
        r = x.shape[0]
        parents, kept = (t[:M * r * width].view(M, r, width) for t in trace)
        cur, B = x.view(r, 1, dim), 1
        for j in range(M):
            Lo, last = min(beam, B * K), j == M - 1
            out = None if last else bufs[j & 1][:r * Lo * dim].view(r, Lo, dim)
            parent, code, err, cur = beam_step(cur, codebook[j], beam, res_out=out, want_res=not last, workspace=ws)
            parents[j, :, :Lo], kept[j, :, :Lo] = parent, code
            B = Lo
        total += err[:, 0].double().sum()
        dense.rq_errbeam_codes(parents, kept, r, out=codes[a:a + per])
    if stats is not None:
        stats["code_mse"] = float(total) / max(1, n)
    return codes


def encode(docs, rows, list_of, centroids, codebook, chunk=ENCODE_CHUNK, beam=1, stats=None):
    """u8 [len(rows), M]: the codes of docs[rows] in that order (rows None: of all rows, in place), residuals and codes produced
    `chunk` rows at a time (never a second f32 copy of the corpus).  The M levels go through `rq.rq_encode` in groups of at most
    ENCODE_MAX_LEVELS; between two groups the chunk's residual is taken on by one mevi_rq_residual_f32, in place.
    beam > 1: `encode_walk` (chunk // beam rows at a time); `stats` then receives 'code_mse'."""
    if check_beam(beam) > 1:
        return encode_walk(docs, rows, list_of, centroids, codebook, beam, chunk=chunk, stats=stats)
    M = codebook.shape[0]
    n = docs.shape[0] if rows is None else rows.numel()
    codes = torch.empty((n, M), dtype=torch.uint8, device=docs.device)
    groups = [codebook[g:g + ENCODE_MAX_LEVELS].contiguous() for g in range(0, M, ENCODE_MAX_LEVELS)]
    for a in range(0, n, chunk):
        x = docs[a:a + chunk] if rows is None else docs[rows[a:a + chunk]]
        own = rows is not None                                  # whether x is this loop's tensor (docs' own rows are never written)
        if centroids is not None:
            sel = list_of[a:a + chunk] if rows is None else list_of[rows[a:a + chunk]]
            x, own = x - centroids[sel.long()], True            # the f32 residual, one rounding per element
        x = x.contiguous()
        for i, book in enumerate(groups):
            part = rq.rq_encode(x, book)
            codes[a:a + chunk, i * ENCODE_MAX_LEVELS:i * ENCODE_MAX_LEVELS + book.shape[0]] = part.to(torch.uint8)
            if i + 1 < len(groups):
                x, own = dense.rq_residual(x, book, part, out=x if own else None), True
    return codes


class RQIndex:
    """`index.train(doc); index.add(doc)` of 'IVF<n>,RQ<M>x<b>' (nlist=None: 'RQ<M>x<b>'): centroids, codebook, codes list by list."""

    def __init__(self, docs, nlist, M, nbits, centroids=None, codebook=None, seed=1234, beam=None):
        self.beam = env_beam("MEVI_RQINDEX_BEAM") if beam is None else check_beam(beam)   # paths the encoder keeps (faiss: 5)
        assert docs.is_cuda and docs.dtype == torch.float32 and docs.dim() == 2
        nd, dim = docs.shape
        assert 1 <= nbits <= 8 and M >= 1, (M, nbits)
        dev = docs.device
        self.nlist, self.M, self.nbits, self.K, self.dim = nlist, M, nbits, 1 << nbits, dim
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
        self.train_stats = {}                                   # filled when the codebook is trained here
        self.codebook = (train_codebook(docs, self.list_of, self.centroids, M, nbits, seed, self.train_stats) if codebook is None
                         else codebook.to(dev).contiguous())
        assert self.codebook.shape == (M, self.K, dim), (self.codebook.shape, M, self.K, dim)
        self.encode_stats = {"beam": self.beam}                 # + 'code_mse' under a beam
        self.codes = encode(docs, None if nlist is None else self.ids, self.list_of, self.centroids, self.codebook, beam=self.beam,
                            stats=self.encode_stats)

    @property
    def n_lists(self):
        return 1 if self.nlist is None else self.nlist

    def clamp_nprobe(self, nprobe):
        return max(1, min(int(nprobe), self.n_lists))

    def workspace_shapes(self, nq, k, nprobe):
        """Argument tuples of the workspace queries of the two calls (coarse: None without a coarse quantiser)."""
        coarse = None if self.nlist is None else (nq, 1, nprobe, self.dim, 1, self.nlist)
        return coarse, (nq, nprobe, k, self.dim, self.M, self.K, self.n_lists, self.max_list_len)

    def search(self, query, k, nprobe=1):
        """(scores f32 [nq, k] desc, ids i64 [nq, k]; -FLT_MAX / -1 padding when the probed lists hold fewer than k)."""
        return self.search_scan(query.contiguous(), k, self.clamp_nprobe(nprobe))

    def search_scan(self, query, k, nprobe, buffers=None):
        """The two device calls.  `buffers` (search_graph) = preallocated (zero probe, coarse out, i32 probe, out, two workspaces)."""
        nq = query.shape[0]
        if buffers is None:
            zero = torch.zeros((nq, 1), dtype=torch.int32, device=query.device)
            if self.nlist is None:
                return dense.aq_scan_topk(query, self.codebook, self.codes, self.offsets_dev, None, self.max_list_len, zero, None, k)
            bias, lists = dense.ivf_scan_topk(query, self.centroids, self.centroid_offsets, None, self.nlist, zero, nprobe)
            return dense.aq_scan_topk(query, self.codebook, self.codes, self.offsets_dev, self.ids, self.max_list_len,
                                      lists.to(torch.int32), bias, k)
        zero, coarse, probe, out, ws_coarse, ws_scan = buffers
        if self.nlist is None:
            return dense.aq_scan_topk(query, self.codebook, self.codes, self.offsets_dev, None, self.max_list_len, zero, None, k,
                                      out=out, workspace=ws_scan)
        dense.ivf_scan_topk(query, self.centroids, self.centroid_offsets, None, self.nlist, zero, nprobe, out=coarse, workspace=ws_coarse)
        probe.copy_(coarse[1])
        return dense.aq_scan_topk(query, self.codebook, self.codes, self.offsets_dev, self.ids, self.max_list_len, probe, coarse[0], k,
                                  out=out, workspace=ws_scan)

    def search_graph(self, nq, k, nprobe=1):
        """A captured graph of `search` for exactly nq <= GRAPH_MAX_QUERIES queries: `.run(query)` -> (scores, ids)."""
        nprobe = self.clamp_nprobe(nprobe)
        coarse, scan = self.workspace_shapes(nq, k, nprobe)
        if not 1 <= nq <= GRAPH_MAX_QUERIES or dense.aq_scan_workspace_bytes(*scan) < 1 or (
                coarse is not None and dense.ivf_scan_workspace_bytes(*coarse) < 1):
            raise ValueError(f"search_graph: nq={nq} k={k} nprobe={nprobe} is outside the device scan (1..{GRAPH_MAX_QUERIES} queries)")
        return SearchGraph(self, nq, k, nprobe)


class SearchGraph:
    """`RQIndex.search` of a fixed (nq, k, nprobe) as one replayed graph: static query, probe and output buffers and both
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
                   torch.empty(dense.aq_scan_workspace_bytes(*scan), dtype=torch.uint8, device=dev))
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


def search(query, docs, k, nlist, M, nbits, nprobe=None, report=True):
    """faiss_search.search for 'IVF<n>,RQ<M>x<b>' / 'RQ<M>x<b>' on device tensors: train + add + search; on stderr the recall vs the
    exact search and the training error per level (mean squared residual norm of the training sample after each level)."""
    hip.require_gpu()
    if nprobe is None:
        nprobe = int(os.environ.get("MEVI_IVF_NPROBE", "1"))
    index = RQIndex(docs, nlist, M, nbits)
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
        st = index.train_stats
        beam = f" beam={index.beam}" if index.beam > 1 else ""    # (the greedy default prints the line it always printed)
        print(f"[mevi_amd] {factory_name(nlist, M, nbits)} nprobe={index.clamp_nprobe(nprobe)}{beam}: recall vs exact search " +
              ", ".join(f"@{c} {v:.4f}" for c, v in rec.items()) +
              f"; {index.codes.numel()} bytes of codes; lists: min {int(sizes.min())} / mean {float(sizes.float().mean()):.0f} / "
              f"max {int(sizes.max())} documents; training error per level (mean squared residual norm of {st['train_rows']} rows, "
              f"{st['input_mse']:.6g} before): " + " ".join(f"{v:.6g}" for v in st["level_mse"]), file=sys.stderr)
    return s, i
