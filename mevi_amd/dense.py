"""Dense arm: exact inner-product top-k on MI355X.

Mirrors the reference's `faiss_search.search(query, doc, dim, topk, param)`
(MEVI/faiss_search.py:13-21) and adds the row-sharded multi-GPU form required by
the north star: every rank searches its contiguous shard with
global ids, one RCCL all-gather of the per-shard top-k, then a device-side merge.
"""
import os

import numpy as np
import torch

from . import hip


def _as_device_f32(x, device):
    if isinstance(x, np.ndarray) and x.ndim == 2 and x.dtype == np.float32 and x.nbytes >= (64 << 20):
        from .io import upload_rows

        return upload_rows(x, device)           # the 27 GB corpus of faiss_search.py: pinned, chunked
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    x = x.to(device=device, dtype=torch.float32)
    return x.contiguous()


def ip_topk(query, docs, k, id_offset=0):
    """Exact top-k of query @ docs.T on the current GPU.

    query f32[nq, dim], docs f32[nd, dim] (torch CUDA tensors, row-major).
    Returns (scores f32[nq,k] descending, ids i64[nq,k]); ids = id_offset + row,
    ties by ascending id, missing slots (-FLT_MAX, -1) like faiss.
    """
    hip.require_gpu()
    assert query.is_cuda and docs.is_cuda and query.dtype == torch.float32 and docs.dtype == torch.float32
    assert query.dim() == 2 and docs.dim() == 2 and query.shape[1] == docs.shape[1]
    query = query.contiguous()
    docs = docs.contiguous()
    nq, dim = query.shape
    nd = docs.shape[0]
    L = hip.lib()
    out_s = torch.empty((nq, k), dtype=torch.float32, device=query.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=query.device)
    if nq == 0:
        return out_s, out_i
    ws_bytes = L.mevi_ip_topk_workspace_bytes(nq, dim, k)
    if ws_bytes == 0:
        raise hip.MeviHipError(f"ip_topk: unsupported shape nq={nq} dim={dim} k={k}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=query.device)
    with hip.device_guard(query.device):
        st = L.mevi_ip_topk_f32(hip.ptr(query), nq, hip.ptr(docs), nd, dim, k, id_offset,
                                hip.ptr(out_s), hip.ptr(out_i), hip.ptr(ws), ws_bytes, hip.stream_ptr())
    hip.check(st, "mevi_ip_topk_f32")
    return out_s, out_i


class DenseIndex:
    """A corpus shard prepared for searching -- the analogue of faiss `index.add(doc)`
    (MEVI/faiss_search.py:19): keeps the f32 rows and their centred, scaled f16 image (+ norms, mean, scales).
    `search` returns exactly what `ip_topk` returns (bit for bit), ~3x faster: candidates are
    selected with f16 MFMAs, re-scored with the exact f32 chain and proven complete per query.  Searches of up to 32 queries
    select through an int8 image instead (half the bytes of the HBM-bound small search; DESIGN 4.1c'): same lists."""

    def __init__(self, docs):
        hip.require_gpu()
        assert docs.is_cuda and docs.dtype == torch.float32 and docs.dim() == 2
        self.docs = docs.contiguous()
        nd, dim = self.docs.shape
        L = hip.lib()
        nbytes = L.mevi_ip_index_bytes(nd, dim)
        self.index = torch.empty(nbytes, dtype=torch.uint8, device=docs.device)
        with hip.device_guard(docs.device):
            st = L.mevi_ip_index_build_f32(hip.ptr(self.docs), nd, dim, hip.ptr(self.index), nbytes, hip.stream_ptr())
        hip.check(st, "mevi_ip_index_build_f32")
        self.index8 = None          # the 8-bit image for searches of <= 32 queries (prepare_small, or once they keep coming)
        self._i8_open = {}          # per k: running share of small searches the 8-bit pass left unproven (above I8_GIVE_UP: not used)
        self._small_calls = 0       # small searches seen so far (the image is built when they keep coming: SMALL_BUILD_AFTER)

    SMALL_QUERIES = 32              # searches up to this many queries go through the 8-bit image (csrc/ip_topk.hip: i8_eligible)
    SMALL_BUILD_AFTER = 8           # ... once the index has seen this many of them: building the image is two passes over the rows
                                    # (42 ms at 8.8 M x 768 = the saving of ~40 searches) -- an index made for one search never pays it;
                                    # prepare_small() builds it at once (faiss_search.profile does, inside its `add` time)
    I8_GIVE_UP = 0.4                # ... while the running share of searches it had to repeat through the f16 image stays below this
                                    # (a repeated search costs both passes: the 8-bit image pays as long as t8 + p t16 < t16, t8 ~ 0.55 t16)

    def small_image_wanted(self, nq, k):
        nd, dim = self.docs.shape
        dimp = max(128, (dim + 63) // 64 * 64)
        return (0 < nq <= self.SMALL_QUERIES and nd >= int(os.environ.get("MEVI_IP_I8_MIN_ROWS", "65536")) and 256 <= dimp <= 896 and 3 * k + 128 <= 4096
                and os.environ.get("MEVI_IP_I8", "1") != "0" and self._i8_open.get(k, 0) < self.I8_GIVE_UP)

    def prepare_small(self):
        """Build the 8-bit image now (otherwise the search after SMALL_BUILD_AFTER small ones does): nd * dim bytes + 8 per row,
        two passes over the rows (column scales, then the image)."""
        if self.index8 is None:
            nd, dim = self.docs.shape
            L = hip.lib()
            nbytes = L.mevi_ip_index8_bytes(nd, dim)
            index8 = torch.empty(nbytes, dtype=torch.uint8, device=self.docs.device)
            with hip.device_guard(self.docs.device):
                st = L.mevi_ip_index8_build_f32(hip.ptr(self.docs), hip.ptr(self.index), nd, dim, hip.ptr(index8), nbytes, hip.stream_ptr())
            hip.check(st, "mevi_ip_index8_build_f32")
            self.index8 = index8
        return self

    def _search_small(self, query, k, id_offset, out_s, out_i):
        nq, dim = query.shape
        nd = self.docs.shape[0]
        L = hip.lib()
        self.prepare_small()
        ws_bytes = L.mevi_ip_topk_indexed8_workspace_bytes(nq, dim, k)
        if ws_bytes == 0:
            raise hip.MeviHipError(f"ip_topk_indexed8: unsupported shape nq={nq} dim={dim} k={k}")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=query.device)
        with hip.device_guard(query.device):
            st = L.mevi_ip_topk_indexed8_f32(hip.ptr(query), nq, hip.ptr(self.docs), hip.ptr(self.index), hip.ptr(self.index8), nd, dim, k,
                                             id_offset, hip.ptr(out_s), hip.ptr(out_i), hip.ptr(ws), ws_bytes, hip.stream_ptr())
        hip.check(st, "mevi_ip_topk_indexed8_f32")
        stats = hip.IpTopkStats()
        L.mevi_ip_topk_get_stats(stats)
        if stats.n_i8_queries:      # a corpus whose scores are too dense for the 8-bit bound pays both searches: stop trying
            self._i8_open[k] = 0.75 * self._i8_open.get(k, 0.0) + (0.25 if stats.n_i8_unproven else 0.0)
        return out_s, out_i

    def search(self, query, k, id_offset=0):
        assert query.is_cuda and query.dtype == torch.float32 and query.dim() == 2 and query.shape[1] == self.docs.shape[1]
        query = query.contiguous()
        nq, dim = query.shape
        nd = self.docs.shape[0]
        L = hip.lib()
        out_s = torch.empty((nq, k), dtype=torch.float32, device=query.device)
        out_i = torch.empty((nq, k), dtype=torch.int64, device=query.device)
        if nq == 0:
            return out_s, out_i
        if self.small_image_wanted(nq, k):
            self._small_calls += 1
            if self.index8 is not None or self._small_calls > self.SMALL_BUILD_AFTER:
                return self._search_small(query, k, id_offset, out_s, out_i)
        ws_bytes = L.mevi_ip_topk_indexed_workspace_bytes(nq, dim, k)
        if ws_bytes == 0:
            raise hip.MeviHipError(f"ip_topk_indexed: unsupported shape nq={nq} dim={dim} k={k}")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=query.device)
        with hip.device_guard(query.device):
            st = L.mevi_ip_topk_indexed_f32(hip.ptr(query), nq, hip.ptr(self.docs), hip.ptr(self.index), nd, dim, k,
                                            id_offset, hip.ptr(out_s), hip.ptr(out_i), hip.ptr(ws), ws_bytes,
                                            hip.stream_ptr())
        hip.check(st, "mevi_ip_topk_indexed_f32")
        return out_s, out_i


def topk_merge(scores, ids, k_out):
    """Merge per-shard lists: scores f32[nlists,nq,k_in], ids i64[nlists,nq,k_in] -> [nq,k_out]."""
    hip.require_gpu()
    assert scores.is_cuda and ids.is_cuda and scores.shape == ids.shape and scores.dim() == 3
    scores = scores.contiguous()
    ids = ids.contiguous()
    nlists, nq, k_in = scores.shape
    L = hip.lib()
    # hierarchical merge if the flat list does not fit one LDS sort
    while nlists * k_in > 16384 and nlists > 1:
        half = (nlists + 1) // 2
        parts_s, parts_i = [], []
        for a in range(0, nlists, 2):
            s, i = topk_merge(scores[a:a + 2], ids[a:a + 2], min(k_out, 2 * k_in))
            parts_s.append(s)
            parts_i.append(i)
        k_in = parts_s[0].shape[1]
        scores, ids, nlists = torch.stack(parts_s), torch.stack(parts_i), half
    out_s = torch.empty((nq, k_out), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((nq, k_out), dtype=torch.int64, device=scores.device)
    with hip.device_guard(scores.device):
        st = L.mevi_topk_merge_f32(hip.ptr(scores), hip.ptr(ids), nlists, nq, k_in, k_out,
                                   hip.ptr(out_s), hip.ptr(out_i), None, 0, hip.stream_ptr())
    hip.check(st, "mevi_topk_merge_f32")
    return out_s, out_i


IVF_PAIR_TILE = 64                  # MEVI_IVF_SCAN_PAIR_TILE: (query, slot) pairs of a list that share one pass over its rows
IVF_ROW_BLOCK = 128                 # MEVI_IVF_SCAN_ROW_BLOCK: rows of a list per work item of the scan
IVF_WORKSPACE_CAP = (2 << 30) + (160 << 20)     # MEVI_IVF_SCAN_WORKSPACE_CAP
IVF_MAX_NPROBE = 256


def _scan_call(query, dim, list_offsets, probe, probe_score, row_ids, nd, max_list_len, k, out, workspace, workspace_bytes, *fmt):
    """What the four `*_scan_topk` wrappers share: the checks of the arguments every scan takes, `out` (allocated when None) and
    its shape, and the workspace (when None: `workspace_bytes(nq, nprobe, k, dim, *fmt, nlist, max_list_len)` bytes, the library's
    own query with the format's arguments in `fmt`; None stays None when there are no queries)."""
    assert query.is_cuda and query.dtype == torch.float32 and query.dim() == 2 and query.is_contiguous() and query.shape[1] == dim
    assert list_offsets.is_cuda and list_offsets.dtype == torch.int64 and list_offsets.is_contiguous()
    assert probe.is_cuda and probe.dtype == torch.int32 and probe.dim() == 2 and probe.is_contiguous() and probe.shape[0] == query.shape[0]
    assert probe_score is None or (probe_score.is_cuda and probe_score.dtype == torch.float32 and probe_score.is_contiguous() and
                                   probe_score.shape == probe.shape)
    assert row_ids is None or (row_ids.is_cuda and row_ids.dtype == torch.int64 and row_ids.is_contiguous() and row_ids.numel() == nd)
    nq, nlist, nprobe = query.shape[0], list_offsets.numel() - 1, probe.shape[1]
    if out is None:
        out = (torch.empty((nq, k), dtype=torch.float32, device=query.device), torch.empty((nq, k), dtype=torch.int64, device=query.device))
    out_s, out_i = out
    assert out_s.shape == (nq, k) and out_i.shape == (nq, k) and out_s.is_contiguous() and out_i.is_contiguous()
    if nq and workspace is None:
        workspace = torch.empty(workspace_bytes(nq, nprobe, k, dim, *fmt, nlist, max_list_len), dtype=torch.uint8, device=query.device)
    return nq, nlist, nprobe, out_s, out_i, workspace


def ivf_scan_workspace_bytes(nq, nprobe, k, dim, nlist, max_list_len):
    """Bytes of workspace `ivf_scan_topk` needs (host arithmetic; 0 = shape outside the kernel's envelope)."""
    return int(hip.lib().mevi_ivf_scan_workspace_bytes(nq, nprobe, k, dim, nlist, max_list_len))


def ivf_scan_query_tile(nq, nprobe, k, dim, nlist, max_list_len):
    """Queries per tile of `ivf_scan_topk` (0 = outside the envelope): each tile scans the lists it probes once more."""
    return int(hip.lib().mevi_ivf_scan_query_tile(nq, nprobe, k, dim, nlist, max_list_len))


def ivf_scan_topk(query, docs, list_offsets, row_ids, max_list_len, probe, k, out=None, workspace=None):
    """Exact top-k of every query among the rows of the lists its probe row names (mevi_ivf_scan_topk_f32).

    query f32 [nq, dim]; docs f32 [nd, dim] list-major; list_offsets i64 [nlist + 1] on the device; row_ids i64 [nd] or None
    (id = row); probe i32 [nq, nprobe] (entries outside [0, nlist) are empty, a repeated list counts once).
    Returns (scores f32 [nq, k] desc, ids i64 [nq, k]; ties by ascending id; -FLT_MAX / -1 padding).  Stream-ordered: with
    `out` = (scores, ids) and `workspace` (uint8, ivf_scan_workspace_bytes) preallocated nothing is allocated either."""
    hip.require_gpu()
    L = hip.lib()
    assert docs.is_cuda and docs.dtype == torch.float32 and docs.dim() == 2 and docs.is_contiguous()
    nd, dim = docs.shape
    nq, nlist, nprobe, out_s, out_i, workspace = _scan_call(query, dim, list_offsets, probe, None, row_ids, nd, max_list_len, k, out,
                                                            workspace, L.mevi_ivf_scan_workspace_bytes)
    if nq == 0:
        return out_s, out_i
    with hip.device_guard(query.device):
        st = L.mevi_ivf_scan_topk_f32(hip.ptr(query), nq, hip.ptr(docs), hip.ptr(list_offsets), None if row_ids is None else hip.ptr(row_ids),
                                      nd, nlist, max_list_len, dim, hip.ptr(probe), nprobe, k, hip.ptr(out_s), hip.ptr(out_i),
                                      hip.ptr(workspace) if workspace.numel() else None, workspace.numel(), hip.stream_ptr())
    hip.check(st, "mevi_ivf_scan_topk_f32")
    return out_s, out_i


IVFPQ_ROW_BLOCK = 1024              # MEVI_IVFPQ_SCAN_ROW_BLOCK: rows of a list per work item of the ADC scan
IVFPQ_MAX_M = 96                    # subspaces (code bytes per row) the ADC scan takes; m % 4 == 0
IVFPQ_MAX_LUT_BYTES = 96 << 10      # m * K * 4: one query's lookup table, kept in LDS by a scan workgroup


def ivfpq_scan_workspace_bytes(nq, nprobe, k, dim, m, K, nlist, max_list_len):
    """Bytes of workspace `ivfpq_scan_topk` needs (host arithmetic; 0 = shape outside the kernel's envelope); never above
    IVF_WORKSPACE_CAP."""
    return int(hip.lib().mevi_ivfpq_scan_workspace_bytes(nq, nprobe, k, dim, m, K, nlist, max_list_len))


def ivfpq_scan_query_tile(nq, nprobe, k, dim, m, K, nlist, max_list_len):
    """Queries per tile of `ivfpq_scan_topk` (0 = outside the envelope)."""
    return int(hip.lib().mevi_ivfpq_scan_query_tile(nq, nprobe, k, dim, m, K, nlist, max_list_len))


def ivfpq_scan_topk(query, codebook, codes, list_offsets, row_ids, max_list_len, probe, probe_score, k, out=None, workspace=None):
    """Top-k of every query among the rows of the lists its probe row names, scored by ADC (mevi_ivfpq_scan_topk_f32).

    query f32 [nq, dim]; codebook f32 [m, K, dim / m]; codes u8 [nd, m] list-major; list_offsets i64 [nlist + 1] on the device;
    row_ids i64 [nd] or None (id = row); probe i32 [nq, nprobe] (entries outside [0, nlist) are empty, a repeated list counts
    once, at its first slot); probe_score f32 [nq, nprobe] or None: the bias of every slot (None = +0).
    score = ((bias + lut[0][code_0]) + lut[1][code_1]) + ..., lut[j][c] = the fmaf chain <q_j, codebook[j][c]>.
    Returns (scores f32 [nq, k] desc, ids i64 [nq, k]; ties by ascending id; -FLT_MAX / -1 padding).  Stream-ordered: with
    `out` = (scores, ids) and `workspace` (uint8, ivfpq_scan_workspace_bytes) preallocated nothing is allocated either."""
    hip.require_gpu()
    L = hip.lib()
    assert codebook.is_cuda and codebook.dtype == torch.float32 and codebook.dim() == 3 and codebook.is_contiguous()
    assert codes.is_cuda and codes.dtype == torch.uint8 and codes.dim() == 2 and codes.is_contiguous() and codes.shape[1] == codebook.shape[0]
    m, K = codebook.shape[0], codebook.shape[1]
    nd, dim = codes.shape[0], m * codebook.shape[2]
    nq, nlist, nprobe, out_s, out_i, workspace = _scan_call(query, dim, list_offsets, probe, probe_score, row_ids, nd, max_list_len, k, out,
                                                            workspace, L.mevi_ivfpq_scan_workspace_bytes, m, K)
    if nq == 0:
        return out_s, out_i
    with hip.device_guard(query.device):
        st = L.mevi_ivfpq_scan_topk_f32(hip.ptr(query), nq, dim, hip.ptr(codebook), m, K, hip.ptr(codes) if nd else None,
                                        hip.ptr(list_offsets), None if row_ids is None else hip.ptr(row_ids), nd, nlist, max_list_len,
                                        hip.ptr(probe), None if probe_score is None else hip.ptr(probe_score), nprobe, k,
                                        hip.ptr(out_s), hip.ptr(out_i), hip.ptr(workspace) if workspace.numel() else None,
                                        workspace.numel(), hip.stream_ptr())
    hip.check(st, "mevi_ivfpq_scan_topk_f32")
    return out_s, out_i


AQ_LUT_QUERY_TILE = 256             # MEVI_AQ_LUT_QUERY_TILE: queries of a matrix-core tile of the additive quantiser's tables
AQ_LUT_FEW_QUERIES = 4              # MEVI_AQ_LUT_FEW_QUERIES: queries of a wave of the few-query table kernel


def aq_lut(query, codebook, out=None):
    """f32 [nq, M, K]: the additive quantiser's lookup tables (mevi_aq_lut_f32), lut[i][j][c] = the sequential fmaf chain
    <query i, codebook[j][c]> from +0 over all dim columns.  query f32 [nq, dim]; codebook f32 [M, K, dim].  Stream-ordered."""
    hip.require_gpu()
    assert query.is_cuda and query.dtype == torch.float32 and query.dim() == 2 and query.is_contiguous()
    assert codebook.is_cuda and codebook.dtype == torch.float32 and codebook.dim() == 3 and codebook.is_contiguous()
    M, K, dim = codebook.shape
    nq = query.shape[0]
    assert query.shape[1] == dim
    if out is None:
        out = torch.empty((nq, M, K), dtype=torch.float32, device=query.device)
    assert out.shape == (nq, M, K) and out.dtype == torch.float32 and out.is_contiguous()
    with hip.device_guard(query.device):
        st = hip.lib().mevi_aq_lut_f32(hip.ptr(query) if nq else None, nq, dim, hip.ptr(codebook), M, K, hip.ptr(out) if nq else None,
                                       hip.stream_ptr())
    hip.check(st, "mevi_aq_lut_f32")
    return out


def aq_scan_workspace_bytes(nq, nprobe, k, dim, M, K, nlist, max_list_len):
    """Bytes of workspace `aq_scan_topk` needs (host arithmetic; 0 = shape outside the kernel's envelope); never above
    IVF_WORKSPACE_CAP."""
    return int(hip.lib().mevi_aq_scan_workspace_bytes(nq, nprobe, k, dim, M, K, nlist, max_list_len))


def aq_scan_query_tile(nq, nprobe, k, dim, M, K, nlist, max_list_len):
    """Queries per tile of `aq_scan_topk` (0 = outside the envelope)."""
    return int(hip.lib().mevi_aq_scan_query_tile(nq, nprobe, k, dim, M, K, nlist, max_list_len))


def aq_scan_topk(query, codebook, codes, list_offsets, row_ids, max_list_len, probe, probe_score, k, out=None, workspace=None):
    """Top-k of every query among the rows of the lists its probe row names, scored by ADC over the byte codes of an additive
    (residual) quantiser (mevi_aq_scan_topk_f32).  The arguments and the result of `ivfpq_scan_topk` with codebook f32
    [M, K, dim]: lut[j][c] = the fmaf chain <q, codebook[j][c]> over the whole query, score = ((bias + lut[0][code_0]) +
    lut[1][code_1]) + ...  Stream-ordered: with `out` and `workspace` (uint8, aq_scan_workspace_bytes) nothing is allocated."""
    hip.require_gpu()
    L = hip.lib()
    assert codebook.is_cuda and codebook.dtype == torch.float32 and codebook.dim() == 3 and codebook.is_contiguous()
    assert codes.is_cuda and codes.dtype == torch.uint8 and codes.dim() == 2 and codes.is_contiguous() and codes.shape[1] == codebook.shape[0]
    M, K, dim = codebook.shape
    nd = codes.shape[0]
    nq, nlist, nprobe, out_s, out_i, workspace = _scan_call(query, dim, list_offsets, probe, probe_score, row_ids, nd, max_list_len, k, out,
                                                            workspace, L.mevi_aq_scan_workspace_bytes, M, K)
    if nq == 0:
        return out_s, out_i
    with hip.device_guard(query.device):
        st = L.mevi_aq_scan_topk_f32(hip.ptr(query), nq, dim, hip.ptr(codebook), M, K, hip.ptr(codes) if nd else None,
                                     hip.ptr(list_offsets), None if row_ids is None else hip.ptr(row_ids), nd, nlist, max_list_len,
                                     hip.ptr(probe), None if probe_score is None else hip.ptr(probe_score), nprobe, k,
                                     hip.ptr(out_s), hip.ptr(out_i), hip.ptr(workspace) if workspace.numel() else None,
                                     workspace.numel(), hip.stream_ptr())
    hip.check(st, "mevi_aq_scan_topk_f32")
    return out_s, out_i


def rq_residual(x, codebook, codes, out=None):
    """x - codebook[0][codes[:, 0]] - codebook[1][codes[:, 1]] - ... (mevi_rq_residual_f32): one rounded f32 subtraction per
    level and element, in ascending level.  x f32 [n, dim]; codebook f32 [G, K, dim]; codes i32 [n, >= G] with any row stride
    (a column slice of a wider code array is fine); out = x works in place.  A code outside [0, K) is clamped to it."""
    hip.require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
    assert codebook.is_cuda and codebook.dtype == torch.float32 and codebook.dim() == 3 and codebook.is_contiguous()
    G, K, dim = codebook.shape
    n = x.shape[0]
    assert x.shape[1] == dim and codes.is_cuda and codes.dtype == torch.int32 and codes.dim() == 2 and codes.shape[0] == n
    assert codes.shape[1] >= G and (n == 0 or codes.stride(1) == 1)
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.dtype == torch.float32 and out.is_contiguous()
    with hip.device_guard(x.device):
        st = hip.lib().mevi_rq_residual_f32(hip.ptr(x) if n else None, n, dim, hip.ptr(codebook), G, K, hip.ptr(codes) if n else None,
                                            codes.stride(0) if n else G, hip.ptr(out) if n else None, hip.stream_ptr())
    hip.check(st, "mevi_rq_residual_f32")
    return out


def rq_errbeam_step_workspace_bytes(n, dim, K, B, L):
    """Bytes of workspace `rq_errbeam_step` needs (host arithmetic, independent of n; 0 = outside the kernel's envelope)."""
    return int(hip.lib().mevi_rq_errbeam_step_workspace_bytes(n, dim, K, B, L))


def rq_errbeam_step_tile_docs(dim, K, B, L):
    """Documents a workgroup of `rq_errbeam_step` draws per ticket (0 = outside the envelope)."""
    return int(hip.lib().mevi_rq_errbeam_step_tile_docs(dim, K, B, L))


def rq_errbeam_step(res_in, centroids, L, res_out=None, want_res=True, workspace=None):
    """One level of the residual quantiser's beam-search encoder (mevi_rq_errbeam_step_f32): res_in f32 [n, B, dim], the B residual
    rows of every document; centroids f32 [K, dim].  -> (parent u8 [n, Lo], code u8 [n, Lo], err f32 [n, Lo], res_out f32
    [n, Lo, dim] or None), Lo = min(L, B * K): the Lo extensions of smallest reconstruction error in ascending (err, b * K + c)
    order and, unless `want_res` is False (the last level), their residual rows res_in[parent] - centroids[code].  `res_out` may
    be given (it must not overlap res_in); with it and `workspace` (uint8, rq_errbeam_step_workspace_bytes) only the three small
    outputs are allocated.  Stream-ordered."""
    hip.require_gpu()
    assert res_in.is_cuda and res_in.dtype == torch.float32 and res_in.dim() == 3 and res_in.is_contiguous()
    assert centroids.is_cuda and centroids.dtype == torch.float32 and centroids.dim() == 2 and centroids.is_contiguous()
    n, B, dim = res_in.shape
    K = centroids.shape[0]
    assert centroids.shape[1] == dim and B >= 1 and K >= 1
    Lo = min(int(L), B * K)
    dev = res_in.device
    parent = torch.empty((n, Lo), dtype=torch.uint8, device=dev)
    code = torch.empty((n, Lo), dtype=torch.uint8, device=dev)
    err = torch.empty((n, Lo), dtype=torch.float32, device=dev)
    if not want_res:
        res_out = None
    elif res_out is None:
        res_out = torch.empty((n, Lo, dim), dtype=torch.float32, device=dev)
    else:
        assert res_out.shape == (n, Lo, dim) and res_out.dtype == torch.float32 and res_out.is_contiguous() and res_out.is_cuda
    if workspace is None:
        workspace = torch.empty(max(1, rq_errbeam_step_workspace_bytes(n, dim, K, B, L)), dtype=torch.uint8, device=dev)
    with hip.device_guard(dev):
        # (an empty tensor has no address to hand over: the centroids stand in, nothing is read)
        st = hip.lib().mevi_rq_errbeam_step_f32(hip.ptr(res_in) if n else hip.ptr(centroids), n, B, dim, hip.ptr(centroids), K, L,
                                                hip.ptr(parent) if n else hip.ptr(workspace), hip.ptr(code) if n else hip.ptr(workspace),
                                                hip.ptr(err) if n else None, hip.ptr(res_out) if n and res_out is not None else None,
                                                hip.ptr(workspace), workspace.numel(), hip.stream_ptr())
    hip.check(st, "mevi_rq_errbeam_step_f32")
    return parent, code, err, res_out


def rq_errbeam_codes(parent, code, n, out=None):
    """u8 [n, M]: the code rows of slot 0's paths (mevi_rq_errbeam_codes_u8) from the traces parent / code u8 [M, n, S] of M steps
    (level j's step wrote its [n, Lo_j] into [j, :, :Lo_j]).  `out` u8 [n, >= M] with any row stride is written in place."""
    hip.require_gpu()
    assert parent.is_cuda and parent.dtype == torch.uint8 and parent.dim() == 3 and parent.is_contiguous()
    assert code.is_cuda and code.dtype == torch.uint8 and code.shape == parent.shape and code.is_contiguous()
    M, rows, S = parent.shape
    assert rows == n and M >= 1 and S >= 1
    if out is None:
        out = torch.empty((n, M), dtype=torch.uint8, device=parent.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 2 and out.shape[0] == n and out.shape[1] >= M
    assert n == 0 or out.stride(1) == 1
    with hip.device_guard(parent.device):
        st = hip.lib().mevi_rq_errbeam_codes_u8(hip.ptr(parent) if n else None, hip.ptr(code) if n else None, M, n, S,
                                                hip.ptr(out) if n else None, out.stride(0) if n else M, hip.stream_ptr())
    hip.check(st, "mevi_rq_errbeam_codes_u8")
    return out


PQFS_ROW_BLOCK = 2048               # MEVI_PQFS_SCAN_ROW_BLOCK: rows of a list per work item of the packed 4-bit ADC scan
PQFS_MIN_M, PQFS_MAX_M = 8, 96      # subspaces (nibbles per row) that scan takes; m % 8 == 0


def pqfs_scan_workspace_bytes(nq, nprobe, k, dim, m, nlist, max_list_len):
    """Bytes of workspace `pqfs_scan_topk` needs (host arithmetic; 0 = shape outside the kernel's envelope); never above
    IVF_WORKSPACE_CAP."""
    return int(hip.lib().mevi_pqfs_scan_workspace_bytes(nq, nprobe, k, dim, m, nlist, max_list_len))


def pqfs_scan_query_tile(nq, nprobe, k, dim, m, nlist, max_list_len):
    """Queries per tile of `pqfs_scan_topk` (0 = outside the envelope)."""
    return int(hip.lib().mevi_pqfs_scan_query_tile(nq, nprobe, k, dim, m, nlist, max_list_len))


def pq4_pack(codes, out=None):
    """u8 [n, m / 2]: the 4-bit codes u8 [n, m] two to a byte, code 2t in the low nibble of byte t and code 2t + 1 in the high one;
    only the low 4 bits of an input byte are kept (mevi_pq4_pack).  One launch, stream-ordered."""
    hip.require_gpu()
    assert codes.is_cuda and codes.dtype == torch.uint8 and codes.dim() == 2 and codes.is_contiguous()
    n, m = codes.shape
    assert m % 2 == 0, m
    if out is None:
        out = torch.empty((n, m // 2), dtype=torch.uint8, device=codes.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.shape == (n, m // 2)
    with hip.device_guard(codes.device):
        st = hip.lib().mevi_pq4_pack(hip.ptr(codes) if n else None, n, m, hip.ptr(out) if n else None, hip.stream_ptr())
    hip.check(st, "mevi_pq4_pack")
    return out


def pqfs_scan_topk(query, codebook, packed, list_offsets, row_ids, max_list_len, probe, probe_score, k, out=None, workspace=None):
    """Top-k of every query among the rows of the lists its probe row names, scored by ADC over packed 4-bit codes
    (mevi_pqfs_scan_topk_f32): the bits of `ivfpq_scan_topk` over the unpacked codes with K = 16.

    query f32 [nq, dim]; codebook f32 [m, 16, dim / m]; packed u8 [nd, m / 2] list-major (`pq4_pack`); list_offsets i64
    [nlist + 1] on the device; row_ids i64 [nd] or None (id = row); probe i32 [nq, nprobe] (entries outside [0, nlist) are empty,
    a repeated list counts once, at its first slot); probe_score f32 [nq, nprobe] or None: the bias of every slot (None = +0).
    Returns (scores f32 [nq, k] desc, ids i64 [nq, k]; ties by ascending id; -FLT_MAX / -1 padding).  Stream-ordered: with
    `out` = (scores, ids) and `workspace` (uint8, pqfs_scan_workspace_bytes) preallocated nothing is allocated either."""
    hip.require_gpu()
    L = hip.lib()
    assert codebook.is_cuda and codebook.dtype == torch.float32 and codebook.dim() == 3 and codebook.is_contiguous()
    assert codebook.shape[1] == 16
    assert packed.is_cuda and packed.dtype == torch.uint8 and packed.dim() == 2 and packed.is_contiguous()
    assert packed.shape[1] * 2 == codebook.shape[0]
    m = codebook.shape[0]
    nd, dim = packed.shape[0], m * codebook.shape[2]
    nq, nlist, nprobe, out_s, out_i, workspace = _scan_call(query, dim, list_offsets, probe, probe_score, row_ids, nd, max_list_len, k, out,
                                                            workspace, L.mevi_pqfs_scan_workspace_bytes, m)
    if nq == 0:
        return out_s, out_i
    with hip.device_guard(query.device):
        st = L.mevi_pqfs_scan_topk_f32(hip.ptr(query), nq, dim, hip.ptr(codebook), m, hip.ptr(packed) if nd else None,
                                       hip.ptr(list_offsets), None if row_ids is None else hip.ptr(row_ids), nd, nlist, max_list_len,
                                       hip.ptr(probe), None if probe_score is None else hip.ptr(probe_score), nprobe, k,
                                       hip.ptr(out_s), hip.ptr(out_i), hip.ptr(workspace) if workspace.numel() else None,
                                       workspace.numel(), hip.stream_ptr())
    hip.check(st, "mevi_pqfs_scan_topk_f32")
    return out_s, out_i


SQ_MAX_DIM = 4096                   # columns a scalar-quantised row may have (include/mevi_hip_sq.h)


def sq_scan_workspace_bytes(nq, nprobe, k, dim, bits, nlist, max_list_len):
    """Bytes of workspace `sq_scan_topk` needs (host arithmetic; 0 = shape outside the kernel's envelope); never above
    IVF_WORKSPACE_CAP."""
    return int(hip.lib().mevi_sq_scan_workspace_bytes(nq, nprobe, k, dim, bits, nlist, max_list_len))


def sq_scan_query_tile(nq, nprobe, k, dim, bits, nlist, max_list_len):
    """Queries per tile of `sq_scan_topk` (0 = outside the envelope)."""
    return int(hip.lib().mevi_sq_scan_query_tile(nq, nprobe, k, dim, bits, nlist, max_list_len))


def sq_encode(x, rows, list_of, centroids, vmin, vdiff, bits, out=None):
    """u8 [n, dim * bits / 8]: the scalar-quantised codes of x[rows] (rows None: of x) in that order (mevi_sq_encode_f32).

    x f32 [n_src, dim]; rows i64 [n] or None; list_of i32 [n_src] + centroids f32 [nlist, dim] (the residual x - centroid[list of
    the source row] is what is coded) or both None; vmin, vdiff f32 [dim]; bits 4 or 8.  One pass, stream-ordered."""
    hip.require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
    assert rows is None or (rows.is_cuda and rows.dtype == torch.int64 and rows.dim() == 1 and rows.is_contiguous())
    assert (list_of is None) == (centroids is None)
    if centroids is not None:
        assert list_of.is_cuda and list_of.dtype == torch.int32 and list_of.is_contiguous() and list_of.numel() == x.shape[0]
        assert centroids.is_cuda and centroids.dtype == torch.float32 and centroids.is_contiguous() and centroids.shape[1] == x.shape[1]
    for v in (vmin, vdiff):
        assert v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.shape == (x.shape[1],)
    n_src, dim = x.shape
    n = n_src if rows is None else rows.numel()
    if out is None:
        out = torch.empty((n, dim * bits // 8), dtype=torch.uint8, device=x.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.shape == (n, dim * bits // 8)
    with hip.device_guard(x.device):
        st = hip.lib().mevi_sq_encode_f32(hip.ptr(x) if n_src else None, n_src, dim, None if rows is None else hip.ptr(rows), n,
                                          None if list_of is None else hip.ptr(list_of),
                                          None if centroids is None else hip.ptr(centroids), 0 if centroids is None else centroids.shape[0],
                                          hip.ptr(vmin), hip.ptr(vdiff), bits, hip.ptr(out) if n else None, hip.stream_ptr())
    hip.check(st, "mevi_sq_encode_f32")
    return out


def sq_scan_topk(query, codes, vmin, vdiff, bits, list_offsets, row_ids, max_list_len, probe, probe_score, k, out=None, workspace=None):
    """Top-k of every query among the rows of the lists its probe row names, every row decoded from its scalar-quantised codes
    (mevi_sq_scan_topk_f32).

    query f32 [nq, dim]; codes u8 [nd, dim * bits / 8] list-major; vmin, vdiff f32 [dim]; bits 4 or 8; list_offsets i64 [nlist + 1]
    on the device; row_ids i64 [nd] or None (id = row); probe i32 [nq, nprobe] (entries outside [0, nlist) are empty, a repeated
    list counts once, at its first slot); probe_score f32 [nq, nprobe] or None: the bias of every slot (None: no addition).
    score = the fmaf chain <q, vmin + vdiff * T[code]> (+ bias): the bits `ivf_scan_topk` gives over the decoded rows.
    Returns (scores f32 [nq, k] desc, ids i64 [nq, k]; ties by ascending id; -FLT_MAX / -1 padding).  Stream-ordered: with
    `out` = (scores, ids) and `workspace` (uint8, sq_scan_workspace_bytes) preallocated nothing is allocated either."""
    hip.require_gpu()
    L = hip.lib()
    assert bits in (4, 8)
    assert codes.is_cuda and codes.dtype == torch.uint8 and codes.dim() == 2 and codes.is_contiguous()
    nd, dim = codes.shape[0], codes.shape[1] * 8 // bits
    for v in (vmin, vdiff):
        assert v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.shape == (dim,)
    nq, nlist, nprobe, out_s, out_i, workspace = _scan_call(query, dim, list_offsets, probe, probe_score, row_ids, nd, max_list_len, k, out,
                                                            workspace, L.mevi_sq_scan_workspace_bytes, bits)
    if nq == 0:
        return out_s, out_i
    with hip.device_guard(query.device):
        st = L.mevi_sq_scan_topk_f32(hip.ptr(query), nq, dim, hip.ptr(codes) if nd else None, hip.ptr(vmin), hip.ptr(vdiff), bits,
                                     hip.ptr(list_offsets), None if row_ids is None else hip.ptr(row_ids), nd, nlist, max_list_len,
                                     hip.ptr(probe), None if probe_score is None else hip.ptr(probe_score), nprobe, k,
                                     hip.ptr(out_s), hip.ptr(out_i), hip.ptr(workspace) if workspace.numel() else None,
                                     workspace.numel(), hip.stream_ptr())
    hip.check(st, "mevi_sq_scan_topk_f32")
    return out_s, out_i


OPQ_MAX_DIM = 4096                  # columns a rotated row may have (include/mevi_hip_opq.h)


def opq_rotate_rows(x, rows, list_of, crot, R, out=None, mode=None):
    """f32 [n, dim]: out[i] = chain(x[rows[i]], R) - crot[list_of[rows[i]]] (rows None: row i; list_of and crot both None: no
    subtraction), chain = the sequential fmaf chain of `ops.linear` and the subtraction one f32 operation
    (mevi_opq_rotate_rows_f32: one launch, stream-ordered, nothing but `out` is written).

    x f32 [n_src, dim]; rows i64 [n] or None; list_of i32 [n_src] + crot f32 [nlist, dim] or both None; R f32 [dim, dim] in the
    nn.Linear layout.  A row id outside [0, n_src) or a list outside [0, nlist) gives a row of zeros.
    mode (default: MEVI_OPQ_ROTATE or 'fused') = 'steps' composes existing calls instead -- gather, `ops.linear`, gather of crot,
    subtract: the same bits through three more passes over the chunk (the A/B partner and the reference of the tests)."""
    hip.require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
    assert rows is None or (rows.is_cuda and rows.dtype == torch.int64 and rows.dim() == 1 and rows.is_contiguous())
    assert (list_of is None) == (crot is None)
    n_src, dim = x.shape
    if crot is not None:
        assert list_of.is_cuda and list_of.dtype == torch.int32 and list_of.is_contiguous() and list_of.numel() == n_src
        assert crot.is_cuda and crot.dtype == torch.float32 and crot.is_contiguous() and crot.dim() == 2 and crot.shape[1] == dim
    assert R.is_cuda and R.dtype == torch.float32 and R.is_contiguous() and R.shape == (dim, dim)
    n = n_src if rows is None else rows.numel()
    if out is None:
        out = torch.empty((n, dim), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == (n, dim)
    if mode is None:
        mode = os.environ.get("MEVI_OPQ_ROTATE", "fused")
    if mode not in ("fused", "steps"):
        raise ValueError(f"MEVI_OPQ_ROTATE={mode!r} is neither 'fused' nor 'steps'")
    if mode == "steps":
        if n == 0:
            return out
        from . import ops

        src = torch.arange(n, dtype=torch.int64, device=x.device) if rows is None else rows
        ok = (src >= 0) & (src < n_src)
        src = torch.where(ok, src, torch.zeros_like(src))
        if n_src == 0:
            return out.zero_()
        with hip.device_guard(x.device):
            ops.linear(x[src], R, out=out)
        if crot is not None:
            lst = list_of[src].long()
            ok &= (lst >= 0) & (lst < crot.shape[0])
            torch.sub(out, crot[torch.where(ok, lst, torch.zeros_like(lst))], out=out)
        return out.masked_fill_(~ok[:, None], 0.0)
    with hip.device_guard(x.device):
        st = hip.lib().mevi_opq_rotate_rows_f32(hip.ptr(x) if n_src else None, n_src, dim, None if rows is None else hip.ptr(rows), n,
                                                None if list_of is None else hip.ptr(list_of), None if crot is None else hip.ptr(crot),
                                                0 if crot is None else crot.shape[0], hip.ptr(R), hip.ptr(out) if n else None,
                                                hip.stream_ptr())
    hip.check(st, "mevi_opq_rotate_rows_f32")
    return out


REFINE_WORKSPACE_CAP = 32 << 20     # MEVI_REFINE_TOPK_WORKSPACE_CAP
REFINE_MAX_CAND = 16384             # MEVI_REFINE_TOPK_MAX_CAND: candidates of one query (the places of the LDS sort)


def refine_topk_workspace_bytes(nq, n_cand, k, dim):
    """Bytes of workspace `refine_topk` needs (host arithmetic; 0 = shape outside the call's envelope)."""
    return int(hip.lib().mevi_refine_topk_workspace_bytes(nq, n_cand, k, dim))


def refine_topk_query_tile(nq, n_cand, k, dim):
    """Queries per tile of `refine_topk` (0 = outside the envelope): two launches per tile."""
    return int(hip.lib().mevi_refine_topk_query_tile(nq, n_cand, k, dim))


def refine_topk(query, docs, cand, k, out=None, workspace=None):
    """The best k of every query's candidate ids by exact score (mevi_refine_topk_f32): faiss IndexRefineFlat's second stage.

    query f32 [nq, dim] and cand i64 [nq, n_cand] may be row-strided views (unit stride inside a row, the query's row stride a
    multiple of 4); docs f32 [nd, dim] contiguous.  An id outside [0, nd) -- the scans' -1 padding -- is skipped, a repeated id is
    listed twice.  Returns (scores f32 [nq, k] desc, ids i64 [nq, k], nvalid i32 [nq]): the scores are the bits of the exact search,
    ties by ascending id, -FLT_MAX / -1 padding.  Stream-ordered: with `out` = (scores, ids, nvalid) and `workspace` (uint8,
    refine_topk_workspace_bytes) preallocated nothing is allocated either."""
    hip.require_gpu()
    L = hip.lib()
    assert query.is_cuda and query.dtype == torch.float32 and query.dim() == 2 and (query.shape[0] < 2 or query.stride(0) >= query.shape[1])
    assert docs.is_cuda and docs.dtype == torch.float32 and docs.dim() == 2 and docs.is_contiguous() and docs.shape[1] == query.shape[1]
    assert cand.is_cuda and cand.dtype == torch.int64 and cand.dim() == 2 and cand.shape[0] == query.shape[0]
    assert (query.shape[1] < 2 or query.stride(1) == 1) and (cand.shape[1] < 2 or cand.stride(1) == 1)
    nq, dim = query.shape
    nd, n_cand = docs.shape[0], cand.shape[1]
    ldq = query.stride(0) if nq > 1 else dim
    ld_cand = cand.stride(0) if nq > 1 else n_cand
    if out is None:
        out = (torch.empty((nq, k), dtype=torch.float32, device=query.device), torch.empty((nq, k), dtype=torch.int64, device=query.device),
               torch.empty((nq,), dtype=torch.int32, device=query.device))
    out_s, out_i, out_n = out
    assert out_s.shape == (nq, k) and out_i.shape == (nq, k) and out_s.is_contiguous() and out_i.is_contiguous()
    assert out_s.dtype == torch.float32 and out_i.dtype == torch.int64
    assert out_n is None or (out_n.shape == (nq,) and out_n.dtype == torch.int32 and out_n.is_contiguous())
    if nq and workspace is None:
        need = L.mevi_refine_topk_workspace_bytes(nq, n_cand, k, dim)
        if need == 0:
            raise hip.MeviHipError(f"refine_topk: unsupported shape nq={nq} n_cand={n_cand} k={k} dim={dim}")
        workspace = torch.empty(need, dtype=torch.uint8, device=query.device)
    with hip.device_guard(query.device):
        st = L.mevi_refine_topk_f32(hip.ptr(query) if nq else None, ldq, nq, hip.ptr(docs) if nd else None, nd, dim,
                                    hip.ptr(cand) if nq else None, ld_cand, n_cand, k, hip.ptr(out_s) if nq else None,
                                    hip.ptr(out_i) if nq else None, None if out_n is None or not nq else hip.ptr(out_n),
                                    hip.ptr(workspace) if nq else None, workspace.numel() if nq else 0, hip.stream_ptr())
    hip.check(st, "mevi_refine_topk_f32")
    return out_s, out_i, out_n


GRAPH_MAX_EF = 4096                 # MEVI_GRAPH_MAX_EF: entries of a walk's candidate list
GRAPH_MAX_BATCH = 2048              # MEVI_GRAPH_MAX_BATCH: width * degree, the ids one step of a walk reads
GRAPH_LINK_MIN_ROWS = 4096          # MEVI_GRAPH_LINK_MIN_ROWS: destination rows the smallest link workspace holds


def graph_link_workspace_bytes(nd, C, M):
    """Bytes of the smallest workspace `graph_link` takes (host arithmetic; 0 = outside the envelope)."""
    return int(hip.lib().mevi_graph_link_workspace_bytes(nd, C, M))


def graph_link(knn, M, workspace=None):
    """graph i32 [nd, 2 * M] from knn i64 [nd, C] (mevi_graph_link, include/mevi_hip_graph.h): the first M distinct valid others
    of every list, then the reverse links in ascending (rank, source) order, -1 padding.  Any workspace of at least
    graph_link_workspace_bytes gives the same graph; a larger one walks the destination rows in fewer ranges."""
    hip.require_gpu()
    assert knn.is_cuda and knn.dtype == torch.int64 and knn.dim() == 2 and knn.is_contiguous()
    nd, C = knn.shape
    graph = torch.empty((nd, 2 * M), dtype=torch.int32, device=knn.device)
    if nd == 0:
        return graph
    L = hip.lib()
    if workspace is None:
        need = L.mevi_graph_link_workspace_bytes(nd, C, M)
        workspace = torch.empty(max(need, min(nd * 2 * M * 8, 1 << 30)) if need else 0, dtype=torch.uint8, device=knn.device)
    with hip.device_guard(knn.device):
        st = L.mevi_graph_link(hip.ptr(knn), nd, C, M, hip.ptr(graph), hip.ptr(workspace) if workspace.numel() else None,
                               workspace.numel(), hip.stream_ptr())
    hip.check(st, "mevi_graph_link")
    return graph


def graph_search_workspace_bytes(nq, dim, degree, nseed, k, ef, width, max_steps):
    """Bytes of workspace `graph_search_topk` needs (host arithmetic; 0 = outside the kernel's envelope)."""
    return int(hip.lib().mevi_graph_search_workspace_bytes(nq, dim, degree, nseed, k, ef, width, max_steps))


def graph_search_topk(query, docs, graph, seed, seed_score, k, ef, width=1, max_steps=None, out=None, workspace=None, steps=None):
    """Best-first search over a neighbour graph (mevi_graph_search_topk_f32, include/mevi_hip_graph.h).

    query f32 [nq, dim]; docs f32 [nd, dim]; graph i32 [nd, degree]; seed i32 [nq, nseed]; seed_score f32 [nq, nseed] or None
    (the seeds are scored); a candidate list of `ef` entries, `width` entries expanded per step, at most `max_steps` steps
    (default 4 * ef).  `steps` i32 [nq] or None receives the steps taken.  Returns (scores f32 [nq, k] desc, ids i64 [nq, k];
    ties by ascending id; -FLT_MAX / -1 padding).  After the call the first nq u32 of `workspace` hold the rows every walk scored.
    Stream-ordered: with `out` and `workspace` (uint8, graph_search_workspace_bytes) preallocated nothing is allocated either."""
    hip.require_gpu()
    assert query.is_cuda and query.dtype == torch.float32 and query.dim() == 2 and query.is_contiguous()
    assert docs.is_cuda and docs.dtype == torch.float32 and docs.dim() == 2 and docs.is_contiguous() and docs.shape[1] == query.shape[1]
    assert graph.is_cuda and graph.dtype == torch.int32 and graph.dim() == 2 and graph.is_contiguous() and graph.shape[0] == docs.shape[0]
    assert seed.is_cuda and seed.dtype == torch.int32 and seed.dim() == 2 and seed.is_contiguous() and seed.shape[0] == query.shape[0]
    assert seed_score is None or (seed_score.is_cuda and seed_score.dtype == torch.float32 and seed_score.is_contiguous() and
                                  seed_score.shape == seed.shape)
    assert steps is None or (steps.is_cuda and steps.dtype == torch.int32 and steps.is_contiguous() and steps.numel() == query.shape[0])
    nq, dim = query.shape
    nd, degree, nseed = docs.shape[0], graph.shape[1], seed.shape[1]
    if max_steps is None:
        max_steps = 4 * ef
    L = hip.lib()
    if out is None:
        out = (torch.empty((nq, k), dtype=torch.float32, device=query.device), torch.empty((nq, k), dtype=torch.int64, device=query.device))
    out_s, out_i = out
    assert out_s.shape == (nq, k) and out_i.shape == (nq, k) and out_s.is_contiguous() and out_i.is_contiguous()
    if nq == 0:
        return out_s, out_i
    if workspace is None:
        workspace = torch.empty(L.mevi_graph_search_workspace_bytes(nq, dim, degree, nseed, k, ef, width, max_steps), dtype=torch.uint8,
                                device=query.device)
    with hip.device_guard(query.device):
        st = L.mevi_graph_search_topk_f32(hip.ptr(query), nq, dim, hip.ptr(docs) if nd else None, nd, hip.ptr(graph) if nd else None,
                                          degree, hip.ptr(seed), None if seed_score is None else hip.ptr(seed_score), nseed, k, ef,
                                          width, max_steps, hip.ptr(out_s), hip.ptr(out_i), None if steps is None else hip.ptr(steps),
                                          hip.ptr(workspace) if workspace.numel() else None, workspace.numel(), hip.stream_ptr())
    hip.check(st, "mevi_graph_search_topk_f32")
    return out_s, out_i


GRAPH_MAX_LEVELS = 8                # MEVI_GRAPH_MAX_LEVELS: walked upper levels of one descent
GRAPH_DESCEND_MAX_EF = 256          # MEVI_GRAPH_DESCEND_MAX_EF: entries of the descent's candidate list


def graph_descend_workspace_bytes(nq, dim, degree, n_levels, nseed_in, nseed_out, ef, width, max_steps):
    """Bytes of workspace `graph_descend` needs (host arithmetic; 0 = outside the kernel's envelope)."""
    return int(hip.lib().mevi_graph_descend_workspace_bytes(nq, dim, degree, n_levels, nseed_in, nseed_out, ef, width, max_steps))


def graph_descend(query, docs, graphs, rows, down, level_n, seed, seed_score, ef, width=1, max_steps=None, nseed_out=None, out=None,
                  workspace=None, steps=None):
    """The descent through the upper levels of a neighbour-graph index (mevi_graph_descend_f32, include/mevi_hip_graph_levels.h).

    query f32 [nq, dim]; docs f32 [nd, dim]; graphs i32 [sum n_l, degree], rows i32 [sum n_l], down i32 [sum n_l]: the walked
    levels concatenated, level 1 first, local ids; level_n: their sizes, a sequence of ints on the host; seed i64 [nq, nseed_in]
    local ids of the last level with seed_score f32, as `ivf_scan_topk` returns them.  Per level a walk with a list of `ef`
    entries, `width` entries expanded per step and at most `max_steps` steps (default 4 * ef); the best `nseed_out` (default
    min(ef, 32)) entries go one level down.  Returns (seed i32 [nq, nseed_out], score f32 [nq, nseed_out]): the `seed` and
    `seed_score` of `graph_search_topk`, -1 / -FLT_MAX padding.  `steps` i32 [nq] or None receives the steps of all levels; after
    the call the first nq u32 of `workspace` hold the rows every descent scored.  Stream-ordered: with `out` and `workspace`
    (uint8, graph_descend_workspace_bytes) preallocated nothing is allocated either."""
    import ctypes

    hip.require_gpu()
    assert query.is_cuda and query.dtype == torch.float32 and query.dim() == 2 and query.is_contiguous()
    assert docs.is_cuda and docs.dtype == torch.float32 and docs.dim() == 2 and docs.is_contiguous() and docs.shape[1] == query.shape[1]
    level_n = [int(n) for n in level_n]
    total = sum(level_n)
    assert graphs.is_cuda and graphs.dtype == torch.int32 and graphs.dim() == 2 and graphs.is_contiguous() and graphs.shape[0] == total
    for m in (rows, down):
        assert m.is_cuda and m.dtype == torch.int32 and m.dim() == 1 and m.is_contiguous() and m.numel() == total
    assert seed.is_cuda and seed.dtype == torch.int64 and seed.dim() == 2 and seed.is_contiguous() and seed.shape[0] == query.shape[0]
    assert seed_score.is_cuda and seed_score.dtype == torch.float32 and seed_score.is_contiguous() and seed_score.shape == seed.shape
    assert steps is None or (steps.is_cuda and steps.dtype == torch.int32 and steps.is_contiguous() and steps.numel() == query.shape[0])
    nq, dim = query.shape
    nd, degree, nseed_in = docs.shape[0], graphs.shape[1], seed.shape[1]
    if max_steps is None:
        max_steps = 4 * ef
    if nseed_out is None:
        nseed_out = min(ef, 32)
    L = hip.lib()
    if out is None:
        out = (torch.empty((nq, nseed_out), dtype=torch.int32, device=query.device),
               torch.empty((nq, nseed_out), dtype=torch.float32, device=query.device))
    out_i, out_s = out
    assert out_i.shape == (nq, nseed_out) and out_s.shape == (nq, nseed_out) and out_i.is_contiguous() and out_s.is_contiguous()
    assert out_i.dtype == torch.int32 and out_s.dtype == torch.float32
    if nq == 0:
        return out_i, out_s
    if workspace is None:
        workspace = torch.empty(L.mevi_graph_descend_workspace_bytes(nq, dim, degree, len(level_n), nseed_in, nseed_out, ef, width, max_steps),
                                dtype=torch.uint8, device=query.device)
    sizes = (ctypes.c_int64 * max(1, len(level_n)))(*level_n)               # read by the call before it launches
    with hip.device_guard(query.device):
        st = L.mevi_graph_descend_f32(hip.ptr(query), nq, dim, hip.ptr(docs) if nd else None, nd, hip.ptr(graphs), degree, hip.ptr(rows),
                                      hip.ptr(down), ctypes.addressof(sizes), len(level_n), hip.ptr(seed), hip.ptr(seed_score), nseed_in,
                                      ef, width, max_steps, nseed_out, hip.ptr(out_i), hip.ptr(out_s),
                                      None if steps is None else hip.ptr(steps), hip.ptr(workspace) if workspace.numel() else None,
                                      workspace.numel(), hip.stream_ptr())
    hip.check(st, "mevi_graph_descend_f32")
    return out_i, out_s


IVF_ASSIGN_ROWS = 256               # MEVI_IVF_ASSIGN_ROWS: rows a workgroup of `ivf_assign` keeps while it walks the centroids
IVF_ASSIGN_COLS = 128               # MEVI_IVF_ASSIGN_COLS: centroids per tile of that walk (64 on grids too small for the device)
IVF_ASSIGN_SPLIT_WGS = 256          # MEVI_IVF_ASSIGN_SPLIT_WGS: below this many row blocks the walk is split among workgroups
IVF_BUILD_MAX_NLIST = 262144        # MEVI_IVF_BUILD_MAX_NLIST
IVF_LISTS_TILE = 2048               # MEVI_IVF_LISTS_TILE: rows per workgroup of `ivf_build_lists`


def ivf_assign_workspace_bytes(n, dim, nlist):
    """Bytes of workspace `ivf_assign` needs (host arithmetic; 0 = shape outside the kernel's envelope)."""
    return int(hip.lib().mevi_ivf_assign_workspace_bytes(n, dim, nlist))


def ivf_build_lists_workspace_bytes(n, nlist):
    """Bytes of workspace `ivf_build_lists` needs (host arithmetic; 0 = outside the envelope)."""
    return int(hip.lib().mevi_ivf_build_lists_workspace_bytes(n, nlist))


def ivf_assign(x, centroids, out=None, workspace=None):
    """Nearest centroid by inner product per row (mevi_ivf_assign_f32): no [n, nlist] score matrix.

    x f32 [n, dim], centroids f32 [nlist, dim].  Returns (list_of i32 [n], best_score f32 [n]): the lowest c that attains
    max_c <x_r, centroid_c> (sequential fmaf chains, the bits of `ip_topk` and `ops.linear`) and that maximum.  `out` =
    (list_of, best_score or None) and `workspace` (uint8, ivf_assign_workspace_bytes) preallocated: nothing is allocated."""
    hip.require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
    assert centroids.is_cuda and centroids.dtype == torch.float32 and centroids.dim() == 2 and centroids.is_contiguous()
    assert centroids.shape[1] == x.shape[1]
    n, dim = x.shape
    nlist = centroids.shape[0]
    L = hip.lib()
    if out is None:
        out = (torch.empty(n, dtype=torch.int32, device=x.device), torch.empty(n, dtype=torch.float32, device=x.device))
    list_of, best = out
    assert list_of.dtype == torch.int32 and list_of.shape == (n,) and list_of.is_contiguous() and list_of.is_cuda
    assert best is None or (best.dtype == torch.float32 and best.shape == (n,) and best.is_contiguous() and best.is_cuda)
    if workspace is None and n:
        workspace = torch.empty(L.mevi_ivf_assign_workspace_bytes(n, dim, nlist), dtype=torch.uint8, device=x.device)
    with hip.device_guard(x.device):
        st = L.mevi_ivf_assign_f32(hip.ptr(x), n, dim, hip.ptr(centroids), nlist, hip.ptr(list_of), None if best is None else hip.ptr(best),
                                   hip.ptr(workspace) if workspace is not None and workspace.numel() else None,
                                   0 if workspace is None else workspace.numel(), hip.stream_ptr())
    hip.check(st, "mevi_ivf_assign_f32")
    return list_of, best


def ivf_build_lists(list_of, nlist, workspace=None):
    """Labels -> inverted lists (mevi_ivf_build_lists): (list_offsets i64 [nlist + 1], row_ids i64 [n], max_list_len i64 [1]),
    all on the device.  row_ids = the rows ordered by (list, row), i.e. torch.argsort(list_of, stable=True); a label outside
    [0, nlist) leaves its row out: list_offsets[nlist] counts the listed rows, the slots of row_ids beyond it are not written."""
    hip.require_gpu()
    assert list_of.is_cuda and list_of.dtype == torch.int32 and list_of.dim() == 1 and list_of.is_contiguous()
    n = list_of.numel()
    dev = list_of.device
    L = hip.lib()
    offsets = torch.empty(nlist + 1, dtype=torch.int64, device=dev)
    row_ids = torch.empty(n, dtype=torch.int64, device=dev)
    longest = torch.empty(1, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(L.mevi_ivf_build_lists_workspace_bytes(n, nlist), dtype=torch.uint8, device=dev)
    with hip.device_guard(dev):
        st = L.mevi_ivf_build_lists(hip.ptr(list_of) if n else None, n, nlist, hip.ptr(offsets), hip.ptr(row_ids) if n else None,
                                    hip.ptr(longest), hip.ptr(workspace) if workspace.numel() else None, workspace.numel(),
                                    hip.stream_ptr())
    hip.check(st, "mevi_ivf_build_lists")
    return offsets, row_ids, longest


def shard_range(n_rows, rank, world_size):
    """Contiguous row shard [start, end) of rank: ceil(n/world) rows each."""
    per = (n_rows + world_size - 1) // world_size
    start = min(rank * per, n_rows)
    return start, min(start + per, n_rows)


def truncated_list_len(k, world):
    """Entries each shard contributes in the first round of a sharded search.  With rows spread evenly a
    shard holds Binomial(k, 1/world) of the global top-k: mean k/world, deviation < sqrt(k/world); five
    deviations + 8 of head-room (W = 8, k = 1000: 193 entries, 6.5 actual deviations: < 1e-9 per query and
    shard) make a second round rare, and the proof in merge_truncated catches the rest.  The per-rank costs
    that do not shrink with the shard (re-scoring K' = k_local + slack survivors, compaction, the all-gather
    payload, the merge) are all proportional to this length."""
    if world <= 1:
        return k
    share = (k + world - 1) // world
    sig = float(os.environ.get("MEVI_SHARD_HEADROOM_SIGMAS", "5"))
    return min(k, share + int(np.ceil(sig * np.ceil(np.sqrt(share)))) + 8)


def merge_truncated(all_s, all_i, k, merge=None):
    """Merge per-shard lists that may have been TRUNCATED to k_local < k entries and decide, per query,
    whether the merged top-k is provably the un-sharded answer.

    all_s f32[world, nq, k_local], all_i i64[world, nq, k_local] (id -1 = padding: that shard is exhausted).
    A shard's unseen rows all rank after its last returned entry, so the merged list is exact unless some
    shard's LAST entry made it into the merged top-k (then deeper rows of that shard might belong too).
    Returns (scores [nq, k], ids [nq, k], unproven bool[nq])."""
    merge = merge or topk_merge
    world, nq, kl = all_s.shape
    ms, mi = merge(all_s, all_i, k)
    last_s, last_i = all_s[:, :, kl - 1], all_i[:, :, kl - 1]          # [world, nq]
    kth_s, kth_i = ms[:, k - 1], mi[:, k - 1]                           # [nq]
    # kth_i == -1: fewer than k rows exist in total -> every returned row is already in the list
    in_topk = (last_i >= 0) & (kth_i[None] >= 0) & (
        (last_s > kth_s[None]) | ((last_s == kth_s[None]) & (last_i <= kth_i[None])))
    truncated = kl < k
    unproven = in_topk.any(0) if truncated else torch.zeros(nq, dtype=torch.bool, device=ms.device)
    return ms, mi, unproven


def pack_lists(scores, ids):
    """(scores f32 [..], ids i64 [..]) -> i64 [..]: score bits << 32 | id as u32 -- the 8-byte wire format of the exchange."""
    scores, ids = scores.contiguous(), ids.contiguous()
    if not scores.is_cuda:       # the gloo CPU tests inject their own search / merge; same format
        return (scores.view(torch.int32).to(torch.int64) << 32) | (ids & 0xFFFFFFFF)
    out = torch.empty(scores.shape, dtype=torch.int64, device=scores.device)
    with hip.device_guard(scores.device):
        hip.check(hip.lib().mevi_pack_lists_i64(hip.ptr(scores), hip.ptr(ids), scores.numel(), hip.ptr(out), hip.stream_ptr()),
                  "mevi_pack_lists_i64")
    return out


def unpack_lists(packed):
    all_s = (packed >> 32).to(torch.int32).view(torch.float32)
    all_i = packed & 0xFFFFFFFF
    return all_s, torch.where(all_i == 0xFFFFFFFF, torch.full_like(all_i, -1), all_i)


def merge_packed(gathered, k):
    """merge_truncated on the all-gathered wire format, in ONE kernel (mevi_topk_merge_packed_f32): gathered i64
    [world, nq, k_local], every list sorted as the local searches return them.  Returns (scores, ids, unproven bool[nq])."""
    world, nq, kl = gathered.shape
    out_s = torch.empty((nq, k), dtype=torch.float32, device=gathered.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=gathered.device)
    unproven = torch.zeros(nq, dtype=torch.uint8, device=gathered.device)
    with hip.device_guard(gathered.device):
        st = hip.lib().mevi_topk_merge_packed_f32(hip.ptr(gathered), world, nq, kl, k, 1 if kl < k else 0, hip.ptr(out_s),
                                                  hip.ptr(out_i), hip.ptr(unproven), hip.stream_ptr())
    hip.check(st, "mevi_topk_merge_packed_f32")
    return out_s, out_i, unproven.bool()


def _packed_merge_fits(world, kl, k):
    lp = 32
    while lp < kl:
        lp <<= 1
    return world <= 64 and world * lp <= 16384 and k <= 16384


class SearchTrace:
    """What bench.py asks a search to record (never set by the CLIs): the kernel counters of EVERY local search of a call
    (mevi_ip_topk_get_stats restarts per library call, so a second round would otherwise overwrite the first) and,
    with `timed`, the wall-clock of each phase of the sharded search -- every phase is then followed by a device
    synchronisation, so a traced call is for diagnosis, not for the timed region."""

    FIELDS = ("n_chunks", "n_failed_queries", "n_fallback_chunks", "filter_ms", "compact_ms", "filter_flops",
              "n_second_pass_queries")

    def __init__(self, timed=False):
        self.timed = timed
        self.stats = {f: 0.0 for f in self.FIELDS}
        self.ms = {"local_search": 0.0, "all_gather": 0.0, "merge": 0.0}
        self.second_round_queries = 0
        self.rounds = 0

    def add_stats(self):
        st = hip.IpTopkStats()
        hip.lib().mevi_ip_topk_get_stats(st)
        for f in self.FIELDS:
            self.stats[f] += getattr(st, f)

    def lap(self, name, t0):
        import time

        if not self.timed:
            return t0
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        self.ms[name] += (t1 - t0) * 1e3
        return t1


def sharded_ip_topk(query, local_docs, k, id_offset, group=None, local_search=None, merge=None, trace=None):
    """Row-sharded search: local top lists with global ids, all-gather, merge.

    Every rank passes the full (replicated) query matrix and its own shard; every rank returns the
    identical merged (scores, ids), equal to the un-sharded search whatever the shard count.
    Round 1 exchanges only k_local = truncated_list_len(k, world) entries per shard -- k/world + 5 sqrt(k/world) + 8
    (193 at k = 1000, world = 8; MEVI_SHARD_HEADROOM_SIGMAS overrides the 5) -- so per-rank re-scoring, compaction
    and the all-gather shrink with the world size; queries whose merged list cannot be proven complete (a shard's
    last entry reached the global top-k) are repeated with full k-entry lists -- every rank takes the same decision
    from the same gathered data.  The binomial head-room assumes the top-k rows are spread evenly over the shards; a
    corpus stored cluster by cluster concentrates them, the second round then runs for most queries (correct, but a
    second search + all-gather): `trace.second_round_queries` reports it, bench.py prints it for N > 1, and
    tools/bench_shard_sim.py --layout sorted measures that case.
    `local_search` / `merge` default to the HIP kernels; they are injection points for the CPU (gloo)
    test of the collective plumbing and are never set by product code.
    """
    import time

    import torch.distributed as dist

    def local(q, kk):
        if local_search is not None:
            return local_search(q, local_docs, kk, id_offset=id_offset)
        if isinstance(local_docs, DenseIndex):
            out = local_docs.search(q, kk, id_offset=id_offset)
        else:
            out = ip_topk(q, local_docs, kk, id_offset=id_offset)
        if trace is not None:
            trace.add_stats()
        return out

    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return local(query, k)
    world = dist.get_world_size(group)

    def exchange(q, kk):
        # one collective per round: (score bits << 32 | id as u32) in an i64 per entry -- 8 bytes instead of the 12
        # of separate f32 + i64 tensors, and half the launches.  Ids fit 32 bits (the C ABI enforces it); the
        # padding id -1 travels as 0xFFFFFFFF.
        t0 = time.perf_counter() if trace is not None else 0.0
        s, i = local(q, kk)
        if trace is not None:
            t0 = trace.lap("local_search", t0)
            trace.rounds += 1
        n = s.shape[0]
        packed = pack_lists(s, i)
        if packed.is_cuda and dist.get_backend(group) == "gloo":     # rehearsal backend: collectives through host memory
            host = torch.empty((world * n, kk), dtype=torch.int64)
            dist.all_gather_into_tensor(host, packed.cpu().contiguous(), group=group)
            gathered = host.to(s.device)
        else:
            gathered = torch.empty((world * n, kk), dtype=torch.int64, device=s.device)   # rank-major concatenation
            dist.all_gather_into_tensor(gathered, packed.contiguous(), group=group)
        if trace is not None:
            trace.lap("all_gather", t0)
        return gathered.view(world, n, kk)

    def merged(q, kk):
        gathered = exchange(q, kk)
        t0 = time.perf_counter() if trace is not None else 0.0
        if merge is None and gathered.is_cuda and _packed_merge_fits(world, kk, k):
            out = merge_packed(gathered, k)                          # unpack + merge + proof in one kernel
        else:
            all_s, all_i = unpack_lists(gathered)
            out = merge_truncated(all_s, all_i, k, merge=merge)
        if trace is not None:
            trace.lap("merge", t0)
        return out

    kl = truncated_list_len(k, world)
    ms, mi, unproven = merged(query, kl)
    redo = torch.nonzero(unproven).flatten()
    if trace is not None:
        trace.second_round_queries += int(redo.numel())
    if redo.numel() > 0:                       # identical on every rank
        rs, ri, _ = merged(query[redo].contiguous(), k)
        ms[redo], mi[redo] = rs, ri
    return ms, mi


def is_trained_before_train(param):
    """What `faiss.index_factory(dim, param).is_trained` reports BEFORE `index.train` (the value the reference prints,
    MEVI/faiss_search.py:16): False for every component that learns from data -- IVF coarse quantisers, product /
    scalar / residual quantisers, OPQ / PCA / ITQ transforms --, True for Flat, HNSW over Flat storage, LSH, IDMap.  A refine
    suffix ('...,RFlat', '...,Refine(Flat)': mevi_amd/refine.py) learns nothing itself: the components before it decide."""
    learns = ("IVF", "IMI", "PQ", "OPQ", "PCA", "ITQ", "SQ", "RQ", "LSQ", "PRQ", "PLSQ")
    for comp in str(param).split(","):
        c = comp.strip()
        if c.startswith("HNSW") and "_" in c:                  # HNSW32_PQ8 ...: storage given after the underscore
            c = c.split("_", 1)[1]
        if c.startswith(learns):
            return False
    return True


def search(query, doc, dim, topk, param="Flat", device=None):
    """Drop-in for faiss_search.search (MEVI/faiss_search.py:13-21).

    `param` is the faiss factory string the reference forwards: "Flat" -> exact search (result parity defined);
    "IVF<n>,Flat" (the script's default) -> IVF-Flat with faiss's structure and defaults (mevi_amd/ivf.py: inner-
    product k-means, nprobe = MEVI_IVF_NPROBE or 1; recall vs the exact search is reported on stderr);
    "IVF<n>,PQ<m>[x<b>]" / "PQ<m>[x<b>]" (b <= 8) -> product-quantised lists searched by ADC on the device
    (mevi_amd/ivfpq.py; same nprobe and recall report; MEVI_IVFPQ=exact answers them with the exact search instead, as do
    shapes outside the index's envelope: dim % m != 0, m % 4 != 0, fewer rows than 2^b, nlist > rows, topk > 4096);
    "IVF<n>,PQ<m>x4fs" / "PQ<m>x4fs" -> the same index at 4 bits with two codes per byte and a scan whose table gathers cannot
    meet an LDS bank conflict (mevi_amd/pqfs.py; f32 tables, residual codes: the results of "PQ<m>x4", not faiss's u8 tables;
    same nprobe and recall report; MEVI_PQFS=exact answers them with the exact search instead, as do dim % m != 0, m % 8 != 0,
    m outside 8..96, fewer than 16 rows, nlist > rows and topk > 4096);
    "HNSW<M>" / "HNSW<M>,Flat" -> a neighbour graph of degree 2M walked on the device (mevi_amd/hnsw.py: exact kNN links plus
    reverse links, no pruning; seeds from strided entry rows or, with MEVI_HNSW_ENTRY=levels, from a descent through
    deterministic upper levels; efSearch = MEVI_HNSW_EFSEARCH or 16; recall and steps on stderr;
    MEVI_HNSW=exact answers it with the exact search instead, as do dim % 4 != 0, M outside 2..256, topk > 4096 and corpora
    of fewer than 64 * 2M rows, where a graph of that degree is close to complete);
    "SQ8" / "SQ4" / "IVF<n>,SQ8" / "IVF<n>,SQ4" -> one byte or one nibble per dimension with a per-dimension min / max range,
    decoded inside the list scan on the device (mevi_amd/sq.py; same nprobe and recall report; MEVI_SQ=exact answers them with
    the exact search instead, as do dim % 4 != 0 (8 bits) / dim % 8 != 0 (4 bits), dim > 4096, nlist > rows and topk > 4096);
    "OPQ<M>,[IVF<n>,]PQ<m>[x<b>]" / "OPQ<M>,[IVF<n>,]PQ<m>x4fs" -> the two PQ families behind a learned orthonormal rotation
    (mevi_amd/opq.py: faiss OPQMatrix's training loop with the SVD on the host, the coarse quantiser kept in the input space, the
    product quantiser on rotated residuals, one more GEMM on the queries per search; the report adds the trainer's iterations
    and errors; MEVI_OPQ=exact answers them with the exact search instead, as do "OPQ<M>_<dout>" with dout != dim, dim % M != 0,
    dim / M % 4 != 0, fewer than 256 rows, an inner index outside its own envelope and OPQ in front of anything else);
    "RQ<M>x<b>" / "IVF<n>,RQ<M>x<b>" (b <= 8) -> a residual quantiser: M code bytes a row as "PQ<M>", every code a full-width
    centroid of what the levels before it leave, searched by ADC with full-width lookup tables (mevi_amd/rqindex.py; greedy
    encoding and training where faiss keeps a beam of 5, unless MEVI_RQINDEX_BEAM / MEVI_RQINDEX_TRAIN_BEAM = 1..16 ask for one; same nprobe and recall report, plus the training error per level;
    MEVI_RQINDEX=exact answers them with the exact search instead, as do dim % 4 != 0, M % 4 != 0, M outside 4..96, M * 2^b * 4
    bytes above 96 KiB, fewer rows than 2^b, nlist > rows, topk > 4096, and the strings "RQ<M>" without a width, "RQ..._N<norm>",
    "RQ1x16-6x8", "LSQ...", "PRQ..." and "OPQ...,RQ...");
    "<index>,RFlat" / "<index>,Refine(Flat)" with <index> one of the PQ, x4fs, OPQ, SQ and RQ strings above -> that index asked for
    k_base = int(topk * MEVI_REFINE_K_FACTOR) candidates (default factor 1, as faiss) whose original rows are then scored with the
    exact search's chain and cut to topk in one device call (mevi_amd/refine.py: every returned score is a bit of the exact
    search; the report gives the recall of the refined list and of the inner index's own first topk; MEVI_REFINE=exact answers
    them with the exact search instead, as do k_base > 4096, an inner index outside its own envelope, "Refine(<not Flat>)" and a
    refine behind Flat, IVF<n>,Flat or HNSW<M>, whose scores are exact already);
    every other index type (HNSW<M>_PQ*, SQ6, SQfp16, PCA*, LSQ*, PRQ*, ...) is served by exact search (recall >= the approximate index it
    names).
    Returns numpy (dists f32[nq,topk], indices i64[nq,topk]).
    """
    hip.require_gpu()
    device = torch.device(device if device is not None else "cuda")
    print(f"Param {param} trained: {is_trained_before_train(param)}.")  # index.is_trained before index.train
    q = _as_device_f32(np.asarray(query).reshape(-1, dim) if isinstance(query, np.ndarray) else query, device)
    d = _as_device_f32(np.asarray(doc).reshape(-1, dim) if isinstance(doc, np.ndarray) else doc, device)
    from . import hnsw, ivf, ivfpq, opq, pqfs, refine, rqindex, sq

    nlist = ivf.parse_factory(param)
    ref = refine.wanted(param, d.shape[0], d.shape[1], topk) if nlist is None else None
    pq = ivfpq.wanted(param, d.shape[0], d.shape[1], topk) if nlist is None else None
    fs = pqfs.wanted(param, d.shape[0], d.shape[1], topk) if nlist is None else None
    sq_spec = sq.wanted(param, d.shape[0], d.shape[1], topk) if nlist is None else None
    links = hnsw.wanted(param, d.shape[0], d.shape[1], topk)
    rot = opq.wanted(param, d.shape[0], d.shape[1], topk) if nlist is None else None
    rqx = rqindex.wanted(param, d.shape[0], d.shape[1], topk) if nlist is None else None
    if nlist is not None and topk <= MAX_K and 0 < nlist <= d.shape[0]:
        s, i = ivf.search(q, d, topk, nlist)
    elif ref is not None:
        s, i = refine.search(q, d, topk, *ref)
    elif rot is not None:
        s, i = opq.search(q, d, topk, *rot)
    elif pq is not None:
        s, i = ivfpq.search(q, d, topk, *pq)
    elif fs is not None:
        s, i = pqfs.search(q, d, topk, *fs)
    elif sq_spec is not None:
        s, i = sq.search(q, d, topk, *sq_spec)
    elif rqx is not None:
        s, i = rqindex.search(q, d, topk, *rqx)
    elif links is not None:
        s, i = hnsw.search(q, d, topk, links)
    elif topk > MAX_K:
        s, i = _search_large_k(q, d, topk)
    else:
        s, i = DenseIndex(d).search(q, topk)  # index.add(doc); index.search(query, topk)
    return s.cpu().numpy(), i.cpu().numpy()


def profile(query, doc, dim, topk, param, bs=[1, 2, 4, 8], device=None):
    """Drop-in for faiss_search.profile (MEVI/faiss_search.py:32-68), the reference authors' timing hook of the dense arm:
    seconds of `train`, `add` (= upload + index build here) and the MEAN seconds of one `index.search` call at each batch size
    over the first ten batches of `query` (a ragged last batch is filled with random other queries, as the reference does).
    Every search takes the batch from host memory and returns numpy arrays, like faiss's API.  Returns the `all_time` dict."""
    import time

    from . import hnsw, ivf, ivfpq, opq, pqfs, refine, rqindex, sq

    hip.require_gpu()
    device = torch.device(device if device is not None else "cuda")
    all_time = {"train": 0, "add": 0}
    for b in bs:
        all_time[f"search_bs{b}"] = 0
    print(f"Param {param} trained: {is_trained_before_train(param)}.")
    query = np.asarray(query, dtype=np.float32).reshape(-1, dim)
    nlist = ivf.parse_factory(param)
    with hip.device_guard(device):
        t = time.time()
        d = _as_device_f32(np.asarray(doc).reshape(-1, dim) if isinstance(doc, np.ndarray) else doc, device)
        torch.cuda.synchronize()
        upload = time.time() - t
        use_ivf = nlist is not None and 0 < nlist <= d.shape[0] and topk <= MAX_K
        ref = refine.wanted(param, d.shape[0], d.shape[1], topk) if nlist is None else None
        pq = ivfpq.wanted(param, d.shape[0], d.shape[1], topk) if nlist is None else None
        sq_spec = sq.wanted(param, d.shape[0], d.shape[1], topk) if nlist is None else None
        fs = pqfs.wanted(param, d.shape[0], d.shape[1], topk) if nlist is None else None
        rot = opq.wanted(param, d.shape[0], d.shape[1], topk) if nlist is None else None
        rqx = rqindex.wanted(param, d.shape[0], d.shape[1], topk) if nlist is None else None
        if ref is not None:                                            # '<index>,RFlat': train and add are the inner index's
            pq, fs, rot, sq_spec, rqx = (ref[1] if ref[0] == name else None for name in ("ivfpq", "pqfs", "opq", "sq", "rqindex"))
        t = time.time()
        cent = ivf.train_centroids(d, nlist) if use_ivf else None      # index.train(doc)
        if pq is not None:                                             # ... of the coarse and the product quantiser
            cent = ivf.train_centroids(d, pq[0]) if pq[0] is not None else None
            book = ivfpq.train_codebook(d, ivf.assign(d, cent) if cent is not None else None, cent, pq[1], pq[2])
        if fs is not None:                                             # ... of the coarse and the 16-centroid product quantiser
            cent = ivf.train_centroids(d, fs[0]) if fs[0] is not None else None
            book = ivfpq.train_codebook(d, ivf.assign(d, cent) if cent is not None else None, cent, fs[1], pqfs.NBITS)
        if sq_spec is not None:                                        # ... of the coarse quantiser and the range
            cent = ivf.train_centroids(d, sq_spec[0]) if sq_spec[0] is not None else None
            sq_range = sq.train_range(d, ivf.assign(d, cent) if cent is not None else None, cent)
        if rot is not None:                                            # ... of the rotation, then both quantisers behind it
            R = opq.train_rotation(d, rot[0])[0]
            cent = ivf.train_centroids(d, rot[1]) if rot[1] is not None else None
            book = ivfpq.train_codebook(d, ivf.assign(d, cent) if cent is not None else None, cent, rot[2], rot[3],
                                        rotation=ivfpq.rotated_centroids(cent, R))
        if rqx is not None:                                            # ... of the coarse and the residual quantiser
            cent = ivf.train_centroids(d, rqx[0]) if rqx[0] is not None else None
            book = rqindex.train_codebook(d, ivf.assign(d, cent) if cent is not None else None, cent, rqx[1], rqx[2])
        torch.cuda.synchronize()
        all_time["train"] += time.time() - t
        t = time.time()
        links = hnsw.wanted(param, d.shape[0], d.shape[1], topk)
        if pq is not None:                                             # index.add(doc): lists and codes
            index = ivfpq.IVFPQIndex(d, pq[0], pq[1], pq[2], centroids=cent, codebook=book)
            use_ivf = True
        elif fs is not None:                                           # index.add(doc): lists and packed codes
            index = pqfs.PQFSIndex(d, fs[0], fs[1], centroids=cent, codebook=book)
            use_ivf = True
        elif rot is not None:                                          # index.add(doc): lists and codes of rotated residuals
            index = opq.OPQIndex(d, *rot, R=R, centroids=cent, codebook=book)
            use_ivf = True
        elif sq_spec is not None:                                      # index.add(doc): lists and codes
            index = sq.SQIndex(d, sq_spec[0], sq_spec[1], centroids=cent, vmin=sq_range[0], vdiff=sq_range[1])
            use_ivf = True
        elif rqx is not None:                                          # index.add(doc): lists and codes, level group by level group
            index = rqindex.RQIndex(d, *rqx, centroids=cent, codebook=book)
            use_ivf = True
        elif links is not None and not use_ivf:                        # index.add(doc): kNN lists, links, entry rows
            index = hnsw.HNSWIndex(d, links)
        else:
            index = ivf.IVFFlatIndex(d, nlist, centroids=cent) if use_ivf else (DenseIndex(d) if topk <= MAX_K else None)
        if ref is not None:                                            # ... the rows are resident already: nothing to add for the refine
            index = refine.RefineIndex(index, d)
        if isinstance(index, DenseIndex) and any(index.small_image_wanted(b, topk) for b in bs):
            index.prepare_small()                               # the 8-bit image of the small batches is part of index.add
        torch.cuda.synchronize()
        all_time["add"] += upload + time.time() - t

        def one(bq):
            q = torch.from_numpy(np.ascontiguousarray(bq)).to(device)
            if use_ivf:
                s, i = index.search(q, topk, int(os.environ.get("MEVI_IVF_NPROBE", "1")))
            elif links is not None:
                s, i = index.search(q, topk)
            elif index is None:
                s, i = _search_large_k(q, d, topk)
            else:
                s, i = index.search(q, topk)
            return s.cpu().numpy(), i.cpu().numpy()

        nquery = len(query)
        for b in bs:
            print(f"Profile batch size {b}...")
            batched = []
            for start in range(0, nquery, b):
                cur = query[start:start + b]
                if len(cur) < b:
                    rest = np.random.choice(np.arange(nquery), size=b - len(cur), replace=False)
                    cur = np.concatenate((cur, query[rest]), axis=0)
                batched.append(cur)
                if len(batched) >= 10:
                    break
            if not batched:
                continue
            one(batched[0])                                     # first-call set-up (module load, LDS opt-in) is not a search cost
            torch.cuda.synchronize()
            t = time.time()
            for bq in batched:
                one(bq)
            all_time[f"search_bs{b}"] += (time.time() - t) / len(batched)
    return all_time


MAX_K = 4096     # list length the threshold-filter kernels keep per query (include/mevi_hip.h)


def _search_large_k(q, d, k, rows_budget=1 << 28):
    """faiss accepts any k; the filter kernels keep at most MAX_K entries per query.  Beyond that (not a configuration of
    any reference script) the scores of a few queries at a time are materialised with the f32 GEMM -- the same
    sequential fmaf chains -- and ordered by (score desc, id asc) with two stable device sorts; -1 / -FLT_MAX padding
    when k exceeds the corpus, as faiss."""
    from . import ops

    nq, nd = q.shape[0], d.shape[0]
    out_s = torch.full((nq, k), torch.finfo(torch.float32).min, dtype=torch.float32, device=q.device)
    out_i = torch.full((nq, k), -1, dtype=torch.int64, device=q.device)
    kk = min(k, nd)
    step = max(1, rows_budget // max(nd, 1))
    for a in range(0, nq, step):
        sc = ops.linear(q[a:a + step].contiguous(), d)                        # [b, nd], exact chains
        order = torch.argsort(sc, dim=1, descending=True, stable=True)         # ties keep ascending id
        out_i[a:a + step, :kk] = order[:, :kk]
        out_s[a:a + step, :kk] = torch.gather(sc, 1, order[:, :kk])
    return out_s, out_i
