"""Residual and product quantisation on MI355X: the 'rq' / 'l2' slice of the reference's
`ProductQuantization` (MEVI/pq.py:15) that the eval scripts use, its 'pq' / 'l2' slice (the reference's default
pq_type), plus the cluster index the fine stage consumes.

Reference surface mirrored (same names and argument meaning):
  ProductQuantization(pq_type, subvector_num, subvector_bits, dist_mode, emb_size, ...)
    .get_codebook()                                           pq.py:133-141
    .initialize(index_file, doc_emb, rank, seed, pq_cluster_path, encode_batch_size)
         -- only the "load rqcodebook*.pt" branch (pq.py:459-463) + broadcast (:484)
    .get_document_cluster(doc_embeddings, rank, nrank, batch_size, return_mapping)  pq.py:217-247
    .forward(vecs) -> index   (forward_rq, pq.py:337-369; proba/loss are training outputs)
    .get_reconstruct_vector(index)                            pq.py:768-784
'pq' differs from 'rq' only in the coding: subspace j of a row (columns j*dsub .. (j+1)*dsub - 1, dsub = dim // M) is
coded against C[j] alone, reconstruct = concatenation.  'opq' is 'pq' behind a rotation (pq.py:67-71, 259-279, 629-630, 775-783):
`rotate` f32[dim, dim] beside the codebook, y = x @ rotate.T is what gets coded (mevi_opq_encode_f32: rotate + encode in one launch),
reconstruct = concatenation @ rotate; its training stands in for the reference's faiss branch (`train_opq`).  EMA / gumbel training
and 'ip' / 'iptol2' are out of scope.
"""
from collections import defaultdict

import numpy as np
import torch

from . import hip


_LAST_ENCODE = {}
_BEAM_WORKSPACES = {}             # (device, stream, emb_size, M, K, R, pq) -> the fused beam encode's workspace


def last_encode_stats():
    """What the last rq_encode call did: path taken and, for the matrix-core path, {ambiguity records, rows re-encoded by
    the exact kernel, ambiguous row-levels} (read back with a stream synchronisation: bench / tests only)."""
    st = dict(_LAST_ENCODE)
    ws = st.pop("_ws", None)
    if ws is not None:
        import ctypes

        out = (ctypes.c_int64 * 3)()
        with hip.device_guard(ws.device):
            hip.check(hip.lib().mevi_rq_encode_fast_stats(hip.ptr(ws), st["n"], st["dim"], st["M"], st["K"], out, hip.stream_ptr()),
                      "mevi_rq_encode_fast_stats")
        st.update(records=int(out[0]), rows_reencoded_exactly=int(out[1]), ambiguous_row_levels=int(out[2]))
    return st


KEEP_ENCODE_WORKSPACE = False     # bench / tests set this: last_encode_stats() then reads the fast path's record counters


def rq_encode(x, codebook, mode=None):
    """codes i32[n, M] of x f32[n, dim] against codebook f32[M, K, dim] (CUDA tensors).

    mode (default MEVI_RQ or 'fast'): 'fast' = the matrix-core encoder with exact re-check (csrc/rq_fast.hip) wherever its
    shape constraints hold, 'exact' = the f32 VALU kernel (csrc/rq_encode.hip).  Both return the oracle's codes bit for bit."""
    import os

    hip.require_gpu()
    assert x.is_cuda and codebook.is_cuda and x.dtype == torch.float32 and codebook.dtype == torch.float32
    x = x.contiguous()
    codebook = codebook.contiguous()
    M, K, dim = codebook.shape
    assert x.dim() == 2 and x.shape[1] == dim
    n = x.shape[0]
    mode = mode or os.environ.get("MEVI_RQ", "fast")
    assert mode in ("fast", "exact"), mode
    codes = torch.empty((n, M), dtype=torch.int32, device=x.device)
    L = hip.lib()
    _LAST_ENCODE.clear()
    with hip.device_guard(x.device):
        nbytes = L.mevi_rq_encode_fast_workspace_bytes(n, dim, M, K) if mode == "fast" and n > 0 else 0
        if nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            st = L.mevi_rq_encode_fast_f32(hip.ptr(x), n, dim, hip.ptr(codebook), M, K, hip.ptr(codes), hip.ptr(ws), nbytes,
                                           hip.stream_ptr())
            hip.check(st, "mevi_rq_encode_fast_f32")
            _LAST_ENCODE.update(path="fast", n=n, dim=dim, M=M, K=K)
            if KEEP_ENCODE_WORKSPACE:       # ~n*M*32 bytes (1.2 GB at MS MARCO size): never pinned in the product path
                _LAST_ENCODE["_ws"] = ws
        else:
            st = L.mevi_rq_encode_f32(hip.ptr(x), n, dim, hip.ptr(codebook), M, K, hip.ptr(codes), hip.stream_ptr())
            hip.check(st, "mevi_rq_encode_f32")
            _LAST_ENCODE.update(path="exact", n=n, dim=dim, M=M, K=K)
    return codes


def pq_encode(x, codebook):
    """codes i32[n, M] of x f32[n, dim] against a product codebook f32[M, K, dsub] (CUDA tensors): code j = the nearest
    centroid of C[j] to x[:, j*dsub:(j+1)*dsub] (csrc/pq_encode.hip; the oracle's arithmetic bit for bit)."""
    hip.require_gpu()
    assert x.is_cuda and codebook.is_cuda and x.dtype == torch.float32 and codebook.dtype == torch.float32
    x = x.contiguous()
    codebook = codebook.contiguous()
    M, K, dsub = codebook.shape
    assert x.dim() == 2 and M * dsub <= x.shape[1], (x.shape, codebook.shape)
    n, dim = x.shape
    codes = torch.empty((n, M), dtype=torch.int32, device=x.device)
    with hip.device_guard(x.device):
        st = hip.lib().mevi_pq_encode_f32(hip.ptr(x), n, dim, hip.ptr(codebook), M, K, dsub, hip.ptr(codes),
                                          hip.stream_ptr())
    hip.check(st, "mevi_pq_encode_f32")
    return codes


OPQ_ENCODE_DEFAULT = "fused"      # MEVI_OPQ_ENCODE: 'fused' = mevi_opq_encode_f32, 'steps' = rotate a chunk, then mevi_pq_encode_f32


def opq_encode(x, R, codebook, mode=None):
    """codes i32[n, M] of chain(x, R) f32[n, dim] against a product codebook f32[M, K, dsub], M * dsub == dim (CUDA tensors): the
    codes `pq_encode` gives for the rows rotated by mevi_opq_rotate_rows_f32, bit for bit.
    mode (default MEVI_OPQ_ENCODE or OPQ_ENCODE_DEFAULT): 'fused' = mevi_opq_encode_f32 (csrc/opq_encode.hip), one launch, no rotated
    value reaches memory; 'steps' = that composition, `ivfpq.ENCODE_CHUNK` rows rotated at a time.  A shape outside the fused
    kernel's envelope (mevi_opq_encode_fused) takes 'steps' whatever the mode."""
    import os

    hip.require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
    assert R.is_cuda and R.dtype == torch.float32 and codebook.is_cuda and codebook.dtype == torch.float32
    x, R, codebook = x.contiguous(), R.contiguous(), codebook.contiguous()
    M, K, dsub = codebook.shape
    n, dim = x.shape
    assert M * dsub == dim and tuple(R.shape) == (dim, dim), (x.shape, R.shape, codebook.shape)
    mode = mode or os.environ.get("MEVI_OPQ_ENCODE", OPQ_ENCODE_DEFAULT)
    if mode not in ("fused", "steps"):
        raise ValueError(f"MEVI_OPQ_ENCODE={mode!r} is neither 'fused' nor 'steps'")
    L = hip.lib()
    if mode == "fused" and L.mevi_opq_encode_fused(dim, M, K, dsub):
        codes = torch.empty((n, M), dtype=torch.int32, device=x.device)
        with hip.device_guard(x.device):
            st = L.mevi_opq_encode_f32(hip.ptr(x) if n else None, n, dim, hip.ptr(R), hip.ptr(codebook), M, K, dsub,
                                       hip.ptr(codes) if n else None, hip.stream_ptr())
        hip.check(st, "mevi_opq_encode_f32")
        return codes
    from . import dense
    from .ivfpq import ENCODE_CHUNK

    codes = torch.empty((n, M), dtype=torch.int32, device=x.device)
    for a in range(0, n, ENCODE_CHUNK):       # the rotated chunk is the only rotated rows that exist
        y = dense.opq_rotate_rows(x[a:a + ENCODE_CHUNK], None, None, None, R, mode="fused")
        codes[a:a + ENCODE_CHUNK] = pq_encode(y, codebook)
    return codes


def cluster_means(x, labels, K, old=None):
    """Per-cluster means of x f32[n, dim] under labels i32[n] (or [n, 1]): (centroids f32[K, dim], counts i32[K],
    sum of squared row norms as a float).  Deterministic; an empty cluster keeps `old[k]` (0 without `old`)."""
    hip.require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and labels.dtype == torch.int32 and x.is_contiguous()
    n, dim = x.shape
    labels = labels.contiguous().view(-1)
    cent = torch.empty((K, dim), dtype=torch.float32, device=x.device)
    counts = torch.empty(K, dtype=torch.int32, device=x.device)
    sumsq = torch.zeros(1, dtype=torch.float64, device=x.device)
    L = hip.lib()
    nbytes = L.mevi_cluster_means_workspace_bytes(n, dim, K)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=x.device)
    with hip.device_guard(x.device):
        st = L.mevi_cluster_means_f32(hip.ptr(x), n, dim, hip.ptr(labels), 1, K,
                                      hip.ptr(old.contiguous()) if old is not None else None, hip.ptr(cent),
                                      hip.ptr(counts), hip.ptr(sumsq), hip.ptr(ws), nbytes, hip.stream_ptr())
    hip.check(st, "mevi_cluster_means_f32")
    return cent, counts, float(sumsq.item())


def _kmeans_pp(xs, K, gen):
    """k-means++ seeding with 2 + log(K) greedy trials per centre (the scheme scikit-learn's `init='k-means++'` uses),
    on a sample that fits a [trials, m] distance matrix; torch ops on the device (seeding is a few thousand rows)."""
    m = xs.shape[0]
    trials = 2 + int(np.log(K))
    centers = torch.empty((K, xs.shape[1]), dtype=torch.float32, device=xs.device)
    first = int(torch.randint(m, (1,), generator=gen, device=xs.device).item())
    centers[0] = xs[first]
    d2 = ((xs - centers[0]) ** 2).sum(1)
    for c in range(1, K):
        # (every remaining point ON a chosen centre -- fewer distinct points than K, or a residual level that is already zero:
        # d2 sums to 0 and torch.multinomial aborts the device on an all-zero distribution -- then any point will do: uniform)
        tot = d2.sum()
        probs = torch.where(tot > 0, (d2 / tot.clamp_min(1e-30)).clamp_min(0), torch.full_like(d2, 1.0 / m))
        probs = torch.nan_to_num(probs, nan=1.0 / m, posinf=1.0 / m)
        cand = torch.multinomial(probs, trials, replacement=True, generator=gen)
        dc = torch.cdist(xs[cand], xs) ** 2                    # [trials, m]
        pot = torch.minimum(dc, d2[None]).sum(1)
        best = int(torch.argmin(pot).item())
        centers[c] = xs[cand[best]]
        d2 = torch.minimum(d2, dc[best])
    return centers


def kmeans(x, K, seed=0, max_iter=100, n_init=10, sample=32768, tol=1e-7):
    """Lloyd's k-means on the GPU: assignment = mevi_rq_encode_f32 against a one-level codebook (lowest index on ties,
    as everywhere), update = mevi_cluster_means_f32.  `n_init` k-means++ seedings are tried on a sample, the one with
    the lowest sample inertia after a few iterations starts the full run.  Returns (centres f32[K, dim],
    labels i32[n], inertia).  Deterministic for a given seed.

    Stands in for the scikit-learn (Mini-batch) KMeans the reference trains its codebooks with (MEVI/pq.py:550-567):
    a randomised algorithm, so parity is statistical -- tests hold the final quantisation error against
    scikit-learn's on the same data."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
    x = x.contiguous()
    n = x.shape[0]
    gen = torch.Generator(device=x.device).manual_seed(int(seed))
    xs = x[torch.randperm(n, generator=gen, device=x.device)[:min(n, sample)]].contiguous()

    def lloyd(data, centers, iters):
        inertia = float("inf")
        labels = None
        for _ in range(iters):
            labels = rq_encode(data, centers[None].contiguous()).view(-1)
            new, counts, sumsq = cluster_means(data, labels, K, old=centers)
            # inertia of the NEW centres w.r.t. this assignment: sum ||x||^2 - sum_k n_k ||m_k||^2
            new_inertia = sumsq - float((counts.double() * (new.double() ** 2).sum(1)).sum().item())
            shift = float(((new - centers) ** 2).sum().item())
            centers = new
            if shift <= tol * max(float((centers ** 2).sum().item()), 1e-30) or abs(inertia - new_inertia) <= tol * abs(new_inertia):
                inertia = new_inertia
                break
            inertia = new_inertia
        return centers, labels, inertia

    best = None
    for _ in range(max(1, n_init)):
        c0 = _kmeans_pp(xs, K, gen)
        c1, _, inert = lloyd(xs, c0, 10)
        if best is None or inert < best[1]:
            best = (c1, inert)
    centers, labels, inertia = lloyd(x, best[0], max_iter)
    labels = rq_encode(x, centers[None].contiguous()).view(-1)   # labels of the returned centres
    return centers, labels, inertia


def train_rq_codebook(x, M, K, seed=0, **kw):
    """Residual quantisation codebook as the reference trains it (MEVI/pq.py:577-592): level i is k-means on the
    residual left by levels < i.  Returns (codebook f32[M, K, dim], codes i32[n, M]); `x` is not modified."""
    res = x.contiguous().clone()
    n, dim = res.shape
    src = torch.arange(n, dtype=torch.int64, device=x.device)
    book, codes = [], []
    L = hip.lib()
    for level in range(M):
        centers, labels, _ = kmeans(res, K, seed=seed + level, **kw)
        book.append(centers)
        codes.append(labels)
        if level != M - 1:
            with hip.device_guard(x.device):   # res -= centers[labels], row by row in place
                st = L.mevi_gather_sub_f32(hip.ptr(res), hip.ptr(src), hip.ptr(centers), hip.ptr(labels), n, dim,
                                           hip.ptr(res), hip.stream_ptr())
            hip.check(st, "mevi_gather_sub_f32")
    return torch.stack(book), torch.stack(codes, 1).contiguous()


def train_pq_codebook(x, M, K, seed=0, **kw):
    """Product quantisation codebook as the reference trains it (MEVI/pq.py:577-587): subspace j is k-means on the column
    slice j*dsub .. (j+1)*dsub - 1 (dsub = dim // M), seeded seed + j.  Returns (codebook f32[M, K, dsub], codes i32[n, M])."""
    x = x.contiguous()
    dsub = x.shape[1] // M
    book, codes = [], []
    for j in range(M):
        centers, labels, _ = kmeans(x[:, j * dsub:(j + 1) * dsub].contiguous(), K, seed=seed + j, **kw)
        book.append(centers)
        codes.append(labels)
    return torch.stack(book), torch.stack(codes, 1).contiguous()


PQ_ENCODE_MAX_M = 32              # subspaces of one mevi_pq_encode_f32 call


def pq_encode_groups(x, codebook):
    """`pq_encode` for any number of subspaces: more than PQ_ENCODE_MAX_M are encoded in groups on contiguous column slices."""
    M, _, dsub = codebook.shape
    if M <= PQ_ENCODE_MAX_M:
        return pq_encode(x, codebook)
    codes = torch.empty((x.shape[0], M), dtype=torch.int32, device=x.device)
    for g in range(0, M, PQ_ENCODE_MAX_M):
        h = min(M, g + PQ_ENCODE_MAX_M)
        codes[:, g:h] = pq_encode(x[:, g * dsub:h * dsub].contiguous(), codebook[g:h].contiguous())
    return codes


def pq_lloyd(x, codebook, iters):
    """`iters` Lloyd iterations of every subspace's k-means on x f32[n, M * dsub], started from `codebook` f32[M, K, dsub]: assign
    (mevi_pq_encode_f32, lowest index on ties), then the means of every subspace's clusters (mevi_cluster_means_f32; an empty
    cluster keeps its old centre).  The count is fixed and nothing is read back to the host: the inner loop of the OPQ rotation
    trainer (mevi_amd/opq.py), which hot-starts it from the codebook of the previous rotation.  Returns the new codebook."""
    hip.require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and codebook.dtype == torch.float32
    M, K, dsub = codebook.shape
    n = x.shape[0]
    assert x.shape[1] == M * dsub, (x.shape, codebook.shape)
    x = x.contiguous()
    parts = x.view(n, M, dsub).permute(1, 0, 2).contiguous()       # [M, n, dsub]: cluster_means reads contiguous rows
    L = hip.lib()
    nbytes = L.mevi_cluster_means_workspace_bytes(n, dsub, K)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=x.device)
    counts = torch.empty(K, dtype=torch.int32, device=x.device)
    book = codebook.contiguous()
    for _ in range(int(iters)):
        codes = pq_encode_groups(x, book)
        new = torch.empty_like(book)
        with hip.device_guard(x.device):
            for j in range(M):
                st = L.mevi_cluster_means_f32(hip.ptr(parts[j]), n, dsub, hip.ptr(codes[:, j]), M, K, hip.ptr(book[j]), hip.ptr(new[j]),
                                              hip.ptr(counts), None, hip.ptr(ws), nbytes, hip.stream_ptr())
                hip.check(st, "mevi_cluster_means_f32")
        book = new
    return book


class ClusterIndex:
    """CSR form of the reference's `pq_doc_cluster: dict[tuple -> list[int]]` and
    `pq_mapping: dict[int -> tuple]` (MEVI/main_models.py:3200-3220).

    key(code) = sum_j code[j] * K**(M-1-j);  doc ids of a cluster are ascending, exactly the
    order in which get_document_cluster appends them (pq.py:236-241)."""

    def __init__(self, M, K, keys, offsets, doc_ids, codes=None):
        self.M, self.K = M, K
        self.keys = keys          # i64[n_clusters] sorted distinct keys
        self.offsets = offsets    # i64[n_clusters + 1]
        self.doc_ids = doc_ids    # i64[N]
        self.codes = codes        # optional i32[N, M] (the mapping)

    @staticmethod
    def code_keys(codes, K):
        codes = np.asarray(codes, dtype=np.int64)
        M = codes.shape[-1]
        w = K ** np.arange(M - 1, -1, -1, dtype=np.int64)
        return (codes * w).sum(-1)

    @classmethod
    def from_codes(cls, codes, K, start=0):
        codes = np.asarray(codes)
        keys_all = cls.code_keys(codes, K)
        order = np.argsort(keys_all, kind="stable")
        sk = keys_all[order]
        keys, first = np.unique(sk, return_index=True)
        offsets = np.append(first, len(sk)).astype(np.int64)
        return cls(codes.shape[1], K, keys, offsets, (order + start).astype(np.int64), codes.astype(np.int32))

    @classmethod
    def from_topk_labels(cls, labels, K):
        """labels i32[N, C, M] (every document's top-C code paths, pq.get_topk_document_mapping): the multi-cluster
        index of gen_pq_doc_topk(return_cluster=True) (MEVI/main_models.py:3246-3256) -- a document is listed in each of
        its C clusters, lists in (document, path rank) order."""
        labels = np.asarray(labels)
        N, C, M = labels.shape
        idx = cls.from_codes(labels.reshape(N * C, M), K)
        return cls(M, K, idx.keys, idx.offsets, idx.doc_ids // C, None)

    @classmethod
    def from_dict(cls, cluster, M, K):
        """From the reference's pickled dict (rqclus*.pkl): vectorised, the dict has ~1 M keys / 8.8 M ids on MS MARCO."""
        from itertools import chain

        n = len(cluster)
        if n == 0:
            return cls(M, K, np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int64))
        keys = cls.code_keys(np.array(list(cluster.keys()), dtype=np.int64).reshape(n, M), K)
        sizes = np.fromiter(map(len, cluster.values()), dtype=np.int64, count=n)
        docs = np.fromiter(chain.from_iterable(cluster.values()), dtype=np.int64, count=int(sizes.sum()))
        order = np.argsort(keys, kind="stable")
        start = np.cumsum(sizes) - sizes                   # segment starts in dict order
        ssz = sizes[order]
        offsets = np.concatenate([[0], np.cumsum(ssz)]).astype(np.int64)
        # gather the segments in key order: element j of sorted segment i comes from start[order[i]] + j
        src = np.repeat(start[order] - offsets[:-1], ssz) + np.arange(len(docs), dtype=np.int64)
        return cls(M, K, keys[order], offsets, docs[src])

    def doc_codes(self, n_docs):
        """i32 [n_docs, M]: the code of every document (the inverse map `rqmapping*.pkl` stores as a dict of tuples);
        rows of documents that appear in no cluster are -1."""
        w = self.K ** np.arange(self.M - 1, -1, -1, dtype=np.int64)
        per_cluster = ((self.keys[:, None] // w[None, :]) % self.K).astype(np.int32)
        out = np.full((n_docs, self.M), -1, dtype=np.int32)
        out[self.doc_ids] = np.repeat(per_cluster, np.diff(self.offsets), axis=0)
        return out

    def lookup(self, code):
        """doc ids (ascending) of one cluster, empty array when the cluster owns no document."""
        key = int(self.code_keys(np.asarray(code), self.K))
        i = int(np.searchsorted(self.keys, key))
        if i >= len(self.keys) or self.keys[i] != key:
            return self.doc_ids[:0]
        return self.doc_ids[self.offsets[i]:self.offsets[i + 1]]

    def to_dicts(self):
        """(cluster dict, mapping dict) in the reference's pickle layout."""
        w = self.K ** np.arange(self.M - 1, -1, -1, dtype=np.int64)
        cluster = {}
        for i, key in enumerate(self.keys.tolist()):
            code = tuple(int((key // int(wj)) % self.K) for wj in w)
            cluster[code] = self.doc_ids[self.offsets[i]:self.offsets[i + 1]].tolist()
        mapping = {d: c for c, ds in cluster.items() for d in ds}
        return cluster, mapping


class ProductQuantization:
    def __init__(self, pq_type="rq", subvector_num=4, subvector_bits=5, dist_mode="l2", emb_size=768,
                 pq_init_method="kmeans", pq_update_method="none", device=None, **unused):
        if pq_type not in ("rq", "pq", "opq") or dist_mode != "l2":
            raise NotImplementedError("only pq_type 'rq', 'pq' or 'opq' with dist_mode='l2' is on the MEVI eval path")
        if pq_type == "opq" and (subvector_num < 1 or emb_size % subvector_num != 0 or (emb_size // subvector_num) % 4 != 0):
            raise NotImplementedError(f"pq_type 'opq': emb_size={emb_size} does not split into subvector_num={subvector_num} "
                                      "slices of a multiple of 4 columns")
        self.pq_type, self.dist_mode = pq_type, dist_mode
        self.subvector_num, self.subvector_bits = subvector_num, subvector_bits
        self.subvector_cents = 2 ** subvector_bits
        self.emb_size = emb_size
        self.last_dim = emb_size if pq_type == "rq" else emb_size // subvector_num     # pq.py:49-53
        self.pq_init_method = pq_init_method
        self.device = torch.device(device if device is not None else "cuda")
        self.codebook = torch.empty((subvector_num, self.subvector_cents, self.last_dim), dtype=torch.float32,
                                    device=self.device)
        # 'opq' (pq.py:67-71): y = x @ rotate.T is what the product quantiser codes; reconstruct rotates back
        self.rotate = torch.eye(emb_size, dtype=torch.float32, device=self.device) if pq_type == "opq" else None

    def get_codebook(self):
        return self.codebook

    def fix(self):
        pass  # nothing trains here

    def load_codebook(self, tensor):
        t = torch.as_tensor(np.asarray(tensor) if not torch.is_tensor(tensor) else tensor.detach(), dtype=torch.float32)
        assert tuple(t.shape) == tuple(self.codebook.shape), (t.shape, self.codebook.shape)
        self.codebook.copy_(t.to(self.device))

    def load_rotation(self, tensor):
        assert self.pq_type == "opq", self.pq_type
        t = torch.as_tensor(np.asarray(tensor) if not torch.is_tensor(tensor) else tensor.detach(), dtype=torch.float32)
        assert tuple(t.shape) == tuple(self.rotate.shape), (t.shape, self.rotate.shape)
        self.rotate.copy_(t.to(self.device))

    def load_opq_file(self, obj, where="the opq file"):
        """The 'opq' form of `pq_path`: torch.save({"codebook": f32[M, K, dsub], "rotate": f32[dim, dim]}) -- this build's own
        format (the reference reads the pair out of a faiss index file, pq.py:143-173, which cannot be read here)."""
        if not isinstance(obj, dict) or "codebook" not in obj or "rotate" not in obj:
            raise ValueError(f"pq_type 'opq': {where} must be a torch.save of {{'codebook': f32[M, K, dim // M], 'rotate': "
                             f"f32[dim, dim]}}; a bare {type(obj).__name__} has no rotation (a 'pq' / 'rq' codebook file, or a "
                             "faiss index, is not an opq file)")
        self.load_codebook(obj["codebook"])
        self.load_rotation(obj["rotate"])

    def initialize(self, index_file, doc_emb=None, rank=0, seed=0, pq_cluster_path=None, encode_batch_size=None):
        """Rank 0 loads `rqcodebook{M}_{bits}.pt` (torch.save of the f32[M,K,dim] parameter; f32[M,K,dim//M] for 'pq'; the
        {"codebook", "rotate"} dict of `load_opq_file` for 'opq'), then the state is broadcast (RCCL) when a process group exists."""
        import os

        import torch.distributed as dist

        if rank == 0:
            if index_file is not None and os.path.isfile(index_file):
                print("Intializing codebook with torch file...")
                obj = torch.load(index_file, map_location="cpu")
                if self.pq_type == "opq":
                    self.load_opq_file(obj, index_file)
                else:
                    self.load_codebook(obj)
            elif doc_emb is not None:  # pq.py:402-419: no file -> train on the embeddings, then save next to it
                if self.pq_type == "opq":
                    self.train_opq(doc_emb, seed)
                else:
                    self.unsupervised_update_codebook_manually(doc_emb, seed, self.pq_init_method)
                if index_file is not None:
                    torch.save({"codebook": self.codebook.detach().cpu(), "rotate": self.rotate.detach().cpu()}
                               if self.pq_type == "opq" else self.codebook.detach().cpu(), index_file)
            else:
                raise FileNotFoundError(f"{self.pq_type.upper()} codebook {index_file} not found and no embeddings to train one on")
        if dist.is_available() and dist.is_initialized():
            dist.broadcast(self.codebook, 0)
            if self.rotate is not None:
                dist.broadcast(self.rotate, 0)

    def train_opq(self, doc_emb, seed):
        """What faiss trains for 'OPQ{M},PQ{M}x{bits}' (the reference's pq_init_method 'faiss', pq.py:455-458, :182): the
        OPQMatrix rotation (`opq.train_rotation`, on the device), then the product quantiser on the rotated training sample of at
        most 256 * K rows (`ivfpq.train_codebook`'s sample and k-means settings).  That sample is the only rotated rows that exist."""
        from . import dense, ivfpq, opq

        x = doc_emb if torch.is_tensor(doc_emb) else torch.from_numpy(np.ascontiguousarray(doc_emb, dtype=np.float32))
        x = x.to(self.device, torch.float32).contiguous()
        M, K = self.subvector_num, self.subvector_cents
        if x.shape[0] < opq.TRAIN_K:
            raise ValueError(f"pq_type 'opq': the rotation trainer needs at least {opq.TRAIN_K} rows, got {x.shape[0]}")
        print("Training the OPQ rotation and its product codebook...")
        with hip.device_guard(self.device):
            R, errors = opq.train_rotation(x, M, seed=int(seed))
            gen = torch.Generator(device=x.device).manual_seed(int(seed))
            n = x.shape[0]
            rows = torch.randperm(n, generator=gen, device=x.device)[:min(n, ivfpq.MAX_POINTS_PER_CENTROID * K)]
            ys = dense.opq_rotate_rows(x, rows, None, None, R.contiguous(), mode="fused")
            book = train_pq_codebook(ys, M, K, seed=int(seed), n_init=1, max_iter=ivfpq.PQ_NITER)[0]
        self.rotate.copy_(R)
        self.codebook.copy_(book)
        print(f"OPQ rotation: niter {len(errors)}, training error {errors[0]:.6g} -> {errors[-1]:.6g}; {dict(opq.LAST_TRAIN)}")

    def unsupervised_update_codebook_manually(self, doc_emb, seed, kmeans_method="kmeans"):
        """Train the codebook on `doc_emb` (MEVI/pq.py:550-598, the scikit-learn path): 'rq' level i = k-means
        (k = 2**bits) on the residual of levels < i, 'pq' subspace j = k-means on column slice j.  Runs on the GPU
        (`train_rq_codebook` / `train_pq_codebook`); sets `last_preds` (i64 ndarray [n, M]) like the reference."""
        assert kmeans_method == "kmeans" and self.pq_type != "opq", (kmeans_method, self.pq_type)      # pq.py:553
        print("Updating codebook using KMeans...")
        x = doc_emb if torch.is_tensor(doc_emb) else torch.from_numpy(np.ascontiguousarray(doc_emb, dtype=np.float32))
        x = x.to(self.device, torch.float32)
        train = train_rq_codebook if self.pq_type == "rq" else train_pq_codebook
        book, codes = train(x, self.subvector_num, self.subvector_cents, seed=int(seed))
        self.codebook.copy_(book)
        self.last_preds = codes.cpu().numpy().astype(np.int64)

    def _encode(self, x):
        if self.pq_type == "opq":
            return opq_encode(x, self.rotate, self.codebook)
        return rq_encode(x, self.codebook) if self.pq_type == "rq" else pq_encode(x, self.codebook)

    def _rotated(self, doc_emb):
        """f32 [bs, dim] on the device: the rows the 'pq' beam encode scores -- chain(x, rotate) under 'opq' (pq.py:629-630)."""
        x = doc_emb.to(self.device, torch.float32).contiguous()
        if self.pq_type != "opq" or x.shape[0] == 0:
            return x
        from . import dense

        return dense.opq_rotate_rows(x, None, None, None, self.rotate, mode="fused")

    def forward(self, vecs, return_loss=False):
        """index i32[n, M]; the reference's (proba, index, loss) triple minus the training outputs."""
        return None, self._encode(vecs.to(self.device, torch.float32)), None

    def get_document_cluster(self, doc_embeddings, rank, nrank, batch_size=1 << 20, return_mapping=False,
                             as_index=False):
        """Encode this rank's contiguous slice (rows // nrank each, last rank takes the rest:
        pq.py:218-224) and group row ids by code tuple.  `batch_size` rows are resident on the
        GPU at a time (the reference's 128-row CPU batches compute the same thing)."""
        num_docs = doc_embeddings.shape[0]
        per = num_docs // nrank
        start = per * rank
        ending = num_docs if rank + 1 == nrank else start + per
        parts = []
        for b0 in range(start, ending, batch_size):
            b1 = min(b0 + batch_size, ending)
            chunk = doc_embeddings[b0:b1]
            chunk = chunk if torch.is_tensor(chunk) else torch.from_numpy(np.ascontiguousarray(chunk, dtype=np.float32))
            parts.append(self._encode(chunk.to(self.device, torch.float32)).cpu())
        codes = torch.cat(parts).numpy() if parts else np.zeros((0, self.subvector_num), np.int32)
        index = ClusterIndex.from_codes(codes, self.subvector_cents, start=start)
        print("Number of document clusters:", len(index.keys))
        if as_index:
            return index
        cluster = defaultdict(list)
        mapping = {}
        for i, c in enumerate(codes.tolist()):
            key = tuple(c)
            cluster[key].append(i + start)
            if return_mapping:
                mapping[i + start] = key
        return (dict(cluster), mapping) if return_mapping else dict(cluster)

    @torch.no_grad()
    def beam_search(self, doc_emb, num_return_sequences, num_beams=None, do_sample=False, return_proba=False):
        """Top-R code paths per row (pq.beam_search, MEVI/pq.py:613-713, rq_topk_score='prod'): per level
        softmax(-distance) times the running beam probability, top-R over beams x K.  'rq' scores the residual each
        beam hands down, 'pq' scores column slice j against C[j] (the same row for every beam).  Returns labels
        i32[bs, R, M] (and probabilities f32[bs, R])."""
        assert not do_sample and num_beams in (None, num_return_sequences)
        with hip.device_guard(self.device):          # stream_ptr() and the launches below refer to the codebook's GPU
            if self.beam_search_is_fused(num_return_sequences):
                return self._beam_search_fused(doc_emb, num_return_sequences, return_proba)
            return self._beam_search_steps(doc_emb, num_return_sequences, return_proba)

    def beam_search_is_fused(self, num_return_sequences):
        """True when `beam_search` takes mevi_rq_beam_encode_f32 (csrc/rq_beam.hip): not MEVI_RQ_BEAM=steps and the shape is
        inside the kernel's envelope (R <= 16, ...); otherwise the per-level composition `_beam_search_steps` runs."""
        import os

        mode = os.environ.get("MEVI_RQ_BEAM", "fused")
        assert mode in ("fused", "steps"), mode
        return mode == "fused" and hip.lib().mevi_rq_beam_encode_tile_docs(
            self.emb_size, self.subvector_num, self.subvector_cents, num_return_sequences, int(self.pq_type != "rq")) > 0

    def _beam_workspace(self, n, R):
        """The fused call's workspace, cached per (device, stream, shape): its size does not depend on n, and calls on one
        stream run one after the other, so they can share the tile ticket it holds."""
        pq = int(self.pq_type != "rq")
        key = (self.device, hip.stream_ptr(), self.emb_size, self.subvector_num, self.subvector_cents, R, pq)
        ws = _BEAM_WORKSPACES.get(key)
        if ws is None:
            nbytes = hip.lib().mevi_rq_beam_encode_workspace_bytes(n, self.emb_size, self.subvector_num, self.subvector_cents, R, pq)
            ws = _BEAM_WORKSPACES[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return ws

    def _beam_search_fused(self, doc_emb, num_return_sequences, return_proba):
        """All levels in one launch: reads x once, writes labels and probabilities only."""
        R, M, K = num_return_sequences, self.subvector_num, self.subvector_cents
        x = self._rotated(doc_emb)
        assert x.dim() == 2 and x.shape[1] == self.emb_size, (x.shape, self.emb_size)
        bs = x.shape[0]
        labels = torch.empty((bs, R, M), dtype=torch.int32, device=self.device)
        proba = torch.empty((bs, R), dtype=torch.float32, device=self.device) if return_proba else None
        if bs == 0:                                 # (an empty tensor has no address to hand over)
            return (labels, proba) if return_proba else labels
        ws = self._beam_workspace(bs, R)
        st = hip.lib().mevi_rq_beam_encode_f32(hip.ptr(x), bs, self.emb_size, hip.ptr(self.codebook), M, K, R,
                                               int(self.pq_type != "rq"), hip.ptr(labels), None if proba is None else hip.ptr(proba),
                                               hip.ptr(ws), ws.numel(), hip.stream_ptr())
        hip.check(st, "mevi_rq_beam_encode_f32")
        return (labels, proba) if return_proba else labels

    def _beam_search_steps(self, doc_emb, num_return_sequences, return_proba):
        """The per-level composition (MEVI_RQ_BEAM=steps, and every shape outside the fused call's envelope)."""
        L = hip.lib()
        R, M, K, dim = num_return_sequences, self.subvector_num, self.subvector_cents, self.last_dim
        pq = self.pq_type != "rq"
        x = self._rotated(doc_emb)
        bs = x.shape[0]
        resid, nb = x, 1
        scores = torch.ones((bs, 1), dtype=torch.float32, device=self.device)
        labels = torch.zeros((bs, 1, 0), dtype=torch.int32, device=self.device)
        base = torch.arange(bs, device=self.device)[:, None]
        for j in range(M):
            src_rows = x[:, j * dim:(j + 1) * dim].contiguous() if pq else resid
            nd = torch.empty((src_rows.shape[0], K), dtype=torch.float32, device=self.device)
            hip.check(L.mevi_rq_neg_dist_f32(hip.ptr(src_rows), src_rows.shape[0], dim, hip.ptr(self.codebook[j]), K,
                                             hip.ptr(nd), hip.stream_ptr()), "mevi_rq_neg_dist_f32")
            if pq and nb > 1:                      # one score row per document, repeated for each of its beams
                nd = nd[:, None, :].expand(bs, nb, K).reshape(bs * nb, K).contiguous()
            if R < nb * K:
                sc = torch.empty((bs, R), dtype=torch.float32, device=self.device)
                parent = torch.empty((bs, R), dtype=torch.int32, device=self.device)
                code = torch.empty((bs, R), dtype=torch.int32, device=self.device)
                hip.check(L.mevi_beam_step_f32(hip.ptr(nd), hip.ptr(scores), bs, nb, K, R, 2, hip.ptr(sc),
                                               hip.ptr(parent), hip.ptr(code), hip.stream_ptr()), "mevi_beam_step_f32")
                nb_new = R
            else:  # fewer candidates than beams: keep them all, in (beam, code) order
                from . import ops

                sc = ops.row_softmax(nd, log=False, scale=scores.reshape(-1)).reshape(bs, nb * K)
                parent = torch.arange(nb, device=self.device, dtype=torch.int32).repeat_interleave(K)[None].expand(bs, -1).contiguous()
                code = torch.arange(K, device=self.device, dtype=torch.int32).repeat(nb)[None].expand(bs, -1).contiguous()
                nb_new = nb * K
            labels = torch.cat([torch.gather(labels, 1, parent.long()[:, :, None].expand(-1, -1, labels.shape[2])),
                                code[:, :, None]], dim=2)
            if j != M - 1 and not pq:
                src = (base * nb + parent.long()).reshape(-1).contiguous()
                nxt = torch.empty((bs * nb_new, dim), dtype=torch.float32, device=self.device)
                hip.check(L.mevi_gather_sub_f32(hip.ptr(resid), hip.ptr(src), hip.ptr(self.codebook[j]),
                                                hip.ptr(code.reshape(-1).contiguous()), bs * nb_new, dim, hip.ptr(nxt),
                                                hip.stream_ptr()), "mevi_gather_sub_f32")
                resid = nxt
            scores, nb = sc, nb_new
        return (labels, scores) if return_proba else labels

    def get_topk_document_mapping(self, doc_embeddings, rank, nrank, num_return_sequences, batch_size=1 << 16):
        """Top-R code paths of this rank's contiguous slice of the corpus (pq.py:715-741: rows // nrank each, the last
        rank takes the rest): i32 [rows, R, M] on the CPU.  A CUDA tensor goes through the fused beam encode in one call
        over the whole slice with one copy back; host arrays (numpy / memmap) are uploaded `batch_size` rows at a time."""
        n = doc_embeddings.shape[0]
        per = n // nrank
        start, end = per * rank, n if rank + 1 == nrank else per * (rank + 1)
        on_device = torch.is_tensor(doc_embeddings) and doc_embeddings.is_cuda
        if on_device and self.pq_type != "opq" and self.beam_search_is_fused(num_return_sequences):
            return self.beam_search(doc_embeddings[start:end], num_return_sequences).cpu()   # one call, one copy back
        if self.pq_type == "opq":      # a chunk is rotated at a time: no second copy of the corpus exists
            from .ivfpq import ENCODE_CHUNK

            batch_size = ENCODE_CHUNK if on_device else min(batch_size, ENCODE_CHUNK)
        out = torch.empty((end - start, num_return_sequences, self.subvector_num), dtype=torch.int32)
        for s in range(start, end, batch_size):
            e = min(s + batch_size, end)
            x = doc_embeddings[s:e]
            x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
            out[s - start:e - start] = self.beam_search(x, num_return_sequences).cpu()
        return out

    def get_reconstruct_vector(self, index, codebook=None):
        """pq.get_reconstruct_vector (MEVI/pq.py:768-784): 'rq' = sum of the chosen centroids (level 0 first),
        'pq' = their concatenation (f32 [..., M * dsub])."""
        cb = self.codebook if codebook is None else codebook
        index = index.to(cb.device).long()
        if self.pq_type == "pq":
            return torch.cat([cb[j][index[..., j]] for j in range(cb.shape[0])], dim=-1)
        if self.pq_type == "opq":      # pq.py:775-783: the concatenation, rotated back into the input space (vectors @ rotate)
            from . import ops

            vectors = torch.cat([cb[j][index[..., j]] for j in range(cb.shape[0])], dim=-1)
            flat = ops.linear(vectors.reshape(-1, vectors.shape[-1]).contiguous(), self.rotate.t().contiguous())
            return flat.reshape(vectors.shape)
        out = torch.zeros(index.shape[:-1] + (cb.shape[-1],), dtype=torch.float32, device=cb.device)
        for j in range(cb.shape[0]):
            out = out + cb[j][index[..., j]]
        return out
