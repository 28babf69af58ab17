"""A learned rotation in front of a product quantiser: `faiss_search.py --param OPQ<M>,[IVF<n>,]PQ<m>[x<b>]` / `...,PQ<m>x4fs`.

faiss builds `IndexPreTransform(OPQMatrix(dim, M), IndexPQ / IndexIVFPQ / their fast-scan forms)` for these strings.  A product
quantiser gives every subspace the same number of centroids whatever variance the subspace carries; OPQ (Ge, He, Ke, Sun 2013)
learns an orthonormal R that spreads the variance over the subspaces before the rows are coded.  R is square, so
<R q, R x> = <q, x>: nothing is added per scanned row, and the scans are those of mevi_amd/ivfpq.py and mevi_amd/pqfs.py.

The trainer (`train_rotation`) follows `OPQMatrix::train` in structure and defaults -- at most 256 * 256 raw rows, a random
orthonormal start, 50 iterations of {rotate, k-means of every subspace (40 iterations the first time, 4 hot-started ones
afterwards), encode, Procrustes} with a training quantiser of M x 256 centroids -- with our own random numbers, as for every
k-means here.  Rotation, k-means, encode, decode and C = Y^^T X run on the device; the dim x dim SVD runs on the host in float64.

The index (`OPQIndex`) is an IVFPQIndex or PQFSIndex with `rotation=R`.  With chain(x, R)[o] = the sequential fmaf chain of
mevi_gemm_nt_f32 over row o of R, every step is one pinned f32 operation:
  * the coarse quantiser stays in the INPUT space: centroids, `ivf.assign`, lists and the coarse search of the queries are those
    of 'IVF<n>,PQ<m>' (faiss rotates first and clusters the rotated rows: another k-means input, the same index up to rounding);
  * crot = chain(centroids, R); the rotated residual of a row is y = chain(x, R) - crot[list of x], one f32 subtraction per element
    (no coarse quantiser: y = chain(x, R)) -- mevi_opq_rotate_rows_f32, a chunk of gathered rows in one launch;
  * the codebook is `ivfpq.train_codebook`'s sample and training applied to y; the codes are mevi_pq_encode_f32(y);
  * search: qr = chain(q, R) (one GEMM launch), the coarse scores and the probe table from the unrotated q, then the ADC scan over
    qr with those scores as bias: score = <q, c> + sum_j lut_qr[j][code_j] (include/mevi_hip_ivfpq.h).
"""
import os
import re
import sys
import time

import numpy as np
import torch

from . import dense, hip, ivf, ivfpq, pqfs, rq

TRAIN_K = 256                     # centroids per subspace of the training quantiser (faiss: 8 bits whatever the index uses)
MAX_TRAIN_ROWS = 256 * TRAIN_K    # OPQMatrix::max_train_points
NITER, NITER_PQ_0, NITER_PQ = 50, 40, 4
GRAPH_MAX_QUERIES = ivf.GRAPH_MAX_QUERIES

LAST_TRAIN = {}                   # seconds of the last train_rotation: {"niter", "device_s", "svd_s"}


def parse_factory(param):
    """(M, dout or None, nlist or None, m, nbits, fs) of 'OPQ<M>[_<dout>],' in front of a string `ivfpq.parse_factory` (fs False)
    or `pqfs.parse_factory` (fs True, nbits 4) takes; else None."""
    g = re.fullmatch(r"\s*OPQ(\d+)(?:_(\d+))?\s*,(.*)", str(param), flags=re.S)
    if not g:
        return None
    M, dout = int(g.group(1)), (int(g.group(2)) if g.group(2) else None)
    fs = pqfs.parse_factory(g.group(3))
    if fs is not None:
        return (M, dout, fs[0], fs[1], pqfs.NBITS, True)
    pq = ivfpq.parse_factory(g.group(3))
    if pq is not None:
        return (M, dout, pq[0], pq[1], pq[2], False)
    return None


def supported(nd, dim, topk, M, nlist, m, nbits, fs):
    """True when the rotation can be trained (dim = M subspaces of a multiple of 4 columns, at least TRAIN_K rows) and the inner
    index is inside its own envelope."""
    if M < 1 or dim % M != 0 or (dim // M) % 4 != 0 or dim > dense.OPQ_MAX_DIM or nd < TRAIN_K:
        return False
    return pqfs.supported(nd, dim, topk, nlist, m) if fs else ivfpq.supported(nd, dim, topk, nlist, m, nbits)


def wanted(param, nd, dim, topk):
    """(M, nlist or None, m, nbits, fs) when `dense.search` / `dense.profile` serve `param` with an OPQIndex: the string parses, a
    given <dout> equals dim (a reducing rotation does not preserve inner products), the shape is `supported` and MEVI_OPQ is not
    'exact' (which restores the exact answer these strings had before); else None."""
    spec = parse_factory(param)
    if spec is None or os.environ.get("MEVI_OPQ", "index") == "exact" or (spec[1] is not None and spec[1] != dim):
        return None
    spec = (spec[0],) + spec[2:]
    return spec if supported(nd, dim, topk, *spec) else None


def random_rotation(dim, seed):
    """A seeded random orthonormal matrix, float64 [dim, dim]: the Q of a Gaussian matrix's QR with the signs of R's diagonal."""
    a = np.random.default_rng(int(seed)).standard_normal((dim, dim))
    q, r = np.linalg.qr(a)
    return q * np.where(np.diag(r) < 0, -1.0, 1.0)[None, :]


def decode(codes, codebook):
    """f32 [n, M * dsub]: the centroids the codes name, subspace by subspace (a gather)."""
    M = codebook.shape[0]
    sub = torch.arange(M, device=codes.device)[None, :]
    return codebook[sub, codes.long()].reshape(codes.shape[0], -1)


def train_rotation(docs, M, K=TRAIN_K, niter=None, niter_pq_0=NITER_PQ_0, niter_pq=NITER_PQ, seed=1234):
    """(R f32 [dim, dim], errors): the rotation of `OPQMatrix::train` for M subspaces and the quantisation error ||Y - Y^||^2 / n
    (float64) of every iteration's rotated sample under that iteration's codebook.  niter None: MEVI_OPQ_NITER or 50."""
    from . import ops

    hip.require_gpu()
    assert docs.is_cuda and docs.dtype == torch.float32 and docs.dim() == 2
    nd, dim = docs.shape
    assert dim % M == 0 and (dim // M) % 4 == 0 and nd >= K, (nd, dim, M, K)
    if niter is None:
        niter = int(os.environ.get("MEVI_OPQ_NITER", str(NITER)))
    dev, dsub = docs.device, dim // M
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    n = min(nd, MAX_TRAIN_ROWS)
    X = docs[torch.randperm(nd, generator=gen, device=dev)[:n]].contiguous()    # raw rows: the transform is trained before the IVF
    start = torch.randperm(n, generator=gen, device=dev)[:K]                    # the rows whose slices seed the first k-means
    XT = torch.zeros((dim, (n + 3) // 4 * 4), dtype=torch.float32, device=dev)  # K of the Procrustes GEMM, padded to the float4 loads
    XT[:, :n] = X.t()
    YT = torch.zeros_like(XT)
    R = torch.from_numpy(random_rotation(dim, seed).astype(np.float32)).to(dev)
    errors, book = [], None
    t_dev = t_svd = 0.0
    for t in range(int(niter)):
        torch.cuda.synchronize()
        t0 = time.time()
        Y = ops.linear(X, R)                                                    # Y = X R^T
        if book is None:
            book = Y[start].view(K, M, dsub).permute(1, 0, 2).contiguous()
        book = rq.pq_lloyd(Y, book, niter_pq_0 if t == 0 else niter_pq)
        Yh = decode(rq.pq_encode_groups(Y, book), book)
        errors.append(float(((Y.double() - Yh.double()) ** 2).sum().item()) / n)
        YT[:, :n] = Yh.t()
        C = ops.linear(YT, XT).cpu().numpy().astype(np.float64)                 # C = Y^^T X, [dim, dim]
        t1 = time.time()
        U, _, Vt = np.linalg.svd(C)                                             # Procrustes: R = argmin ||X R^T - Y^|| = U V^T
        R = torch.from_numpy((U @ Vt).astype(np.float32)).to(dev)
        t_dev += t1 - t0
        t_svd += time.time() - t1
    LAST_TRAIN.clear()
    LAST_TRAIN.update(niter=int(niter), device_s=t_dev, svd_s=t_svd)
    return R, errors


class OPQIndex:
    """`index.train(doc); index.add(doc)` of 'OPQ<M>,[IVF<n>,]PQ<m>x<b>' (fs: '...PQ<m>x4fs'): the rotation and, behind it,
    `self.inner` = an IVFPQIndex / PQFSIndex built with `rotation=R`, whose search rotates the queries for the ADC scan only."""

    def __init__(self, docs, M, nlist, m, nbits=8, fs=False, R=None, centroids=None, codebook=None, seed=1234, niter=None):
        self.M, self.fs = M, fs
        self.errors = None
        if R is None:
            R, self.errors = train_rotation(docs, M, niter=niter, seed=seed)
        self.R = R.to(docs.device).contiguous()
        if fs:
            assert nbits == pqfs.NBITS
            self.inner = pqfs.PQFSIndex(docs, nlist, m, centroids=centroids, codebook=codebook, seed=seed, rotation=self.R)
        else:
            self.inner = ivfpq.IVFPQIndex(docs, nlist, m, nbits, centroids=centroids, codebook=codebook, seed=seed, rotation=self.R)

    def __getattr__(self, name):            # centroids, codebook, codes, offsets, ids, clamp_nprobe, ... are the inner index's
        if name == "inner":
            raise AttributeError(name)
        return getattr(self.inner, name)

    def search(self, query, k, nprobe=1):
        """(scores f32 [nq, k] desc, ids i64 [nq, k]): one GEMM on the queries, the coarse call, the ADC scan."""
        return self.inner.search(query, k, nprobe)

    def search_scan(self, query, k, nprobe, buffers=None):
        return self.inner.search_scan(query, k, nprobe, buffers)

    def search_graph(self, nq, k, nprobe=1):
        """A captured graph of `search` for exactly nq <= GRAPH_MAX_QUERIES queries, the rotation inside it."""
        return self.inner.search_graph(nq, k, nprobe)


def factory_name(M, nlist, m, nbits, fs):
    return f"OPQ{M}," + (pqfs.factory_name(nlist, m) if fs else ivfpq.factory_name(nlist, m, nbits))


def search(query, docs, k, M, nlist, m, nbits=8, fs=False, nprobe=None, report=True):
    """faiss_search.search for the OPQ strings on device tensors: train + add + search; recall vs exact, the trainer's iterations
    and first / last error and the bytes of codes on stderr."""
    hip.require_gpu()
    if nprobe is None:
        nprobe = int(os.environ.get("MEVI_IVF_NPROBE", "1"))
    index = OPQIndex(docs, M, nlist, m, nbits, fs)
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
        print(f"[mevi_amd] {factory_name(M, nlist, m, nbits, fs)} nprobe={index.clamp_nprobe(nprobe)}: recall vs exact search " +
              ", ".join(f"@{c} {v:.4f}" for c, v in rec.items()) +
              f"; rotation: niter {len(index.errors)}, training error {index.errors[0]:.6g} -> {index.errors[-1]:.6g} "
              f"({LAST_TRAIN['device_s']:.2f} s on the device, {LAST_TRAIN['svd_s']:.2f} s of host SVD)"
              f"; {index.codes.numel()} bytes of codes; lists: min {int(sizes.min())} / mean {float(sizes.float().mean()):.0f} / "
              f"max {int(sizes.max())} documents", file=sys.stderr)
    return s, i
