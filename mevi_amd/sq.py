"""Scalar-quantised indexes behind `faiss_search.py --param SQ8` / `SQ4` / `IVF<n>,SQ8` / `IVF<n>,SQ4`.

faiss builds `IndexScalarQuantizer(dim, QT_8bit | QT_4bit, METRIC_INNER_PRODUCT)`, or `IndexIVFScalarQuantizer` over an
`IndexFlatIP` quantiser with `by_residual = true`: one byte or one nibble per dimension, with a per-dimension range [vmin, vmin +
vdiff] trained as the minimum and maximum (RS_minmax, argument 0) of ALL rows -- of their residuals x - centroid[list of x] behind
an IVF.  With L = 255 or 15, every step one f32 operation (include/mevi_hip_sq.h):
  * encode: c = (int)(L * clamp((r - vmin) / vdiff, 0, 1)), 0 where vdiff == 0; 4 bits: dimension 2i in the low nibble of byte i;
  * decode: x^ = vmin + vdiff * ((c + 0.5f) / L), a rounded product and a rounded sum;
  * search: the sequential fmaf chain <q, x^> from +0, plus the coarse score <q, centroid> of the probed list as one f32 addition;
    top-k over all probed rows (score desc, id asc, -FLT_MAX / -1 padding).
Nothing here is random without an IVF, so a flat index -- range, codes and results -- is pinned bit for bit by the corpus; with
an IVF the same holds given the centroids (k-means is seeded from our own RNG, as for IVF-Flat).  Lists are `ivf.assign` /
`ivf.build_lists`: ids ascending inside a list, codes list-major.

`SQIndex.search` is two stream-ordered device calls: the coarse quantiser (mevi_ivf_scan_topk_f32 on the centroids as one list,
k = nprobe) and the scan (mevi_sq_scan_topk_f32, csrc/sq_scan.hip) with the coarse scores as the bias of every probe slot; a flat
index is the scan alone over its one list.  The result is approximate by construction; `search` also runs the exact search and
reports recall on stderr.
"""
import os
import re
import sys

import numpy as np
import torch

from . import dense, hip, ivf

TRAIN_CHUNK = 1 << 18             # rows whose residuals exist at a time while the range is trained


def parse_factory(param):
    """(nlist or None, bits) of 'SQ8', 'SQ4', 'IVF<n>,SQ8' and 'IVF<n>,SQ4', else None (SQ6, SQfp16, refinements, ...)."""
    g = re.fullmatch(r"\s*(?:IVF(\d+)\s*,\s*)?SQ([48])\s*", str(param))
    return (int(g.group(1)) if g.group(1) else None, int(g.group(2))) if g else None


def supported(nd, dim, topk, nlist, bits):
    """True when an index of this shape is inside the envelope of the scan (host arithmetic): bits 4 or 8, dim a multiple of 4 (8
    bits) or 8 (4 bits) up to 4096, 0 < nlist <= nd, topk <= 4096, and one query's candidates within the cap."""
    if nd < 1 or (nlist is not None and not 0 < nlist <= nd):
        return False
    return dense.sq_scan_workspace_bytes(1, 1, topk, dim, bits, 1 if nlist is None else nlist, nd) > 0


def wanted(param, nd, dim, topk):
    """(nlist or None, bits) when `dense.search` / `dense.profile` serve `param` with an SQIndex: the string parses, the shape is
    `supported` and MEVI_SQ is not 'exact' (which restores the exact answer these strings had before); else None."""
    spec = parse_factory(param)
    if spec is None or os.environ.get("MEVI_SQ", "index") == "exact" or not supported(nd, dim, topk, *spec):
        return None
    return spec


def train_range(docs, list_of=None, centroids=None, chunk=TRAIN_CHUNK):
    """(vmin, vdiff) f32 [dim]: minimum and maximum - minimum over ALL rows of docs (of docs - centroids[list_of] with an IVF), on
    the device, `chunk` rows at a time."""
    lo = hi = None
    for a in range(0, docs.shape[0], chunk):
        x = docs[a:a + chunk]
        if centroids is not None:
            x = x - centroids[list_of[a:a + chunk].long()]              # the f32 residual, one rounding per element
        mn, mx = torch.aminmax(x, dim=0)
        lo = mn if lo is None else torch.minimum(lo, mn)
        hi = mx if hi is None else torch.maximum(hi, mx)
    return lo.contiguous(), (hi - lo).contiguous()


def encode(docs, rows, list_of, centroids, vmin, vdiff, bits):
    """u8 [len(rows), dim * bits / 8]: the codes of docs[rows] in that order (rows None: of docs), straight from `docs`
    (mevi_sq_encode_f32 gathers, subtracts the centroid and quantises in one pass: no second f32 copy of the corpus)."""
    return dense.sq_encode(docs, rows, list_of, centroids, vmin, vdiff, bits)


def levels(bits):
    """f32 [2^bits]: T[c] = (c + 0.5f) / L, the f32 quotient (numpy on the host: no fused or approximated division)."""
    L = (1 << bits) - 1
    return (np.arange(L + 1, dtype=np.float32) + np.float32(0.5)) / np.float32(L)


def decode(codes, vmin, vdiff, bits):
    """f32 [n, dim]: the rows the scan scores, vmin + vdiff * T[c] as two rounded operations (two kernels).  For tests and reports."""
    if bits == 4:
        codes = torch.stack((codes & 15, codes >> 4), dim=2).reshape(codes.shape[0], -1)
    t = torch.from_numpy(levels(bits)).to(codes.device)[codes.long()]
    prod = torch.mul(vdiff, t)
    return torch.add(vmin, prod)


class SQIndex:
    """`index.train(doc); index.add(doc)` of 'IVF<n>,SQ<bits>' (nlist=None: 'SQ<bits>'): centroids, range, codes list by list."""

    def __init__(self, docs, nlist, bits, centroids=None, vmin=None, vdiff=None, seed=1234):
        assert docs.is_cuda and docs.dtype == torch.float32 and docs.dim() == 2 and bits in (4, 8)
        nd, dim = docs.shape
        dev = docs.device
        self.nlist, self.bits, self.dim = nlist, bits, dim
        if nlist is None:                                       # one list, no coarse quantiser, the id is the row
            self.centroids = self.list_of = self.ids = None
            self.offsets = torch.tensor([0, nd], dtype=torch.int64)
            self.offsets_dev = self.offsets.to(dev)
            self.max_list_len = nd
        else:
            self.centroids = ivf.train_centroids(docs, nlist, seed) if centroids is None else centroids.to(dev).contiguous()
            self.list_of = ivf.assign(docs, self.centroids)
            self.offsets, self.offsets_dev, self.ids, self.max_list_len = ivf.build_lists(self.list_of, nlist)
            self.centroid_offsets = torch.tensor([0, nlist], dtype=torch.int64, device=dev)   # the quantiser's one list
        if vmin is None or vdiff is None:
            vmin, vdiff = train_range(docs, self.list_of, self.centroids)
        self.vmin, self.vdiff = vmin.to(dev).contiguous(), vdiff.to(dev).contiguous()
        self.codes = encode(docs.contiguous(), self.ids, self.list_of, self.centroids, self.vmin, self.vdiff, bits)

    @property
    def n_lists(self):
        return 1 if self.nlist is None else self.nlist

    def clamp_nprobe(self, nprobe):
        return max(1, min(int(nprobe), self.n_lists))

    def search(self, query, k, nprobe=1):
        """(scores f32 [nq, k] desc, ids i64 [nq, k]; -FLT_MAX / -1 padding when the probed lists hold fewer than k)."""
        query = query.contiguous()
        zero = torch.zeros((query.shape[0], 1), dtype=torch.int32, device=query.device)
        if self.nlist is None:
            return dense.sq_scan_topk(query, self.codes, self.vmin, self.vdiff, self.bits, self.offsets_dev, None, self.max_list_len,
                                      zero, None, k)
        bias, lists = dense.ivf_scan_topk(query, self.centroids, self.centroid_offsets, None, self.nlist, zero, self.clamp_nprobe(nprobe))
        return dense.sq_scan_topk(query, self.codes, self.vmin, self.vdiff, self.bits, self.offsets_dev, self.ids, self.max_list_len,
                                  lists.to(torch.int32), bias, k)


def factory_name(nlist, bits):
    return ("" if nlist is None else f"IVF{nlist},") + f"SQ{bits}"


def search(query, docs, k, nlist, bits, nprobe=None, report=True):
    """faiss_search.search for 'IVF<n>,SQ<bits>' / 'SQ<bits>' on device tensors: train + add + search, recall vs exact on stderr."""
    hip.require_gpu()
    if nprobe is None:
        nprobe = int(os.environ.get("MEVI_IVF_NPROBE", "1"))
    index = SQIndex(docs, nlist, bits)
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
        print(f"[mevi_amd] {factory_name(nlist, bits)} nprobe={index.clamp_nprobe(nprobe)}: recall vs exact search " +
              ", ".join(f"@{c} {v:.4f}" for c, v in rec.items()) +
              f"; {index.codes.numel()} bytes of codes; lists: min {int(sizes.min())} / mean {float(sizes.float().mean()):.0f} / "
              f"max {int(sizes.max())} documents", file=sys.stderr)
    return s, i
