"""Exact re-ranking behind the compressed indexes: `faiss_search.py --param <index>,RFlat` / `<index>,Refine(Flat)`.

faiss builds `IndexRefineFlat(<index>)` for these strings: the base index returns k_base = k * k_factor candidates, they are scored
against the original rows (an IndexFlat beside the base index) and the best k are kept.  Here the original f32 rows are resident
on the device anyway -- `dense.search` uploads them before any index is built -- so `RefineIndex` keeps a reference to them, not a
copy, and the second stage is one device call (mevi_refine_topk_f32, csrc/refine_topk.hip): a gather of the candidates' rows with
the exact search's pinned fmaf chain and an LDS sort.  Every returned score is a bit of the exact search; what stays approximate
is which rows were among the candidates.

<index> is one of the compressed families: 'PQ<m>[x<b>]' / 'IVF<n>,PQ<m>[x<b>]' (mevi_amd/ivfpq.py), '...PQ<m>x4fs'
(mevi_amd/pqfs.py), 'OPQ<M>,...' (mevi_amd/opq.py), 'SQ8' / 'SQ4' / 'IVF<n>,SQ8' / 'IVF<n>,SQ4' (mevi_amd/sq.py), 'RQ<M>x<b>' / 'IVF<n>,RQ<M>x<b>' (mevi_amd/rqindex.py).
k_factor = MEVI_REFINE_K_FACTOR (a float, faiss's default 1, below 1 taken as 1), k_base = int(k * k_factor) as in faiss; the
scans return at most 4096 candidates, so a k_base above that keeps the exact search, as does MEVI_REFINE=exact.

Not served, and answered by the exact search as before: 'Refine(<anything but Flat>)' (a second compressed copy of the rows), a
refine behind 'Flat', 'IVF<n>,Flat' or 'HNSW<M>' (their scores are exact already), two refine suffixes.  `RefineIndex` has no
captured-graph `search_graph` and no sharded form under torchrun.
"""
import os
import re
import sys

import torch

from . import dense, hip, ivf, ivfpq, opq, pqfs, rqindex, sq

FAMILIES = {"opq": opq, "ivfpq": ivfpq, "pqfs": pqfs, "sq": sq, "rqindex": rqindex}     # in the order their parsers are asked
MAX_K_BASE = 4096                                                    # the list length of the scans


def split_factory(param):
    """(inner string, True) with a trailing ',RFlat' / ',Refine(Flat)' taken off, else (param, False)."""
    g = re.fullmatch(r"(.*),\s*(?:RFlat|Refine\(\s*Flat\s*\))\s*", str(param), flags=re.S)
    return (g.group(1), True) if g else (str(param), False)


def parse_factory(param):
    """(family, inner_spec) of '<index>,RFlat' and '<index>,Refine(Flat)': family in 'opq' / 'ivfpq' / 'pqfs' / 'sq' / 'rqindex' and inner_spec
    what that module's `parse_factory` returns for <index>; else None ('Refine(SQ8)', a refine behind 'Flat' / 'IVF<n>,Flat' /
    'HNSW<M>', two refine suffixes, no suffix)."""
    inner, found = split_factory(param)
    if not found:
        return None
    for name, mod in FAMILIES.items():
        spec = mod.parse_factory(inner)
        if spec is not None:
            return name, spec
    return None


def default_k_factor():
    """MEVI_REFINE_K_FACTOR as a float, 1 when unset; values below 1 (and NaN) are 1."""
    f = float(os.environ.get("MEVI_REFINE_K_FACTOR", "1"))
    return f if f >= 1.0 else 1.0


def k_base(k, k_factor=None):
    """Candidates the inner index is asked for: int(k * k_factor), faiss's IndexRefine::search."""
    f = default_k_factor() if k_factor is None else max(1.0, float(k_factor))
    return int(k * f)


def wanted(param, nd, dim, topk):
    """(family, spec) when `dense.search` / `dense.profile` serve `param` with a RefineIndex -- spec is what the family's own
    `wanted` returns for the inner string at k_base --; None when the string does not parse, MEVI_REFINE is 'exact', k_base is
    above the scans' 4096 or the inner family refuses (its own switch, its envelope)."""
    parsed = parse_factory(param)
    if parsed is None or os.environ.get("MEVI_REFINE", "index") == "exact":
        return None
    kb = k_base(topk)
    if kb > MAX_K_BASE or dense.refine_topk_workspace_bytes(1, kb, topk, dim) < 1:
        return None
    spec = FAMILIES[parsed[0]].wanted(split_factory(param)[0], nd, dim, kb)
    return None if spec is None else (parsed[0], spec)


def build_inner(docs, family, spec, **given):
    """The inner index of a family: OPQIndex / IVFPQIndex / PQFSIndex / SQIndex / RQIndex(docs, *spec, **given)."""
    cls = {"opq": opq.OPQIndex, "ivfpq": ivfpq.IVFPQIndex, "pqfs": pqfs.PQFSIndex, "sq": sq.SQIndex, "rqindex": rqindex.RQIndex}[family]
    return cls(docs, *spec, **given)


class RefineIndex:
    """faiss IndexRefineFlat: `inner` (any index with `search(query, k, nprobe)` -> (scores, ids i64 with -1 padding)) and the
    rows its ids name.  `docs` is referenced, not copied."""

    def __init__(self, inner, docs):
        assert docs.is_cuda and docs.dtype == torch.float32 and docs.dim() == 2 and docs.is_contiguous()
        self.inner, self.docs = inner, docs
        self.last_candidates = None     # (ids i64 [nq, k_base], nvalid i32 [nq]) of the last search

    def __getattr__(self, name):        # offsets, codes, clamp_nprobe, ... are the inner index's
        if name == "inner":
            raise AttributeError(name)
        return getattr(self.inner, name)

    def search(self, query, k, nprobe=1, k_factor=None):
        """(scores f32 [nq, k] desc, ids i64 [nq, k]): the inner search for k_base = int(k * k_factor) candidates, then one
        `dense.refine_topk` call.  Padding -FLT_MAX / -1 where the inner index returned fewer than k rows."""
        query = query.contiguous()
        _, cand = self.inner.search(query, k_base(k, k_factor), nprobe)
        s, i, nvalid = dense.refine_topk(query, self.docs, cand, k)
        self.last_candidates = (cand, nvalid)
        return s, i


def factory_name(family, spec):
    return FAMILIES[family].factory_name(*spec) + ",RFlat"


def _recall(ids, exact):
    rec = {}
    nq = ids.shape[0]
    for a in range(0, nq, 256):                                  # in chunks of queries: the comparison tensor is [nq, c, c]
        part = ivf.recall_report(ids[a:a + 256, :exact.shape[1]], exact[a:a + 256])
        for c, v in part.items():
            rec[c] = rec.get(c, 0.0) + v * min(256, nq - a)
    return {c: v / max(1, nq) for c, v in rec.items()}


def search(query, docs, k, family, spec, nprobe=None, k_factor=None, report=True):
    """faiss_search.search for '<index>,RFlat' on device tensors: train + add of the inner index, search, refine.  On stderr: recall
    vs the exact search of the refined list and of the inner index's own first k, k_factor, k_base, the mean valid candidates."""
    hip.require_gpu()
    if nprobe is None:
        nprobe = int(os.environ.get("MEVI_IVF_NPROBE", "1"))
    index = RefineIndex(build_inner(docs, family, spec), docs)
    s, i = index.search(query, k, nprobe, k_factor)
    if report:
        cand, nvalid = index.last_candidates
        _, ei = dense.DenseIndex(docs).search(query, min(k, 4096))
        fmt = lambda rec: ", ".join(f"@{c} {v:.4f}" for c, v in rec.items())          # noqa: E731
        f = default_k_factor() if k_factor is None else max(1.0, float(k_factor))
        print(f"[mevi_amd] {factory_name(family, spec)} nprobe={index.clamp_nprobe(nprobe)}: recall vs exact search refined "
              f"{fmt(_recall(i, ei))}; inner first {k} {fmt(_recall(cand[:, :k], ei))}; k_factor {f:g}, k_base {cand.shape[1]}, "
              f"valid candidates per query: mean {float(nvalid.float().mean()) if nvalid.numel() else 0.0:.1f}", file=sys.stderr)
    return s, i
