"""Residual-quantiser indexes (faiss_search.py --param RQ<M>x<b> / IVF<n>,RQ<M>x<b>) against the product-quantiser indexes of the same
bytes per row, at C2 size on the `ance_scale` corpus of tools/synth.py, in one process.  Groups compared at equal bytes:
  flat, 64 bytes    RQ64x8 | PQ64 | OPQ64,PQ64
  IVF100, 64 bytes  IVF100,RQ64x8 | IVF100,PQ64      (nprobe 1 and 8)
  flat, 32 bytes    RQ32x8 | PQ32
Per index: build seconds split into coarse training, codebook training (for OPQ: + the rotation) and add (lists + encode; for RQ the
encode's residual passes are timed again by themselves), bytes of codes, the training error per level.  Per (group, nprobe, query
count, k): ms of the whole search of every index of the group (median of 3 timed windows after a warm-up, the indexes taking turns:
tools/bench_ivf.py: timed), for RQ the ms of the table kernel alone (dense.aq_lut on the same queries) beside the product
quantiser's search -- same scan body, same bytes, so the gap is the tables --, recall@1/10/k against the exact search, and the recall
behind ',RFlat' at MEVI_REFINE_K_FACTOR 1 and 4 (k_base <= 4096).
  python tools/bench_rqindex.py [--docs N] [--nq 6980,32,8,1] [--k 10,1000] [--groups flat64,ivf64,flat32] [--out table.json]
  python tools/bench_rqindex.py --trace      # builds RQ64x8 and searches it 3 times per query count: the run to put under a kernel trace
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import synth  # noqa: E402
from bench_ivf import ints, recall, timed  # noqa: E402
from mevi_amd import dense, ivf, ivfpq, opq, refine, rqindex  # noqa: E402

GROUPS = {"flat64": (None, 64, (1,)), "ivf64": (100, 64, (1, 8)), "flat32": (None, 32, (1,))}     # nlist, bytes a row, nprobes


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, round(time.perf_counter() - t, 3)


def residual_passes(index, docs):
    """Seconds of the M / 8 - 1 in-place residual calls of every chunk of the encode alone (on the chunk's own rows; the codes are
    the index's)."""
    M = index.M
    groups = [index.codebook[g:g + rqindex.ENCODE_MAX_LEVELS].contiguous() for g in range(0, M, rqindex.ENCODE_MAX_LEVELS)]
    total = 0.0
    for a in range(0, docs.shape[0], rqindex.ENCODE_CHUNK):
        rows = index.ids[a:a + rqindex.ENCODE_CHUNK]
        x = docs[rows].contiguous()
        codes = index.codes[a:a + rqindex.ENCODE_CHUNK].to(torch.int32)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i, book in enumerate(groups[:-1]):
            dense.rq_residual(x, book, codes[:, i * rqindex.ENCODE_MAX_LEVELS:], out=x)
        torch.cuda.synchronize()
        total += time.perf_counter() - t
    return round(total, 3)


def build_rq(docs, nlist, M, cent, t_coarse):
    stats = {}
    list_of = ivf.assign(docs, cent) if cent is not None else None
    book, t_train = clock(lambda: rqindex.train_codebook(docs, list_of, cent, M, 8, stats=stats))
    index, t_add = clock(lambda: rqindex.RQIndex(docs, nlist, M, 8, centroids=cent, codebook=book))
    info = {"index": rqindex.factory_name(nlist, M, 8), "train_coarse_s": t_coarse, "train_codebook_s": t_train, "add_s": t_add,
            "residual_passes_s": residual_passes(index, docs), "code_bytes": index.codes.numel(), "train_rows": stats["train_rows"],
            "input_mse": stats["input_mse"], "level_mse": [round(v, 6) for v in stats["level_mse"]]}
    return index, info


def build_pq(docs, nlist, m, cent, t_coarse):
    list_of = ivf.assign(docs, cent) if cent is not None else None
    book, t_train = clock(lambda: ivfpq.train_codebook(docs, list_of, cent, m, 8))
    index, t_add = clock(lambda: ivfpq.IVFPQIndex(docs, nlist, m, 8, centroids=cent, codebook=book))
    return index, {"index": ivfpq.factory_name(nlist, m, 8), "train_coarse_s": t_coarse, "train_codebook_s": t_train, "add_s": t_add,
                   "code_bytes": index.codes.numel()}


def build_opq(docs, nlist, m, cent, t_coarse, niter):
    (R, errors), t_rot = clock(lambda: opq.train_rotation(docs, m, niter=niter))
    index, t_add = clock(lambda: opq.OPQIndex(docs, m, nlist, m, 8, False, R=R, centroids=cent))
    return index, {"index": f"OPQ{m}," + ivfpq.factory_name(nlist, m, 8), "train_coarse_s": t_coarse, "train_rotation_s": t_rot,
                   "train_codebook_and_add_s": t_add, "code_bytes": index.codes.numel(), "opq_error_first": errors[0],
                   "opq_error_last": errors[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=bench.N_DOCS)
    ap.add_argument("--nq", default=f"{bench.N_QUERIES},32,8,1")
    ap.add_argument("--k", default="10,1000")
    ap.add_argument("--groups", default="flat64,ivf64,flat32")
    ap.add_argument("--niter", type=int, default=opq.NITER)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nqs, ks = ints(a.nq), ints(a.k)
    docs, info = synth.corpus("ance_scale", dev, a.docs)
    dim = docs.shape[1]
    q_all = synth.corpus_queries("ance_scale", docs, max(nqs), info)[0]

    if a.trace:                                                  # nothing timed here: the trace is the measurement
        index, b = build_rq(docs, None, 64, None, 0.0)
        for nq in nqs:
            for _ in range(3):
                index.search(q_all[:nq].contiguous(), max(ks))
        torch.cuda.synchronize()
        print(json.dumps({"traced": b["index"], "nq": nqs, "k": max(ks), "searches_per_nq": 3}))
        return

    table = {"docs": a.docs, "dim": dim, "corpus": "ance_scale", "niter_opq": a.niter,
             "note": "ms = the whole search (coarse + tables + scan + select; OPQ: + the rotation GEMM), median of 3 windows after a "
                     "warm-up, the indexes of a group taking turns; lut_ms = dense.aq_lut on the same queries alone (the table kernel); "
                     "recall vs the exact search at 1 / 10 / k; rflat = recall behind ',RFlat' at k_factor 1 and 4 (null: k_base > 4096); "
                     "level_mse = mean squared residual norm of the training sample after each level (input_mse before)",
             "builds": [], "rows": []}

    def save():
        if a.out:                                                # after every row: a long table survives a short limit
            with open(a.out, "w") as f:
                json.dump(table, f, indent=1)

    exact_ids = dense.DenseIndex(docs).search(q_all, max(ks))[1]
    torch.cuda.empty_cache()
    for group in a.groups.split(","):
        nlist, nbytes, nprobes = GROUPS[group]
        cent, t_coarse = clock(lambda: ivf.train_centroids(docs, nlist)) if nlist else (None, 0.0)
        members = [build_rq(docs, nlist, nbytes, cent, t_coarse), build_pq(docs, nlist, nbytes, cent, t_coarse)]
        if group == "flat64":
            members.append(build_opq(docs, nlist, nbytes, cent, t_coarse, a.niter))
        for _, b in members:
            b["group"] = group
            table["builds"].append(b)
            print(json.dumps(b), flush=True)
        save()
        rq_index = members[0][0]
        for nprobe in nprobes:
            for nq in nqs:
                q = q_all[:nq].contiguous()
                for k in ks:
                    fns = [(lambda ix=ix: ix.search_scan(q, k, nprobe)) for ix, _ in members] + [lambda: dense.aq_lut(q, rq_index.codebook)]
                    laps = timed(fns)
                    row = {"group": group, "nprobe": nprobe, "nq": nq, "k": k, "lut_ms": round(laps[-1] * 1e3, 4), "indexes": {}}
                    for (ix, b), t in zip(members, laps):
                        ids = ix.search_scan(q, k, nprobe)[1]
                        r = {"ms": round(t * 1e3, 4), "recall": recall(ids, exact_ids[:nq, :k])}
                        rflat = {}
                        for f in (1, 4):
                            if refine.k_base(k, f) <= refine.MAX_K_BASE:
                                ri = refine.RefineIndex(ix, docs).search(q, k, nprobe, k_factor=f)[1]
                                rflat[str(f)] = recall(ri, exact_ids[:nq, :k])
                            else:
                                rflat[str(f)] = None
                        r["rflat"] = rflat
                        row["indexes"][b["index"]] = r
                    pq_ms = row["indexes"][members[1][1]["index"]]["ms"]
                    rq_ms = row["indexes"][members[0][1]["index"]]["ms"]
                    row["rq_over_pq"] = round(rq_ms / pq_ms, 3)
                    row["lut_share_of_rq"] = round(row["lut_ms"] / rq_ms, 3)
                    table["rows"].append(row)
                    print(json.dumps(row), flush=True)
                    save()
        del members, rq_index
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
