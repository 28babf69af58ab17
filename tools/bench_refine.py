"""The refine stage (faiss_search.py --param <index>,RFlat; mevi_amd/refine.py, csrc/refine_topk.hip) at C2 size on the
`ance_scale` corpus of tools/synth.py, in one process.  Four tables:
  call      mevi_refine_topk_f32 alone on the candidates of 'IVF100,PQ64' (nprobe 8): ms (median of 3 windows after a warm-up,
            tools/bench_ivf.py: timed) and gathered TB/s = valid candidates x dim x 4 bytes / s, per (nq, k, k_factor);
  torch     the same candidates through a torch composition -- per chunk of queries docs[ids] (a gather that materialises the
            rows), bmm, topk -- which has no bit parity with the exact search: the thing the kernel must not lose to;
  bodies    the score launch's bodies on the same candidates, mevi_refine_topk_set_score_body: the shipped one against the
            slab loop of fine_score_kernel (and, with --bodies, whatever else the library still carries);
  indexes   per inner index (PQ64, OPQ64,PQ64, IVF100,PQ64 at nprobe 1 / 8, SQ4) and top-k (1000, 10): ms and recall@10 / @1000
            of the bare index and of the index with refine at k_factor 1 and 4, beside IVF100,Flat (nprobe 1 / 8) and the exact
            search.
  python tools/bench_refine.py [--docs N] [--nq 1,8,32,6980] [--k 1000,10] [--k_factor 1,2,4] [--bodies 0,1] [--skip indexes]
                               [--niter 50] [--out table.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import synth  # noqa: E402
from bench_ivf import ints, recall, timed  # noqa: E402
from mevi_amd import dense, hip, ivf, ivfpq, opq, refine, sq  # noqa: E402

GUIDE_GATHER_TBS = (5.5, 5.8)           # random whole rows of 1-2 KiB fetched once, chip-wide (the only measured rate that applies)


def lap(fn, result=False):
    """Median seconds of one call: `timed` for short calls, 3 single calls after a warm-up for calls above 0.2 s.  result: (seconds,
    what the warm-up call returned)."""
    out = fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first = time.perf_counter() - t
    if first < 0.2:
        sec = timed([fn])[0]
    else:
        laps = [first]
        for _ in range(2):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            laps.append(time.perf_counter() - t)
        sec = statistics.median(laps)
    return (sec, out) if result else sec


def torch_refine(q, docs, cand, k, chunk_bytes=2 << 30):
    """Gather + bmm + topk in chunks of queries whose gathered rows stay below chunk_bytes.  -1 ids score -inf."""
    nq, n_cand = cand.shape
    step = max(1, chunk_bytes // (n_cand * docs.shape[1] * 4))
    out_s, out_i = [], []
    kk = min(k, n_cand)
    for a in range(0, nq, step):
        ids = cand[a:a + step]
        ok = ids >= 0
        rows = docs[ids.clamp_min(0)]                                        # [b, n_cand, dim]
        s = torch.bmm(rows, q[a:a + step, :, None])[:, :, 0].masked_fill_(~ok, float("-inf"))
        top = torch.topk(s, kk, dim=1)
        out_s.append(top.values)
        out_i.append(torch.gather(ids, 1, top.indices))
    return torch.cat(out_s), torch.cat(out_i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=bench.N_DOCS)
    ap.add_argument("--nq", default=f"1,8,32,{bench.N_QUERIES}")
    ap.add_argument("--k", default="1000,10")
    ap.add_argument("--k_factor", default="1,2,4")
    ap.add_argument("--bodies", default="0,1")
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--nlist", type=int, default=100)
    ap.add_argument("--niter", type=int, default=opq.NITER)
    ap.add_argument("--skip", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nqs, ks, factors, m = ints(a.nq), ints(a.k), ints(a.k_factor), a.m
    L = hip.lib()
    table = {"docs": a.docs, "corpus": "ance_scale", "m": m, "nlist": a.nlist, "guide_gather_TBps": list(GUIDE_GATHER_TBS),
             "note": "ms = median of 3 timed windows after a warm-up; gathered_TBps = valid candidates x dim x 4 bytes / s of the "
                     "refine call (both launches); share_of_guide = that over the guide's 5.5 and 5.8 TB/s for random whole rows "
                     "fetched once; torch_ms = chunked docs[ids] + bmm + topk on the same candidates (no bit parity); bodies: "
                     "the score launch's variants on the same call; indexes: inner_ms = the bare index's search for k, "
                     "refined_ms = the inner search for k_base plus the refine call, recalls against the exact search",
             "call": [], "bodies": [], "indexes": []}

    def save():
        if a.out:                                                # after every row: a long table survives a short limit
            with open(a.out, "w") as f:
                json.dump(table, f, indent=1)

    def emit(kind, row):
        table[kind].append(row)
        print(json.dumps(row), flush=True)
        save()

    docs, info = synth.corpus("ance_scale", dev, a.docs)
    dim = docs.shape[1]
    table["dim"] = dim
    q_all = synth.corpus_queries("ance_scale", docs, max(nqs), info)[0]
    exact = dense.DenseIndex(docs)
    kmax = max(ks)
    exact_ids = exact.search(q_all, kmax)[1]
    cent = ivf.train_centroids(docs, a.nlist)
    base = ivfpq.IVFPQIndex(docs, a.nlist, m, 8, centroids=cent)
    cand_all = base.search(q_all, min(4096, kmax * max(factors)), 8)[1]
    torch.cuda.synchronize()

    # ---- the call alone, the torch composition, the bodies ----------------------------------------------------------------
    for k in ks:
        for f in factors:
            n_cand = k * f
            for nq in nqs:
                q, cand = q_all[:nq].contiguous(), cand_all[:nq, :n_cand].contiguous()
                ws = torch.empty(dense.refine_topk_workspace_bytes(nq, n_cand, k, dim), dtype=torch.uint8, device=dev)
                out = dense.refine_topk(q, docs, cand, k, workspace=ws)
                run = lambda: dense.refine_topk(q, docs, cand, k, out=out, workspace=ws)      # noqa: E731
                t = lap(run)
                valid = int(out[2].sum().item())
                tbs = valid * dim * 4 / t / 1e12
                row = {"nq": nq, "k": k, "k_factor": f, "n_cand": n_cand, "valid_candidates": valid, "refine_ms": round(t * 1e3, 4),
                       "gathered_TBps": round(tbs, 3), "share_of_guide": [round(tbs / g, 3) for g in GUIDE_GATHER_TBS],
                       "query_tiles": -(-nq // dense.refine_topk_query_tile(nq, n_cand, k, dim)),
                       "recall": recall(out[1], exact_ids[:nq, :k])}
                if "torch" not in a.skip:
                    ts, ti = torch_refine(q, docs, cand, k)
                    row["torch_ms"] = round(lap(lambda: torch_refine(q, docs, cand, k)) * 1e3, 4)
                    row["torch_over_refine"] = round(row["torch_ms"] / row["refine_ms"], 2)
                    row["torch_same_ids"] = float((ti == out[1][:, :ti.shape[1]]).float().mean().item())
                    del ts, ti
                emit("call", row)
                if nq == max(nqs) and "bodies" not in a.skip:
                    for body in ints(a.bodies):
                        L.mevi_refine_topk_set_score_body(body)
                        tb = lap(run)
                        L.mevi_refine_topk_set_score_body(0)
                        emit("bodies", {"nq": nq, "k": k, "n_cand": n_cand, "body": body, "refine_ms": round(tb * 1e3, 4),
                                        "gathered_TBps": round(valid * dim * 4 / tb / 1e12, 3)})
                del ws, out
                torch.cuda.empty_cache()
    if "indexes" in a.skip:
        return

    # ---- the indexes with and without refine ----------------------------------------------------------------------------------
    nq = max(nqs)
    q = q_all[:nq].contiguous()
    for k in ks:
        emit("indexes", {"index": "Flat (exact)", "k": k, "nq": nq, "inner_ms": round(lap(lambda: exact.search(q, k)) * 1e3, 3),
                         "inner_recall": recall(exact_ids[:nq, :k], exact_ids[:nq, :k])})
    flat = ivf.IVFFlatIndex(docs, a.nlist, centroids=cent)
    for nprobe in (1, 8):
        for k in ks:
            t, found = lap(lambda: flat.search(q, k, nprobe), result=True)
            emit("indexes", {"index": f"IVF{a.nlist},Flat", "nprobe": nprobe, "k": k, "nq": nq, "inner_ms": round(t * 1e3, 3),
                             "inner_recall": recall(found[1], exact_ids[:nq, :k])})
    del flat
    torch.cuda.empty_cache()

    def rows_of(name, index, nprobes):
        ref = refine.RefineIndex(index, docs)
        for nprobe in nprobes:
            for k in ks:
                t, found = lap(lambda: index.search(q, k, nprobe), result=True)
                row = {"index": name, "nprobe": nprobe, "k": k, "nq": nq, "inner_ms": round(t * 1e3, 3),
                       "inner_recall": recall(found[1], exact_ids[:nq, :k])}
                for f in (1, 4):
                    if k * f > refine.MAX_K_BASE:
                        continue
                    t, found = lap(lambda: ref.search(q, k, nprobe, k_factor=f), result=True)
                    row[f"refined_x{f}_ms"] = round(t * 1e3, 3)
                    row[f"refined_x{f}_recall"] = recall(found[1], exact_ids[:nq, :k])
                    row[f"refined_x{f}_valid_mean"] = round(float(ref.last_candidates[1].float().mean().item()), 1)
                emit("indexes", row)

    rows_of(f"IVF{a.nlist},PQ{m}", base, (1, 8))
    del base
    torch.cuda.empty_cache()
    rows_of(f"PQ{m}", ivfpq.IVFPQIndex(docs, None, m, 8), (1,))
    torch.cuda.empty_cache()
    rows_of(f"OPQ{m},PQ{m}", opq.OPQIndex(docs, m, None, m, 8, False, niter=a.niter), (1,))
    torch.cuda.empty_cache()
    rows_of("SQ4", sq.SQIndex(docs, None, 4), (1,))


if __name__ == "__main__":
    main()
