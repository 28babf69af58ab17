"""IVF-Flat (faiss_search.py --param IVF<n>,Flat) at C2 size on the synthetic corpus: build time, then per regime the device
scan (IVFFlatIndex.search_scan) against the host loop over lists (search_lists) in one process -- same bits checked, median of
3 timed windows after a warm-up, the two paths alternating -- with recall vs exact, the exact search's own time
(DenseIndex.search), the replayed graph's latency for up to 32 queries, and the rate at which the scan call reads the rows of
the probed lists.
  python tools/bench_ivf.py [nlist,...] [nprobe,...] [--nq 1,8,32,6980] [--k 1000] [--docs N] [--out table.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from mevi_amd import dense, ivf  # noqa: E402

HBM_PEAK = 8.0e12       # bytes/s, MI355X


def ints(text):
    return [int(v) for v in str(text).split(",")]


def timed(fns, min_window=0.05, max_iters=50):
    """Median seconds per call of every function of `fns`: one warm-up call each (it also sizes the window), then 3 windows per
    function, the functions taking turns."""
    iters = []
    for fn in fns:
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        iters.append(max(1, min(max_iters, int(min_window / max(time.perf_counter() - t, 1e-6)))))
    laps = [[] for _ in fns]
    for _ in range(3):
        for j, fn in enumerate(fns):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(iters[j]):
                fn()
            torch.cuda.synchronize()
            laps[j].append((time.perf_counter() - t) / iters[j])
    return [statistics.median(x) for x in laps]


def recall(ids, exact_ids):
    rec = {}
    n = ids.shape[0]
    for a in range(0, n, 256):
        for c, v in ivf.recall_report(ids[a:a + 256], exact_ids[a:a + 256]).items():
            rec[c] = rec.get(c, 0.0) + v * min(256, n - a) / n
    return {str(c): round(v, 4) for c, v in rec.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("nlist", nargs="?", default="100")
    ap.add_argument("nprobe", nargs="?", default="1,4,16")
    ap.add_argument("--nq", default=f"1,8,32,{bench.N_QUERIES}")
    ap.add_argument("--k", type=int, default=bench.TOPK)
    ap.add_argument("--docs", type=int, default=bench.N_DOCS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    docs = bench.gen_shard(0, a.docs, dev, a.docs)
    nqs = ints(a.nq)
    q_all = bench.gen_queries(max(nqs), dev, a.docs)
    k = a.k
    flat = dense.DenseIndex(docs).prepare_small()
    rows = []
    exact = {}
    for nq in nqs:
        q = q_all[:nq].contiguous()
        (t_exact,) = timed([lambda: flat.search(q, k)])
        exact[nq] = (t_exact, flat.search(q, k)[1])
        print(f"exact search, {nq} queries: {t_exact * 1e3:.3f} ms", flush=True)
    for nlist in ints(a.nlist):
        torch.cuda.synchronize()
        t = time.perf_counter()
        index = ivf.IVFFlatIndex(docs, nlist)
        torch.cuda.synchronize()
        sizes = index.offsets[1:] - index.offsets[:-1]
        print(f"IVF{nlist},Flat build (k-means {ivf.NITER} it. on {min(a.docs, 256 * nlist)} rows + assign + list-major copy): "
              f"{time.perf_counter() - t:.2f} s; lists min {int(sizes.min())} / max {int(sizes.max())} rows", flush=True)
        for nprobe in ints(a.nprobe):
            for nq in nqs:
                q = q_all[:nq].contiguous()
                if not index.scan_wanted(nq, k, nprobe):
                    print(f"IVF{nlist} nprobe {nprobe} nq {nq}: outside the scan's envelope", flush=True)
                    continue
                s1, i1 = index.search_scan(q, k, nprobe)
                s0, i0 = index.search_lists(q, k, nprobe)
                same = bool(torch.equal(i0, i1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32)))
                t_scan, t_lists = timed([lambda: index.search_scan(q, k, nprobe), lambda: index.search_lists(q, k, nprobe)])
                row = {"nlist": nlist, "nprobe": nprobe, "nq": nq, "k": k, "scan_ms": round(t_scan * 1e3, 4), "lists_ms": round(t_lists * 1e3, 4),
                       "exact_ms": round(exact[nq][0] * 1e3, 4), "same_bits": same, "recall": recall(i1, exact[nq][1])}
                # the rows the batch has to read at least once: those of the distinct lists it probes
                probe = dense.ivf_scan_topk(q, index.centroids, index.centroid_offsets, None, nlist,
                                            torch.zeros((nq, 1), dtype=torch.int32, device=dev), nprobe)[1]
                lists = torch.unique(probe).cpu()
                row["probed_bytes"] = int(sizes[lists].sum()) * docs.shape[1] * 4
                row["hbm_fraction"] = round(row["probed_bytes"] / t_scan / HBM_PEAK, 4)
                if nq <= ivf.GRAPH_MAX_QUERIES:
                    g = index.search_graph(nq, k, nprobe)
                    (t_graph,) = timed([lambda: g.run(q)])
                    gs, gi = g.run(q)
                    row["graph_ms"] = round(t_graph * 1e3, 4)
                    row["same_bits"] = bool(same and torch.equal(gi, i1) and torch.equal(gs.view(torch.int32), s1.view(torch.int32)))
                    del g
                rows.append(row)
                print(json.dumps(row), flush=True)
                if a.out:                                                   # after every row: a long table survives a short limit
                    with open(a.out, "w") as f:
                        json.dump({"docs": a.docs, "dim": docs.shape[1], "hbm_peak_bytes_per_s": HBM_PEAK,
                                   "note": "hbm_fraction = bytes of the distinct probed lists / time of the whole search "
                                           "(coarse + scan + select) / peak", "rows": rows}, f, indent=1)
        del index
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
