"""IVF-PQ (faiss_search.py --param IVF<n>,PQ<m>) against IVF-Flat at C2 size on the synthetic corpus, in one process: per nlist the
build time of both indexes and the bytes of codes, then per (nprobe, query count) the ADC search (IVFPQIndex.search_scan: coarse
call + mevi_ivfpq_scan_topk_f32) against the IVF-Flat device scan (IVFFlatIndex.search_scan) at the same nlist and nprobe --
median of 3 timed windows after a warm-up, the two taking turns (tools/bench_ivf.py: timed) --, recall of both against the exact
search, the replayed graph's latency for up to 32 queries, and the rate of table gathers against the LDS's conflict-free
ds_read_b32 rate.
  python tools/bench_ivfpq.py [nlist,...] [nprobe,...] [--m 64] [--nbits 8] [--nq 1,8,32,6980] [--k 1000] [--docs N] [--out table.json]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from bench_ivf import HBM_PEAK, ints, recall, timed  # noqa: E402
from mevi_amd import dense, ivf, ivfpq  # noqa: E402

LDS_GATHER_PEAK = 256 * 32 * 2.4e9      # ds_read_b32 lanes/s without conflicts: 128 B/clk/CU on 256 CUs at 2.4 GHz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("nlist", nargs="?", default="100,4096")
    ap.add_argument("nprobe", nargs="?", default="1,4,16")
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--nbits", type=int, default=8)
    ap.add_argument("--nq", default=f"1,8,32,{bench.N_QUERIES}")
    ap.add_argument("--k", type=int, default=bench.TOPK)
    ap.add_argument("--docs", type=int, default=bench.N_DOCS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    docs = bench.gen_shard(0, a.docs, dev, a.docs)
    dim = docs.shape[1]
    nqs = ints(a.nq)
    q_all = bench.gen_queries(max(nqs), dev, a.docs)
    k, m = a.k, a.m
    exact_ids = dense.DenseIndex(docs).search(q_all, k)[1]       # per query: the same lists whatever the batch
    torch.cuda.empty_cache()
    rows, builds = [], []

    def save():
        if a.out:                                                # after every row: a long table survives a short limit
            with open(a.out, "w") as f:
                json.dump({"docs": a.docs, "dim": dim, "m": m, "nbits": a.nbits, "k": k, "hbm_peak_bytes_per_s": HBM_PEAK,
                           "lds_gather_peak_per_s": LDS_GATHER_PEAK,
                           "note": "pq_ms / flat_ms = the whole search (coarse + scan + select) of IVFPQIndex.search_scan / "
                                   "IVFFlatIndex.search_scan, median of 3 windows after a warm-up, taking turns; scanned_rows = rows of "
                                   "the probed lists summed over the queries; lds_gather_fraction = scanned_rows * m / pq_ms / the "
                                   "conflict-free ds_read_b32 rate; pq_hbm_fraction = scanned_rows * m bytes / pq_ms / peak",
                           "builds": builds, "rows": rows}, f, indent=1)

    for nlist in ints(a.nlist):
        torch.cuda.synchronize()
        t = time.perf_counter()
        flat = ivf.IVFFlatIndex(docs, nlist)
        torch.cuda.synchronize()
        t_flat = time.perf_counter() - t
        t = time.perf_counter()
        cent = ivf.train_centroids(docs, nlist)                  # the same seed: the centroids of `flat`, timed as part of this build
        torch.cuda.synchronize()
        t_coarse = time.perf_counter() - t
        t = time.perf_counter()
        book = ivfpq.train_codebook(docs, ivf.assign(docs, cent), cent, m, a.nbits)
        torch.cuda.synchronize()
        t_book = time.perf_counter() - t
        t = time.perf_counter()
        pq = ivfpq.IVFPQIndex(docs, nlist, m, a.nbits, centroids=cent, codebook=book)
        torch.cuda.synchronize()
        t_add = time.perf_counter() - t
        sizes = pq.offsets[1:] - pq.offsets[:-1]
        b = {"nlist": nlist, "flat_build_s": round(t_flat, 2), "pq_train_coarse_s": round(t_coarse, 2), "pq_train_codebook_s": round(t_book, 2),
             "pq_add_s": round(t_add, 2), "code_bytes": pq.codes.numel(), "flat_bytes": flat.docs.numel() * 4,
             "same_lists": bool(torch.equal(pq.ids, flat.ids)), "list_rows_min": int(sizes.min()), "list_rows_max": int(sizes.max())}
        builds.append(b)
        print(json.dumps(b), flush=True)
        save()
        for nprobe in ints(a.nprobe):
            for nq in nqs:
                q = q_all[:nq].contiguous()
                row = {"nlist": nlist, "nprobe": nprobe, "nq": nq, "k": k}
                fns = [lambda: pq.search_scan(q, k, nprobe)]
                flat_scan = flat.scan_wanted(nq, k, nprobe) or dense.ivf_scan_query_tile(nq, nprobe, k, dim, nlist, flat.max_list_len) > 0
                if flat_scan:
                    fns.append(lambda: flat.search_scan(q, k, nprobe))
                times = timed(fns)
                row["pq_ms"] = round(times[0] * 1e3, 4)
                i_pq = pq.search_scan(q, k, nprobe)[1]
                row["pq_recall"] = recall(i_pq, exact_ids[:nq])
                if flat_scan:
                    row["flat_ms"] = round(times[1] * 1e3, 4)
                    row["flat_recall"] = recall(flat.search_scan(q, k, nprobe)[1], exact_ids[:nq])
                    row["pq_faster"] = bool(times[0] < times[1])
                    row["speedup"] = round(times[1] / times[0], 2)
                if not flat.scan_wanted(nq, k, nprobe):          # the regime where IVFFlatIndex.search takes the loop over lists
                    (t_lists,) = timed([lambda: flat.search_lists(q, k, nprobe)])
                    row["flat_lists_ms"] = round(t_lists * 1e3, 4)
                probe = dense.ivf_scan_topk(q, pq.centroids, pq.centroid_offsets, None, nlist,
                                            torch.zeros((nq, 1), dtype=torch.int32, device=dev), nprobe)[1].cpu()
                scanned = int(sizes[probe].sum())
                row["scanned_rows"] = scanned
                row["lds_gather_fraction"] = round(scanned * m / times[0] / LDS_GATHER_PEAK, 4)
                row["pq_hbm_fraction"] = round(scanned * m / times[0] / HBM_PEAK, 5)
                row["query_tiles"] = -(-nq // dense.ivfpq_scan_query_tile(nq, nprobe, k, dim, m, 1 << a.nbits, nlist, pq.max_list_len))
                if nq <= ivfpq.GRAPH_MAX_QUERIES:
                    g = pq.search_graph(nq, k, nprobe)
                    (t_graph,) = timed([lambda: g.run(q)])
                    row["pq_graph_ms"] = round(t_graph * 1e3, 4)
                    row["graph_same_bits"] = bool(torch.equal(g.run(q)[1], i_pq))
                    del g
                rows.append(row)
                print(json.dumps(row), flush=True)
                save()
        del flat, pq
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
