"""4-bit fast-scan PQ (faiss_search.py --param IVF<n>,PQ<m>x4fs) at C2 size on the synthetic corpus, in one process.  Per nlist four
indexes over the same centroids and lists take turns:
  fs   PQ<m>x4fs: pqfs.PQFSIndex, packed rows of m / 2 bytes, mevi_pqfs_scan_topk_f32;
  a    PQ<m>x4 on the SAME codebook and codes through the byte scan mevi_ivfpq_scan_topk_f32: identical results, so the ratio
       a_ms / fs_ms isolates the kernel;
  b    PQ<m/2>x8: the same bytes per row as fs -- the classical fast-scan trade of time and recall;
  c    PQ<m>x8: today's default.
Per (nprobe, query count): ms of the whole search (coarse + scan + select; median of 3 timed windows after a warm-up,
tools/bench_ivf.py: timed), the ratios to fs, recall@1/10/1000 against the exact search, the scanned rows and the rate of table
gathers against the LDS's conflict-free ds_read_b32 rate; per nlist the code bytes and build times.  nlist 0 is the flat index
PQ<m>x4fs against the exact search.
  python tools/bench_pqfs.py [nlist,...] [nprobe,...] [--m 64] [--nq 1,8,32,6980] [--k 1000] [--docs N] [--out table.json]
  python tools/bench_pqfs.py 100 4 --nq 6980 --once fs|a    one untimed search of one index after a warm-up: the run to put under
                                                             a counter collection of its own (kernels: pqfs_scan_kernel /
                                                             ivfpq_scan_kernel)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from bench_ivf import ints, recall, timed  # noqa: E402
from mevi_amd import dense, ivf, ivfpq, pqfs  # noqa: E402

LDS_GATHER_PEAK = 256 * 32 * 2.4e9      # ds_read_b32 lanes/s without conflicts: 128 B/clk/CU on 256 CUs at 2.4 GHz


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, round(time.perf_counter() - t, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("nlist", nargs="?", default="100,4096,0")
    ap.add_argument("nprobe", nargs="?", default="1,4,16")
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--nq", default=f"1,8,32,{bench.N_QUERIES}")
    ap.add_argument("--k", type=int, default=bench.TOPK)
    ap.add_argument("--docs", type=int, default=bench.N_DOCS)
    ap.add_argument("--once", choices=("fs", "a"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    docs = bench.gen_shard(0, a.docs, dev, a.docs)
    dim = docs.shape[1]
    nqs = ints(a.nq)
    q_all = bench.gen_queries(max(nqs), dev, a.docs)
    k, m = a.k, a.m
    rows, builds = [], []

    def save():
        if a.out:                                                # after every row: a long table survives a short limit
            with open(a.out, "w") as f:
                json.dump({"docs": a.docs, "dim": dim, "m": m, "k": k, "lds_gather_peak_per_s": LDS_GATHER_PEAK,
                           "note": "fs = PQ<m>x4fs (packed rows, mevi_pqfs_scan_topk_f32); a = PQ<m>x4 on the same codebook and codes "
                                   "through mevi_ivfpq_scan_topk_f32 (identical results); b = PQ<m/2>x8 (the same bytes per row as fs); "
                                   "c = PQ<m>x8.  *_ms = the whole search (coarse + scan + select), median of 3 windows after a warm-up, "
                                   "the indexes taking turns; x_over_fs = x_ms / fs_ms (above 1: fs is faster); scanned_rows = rows of "
                                   "the probed lists summed over the queries; fs_lds_gather_fraction = scanned_rows * m / fs_ms / the "
                                   "conflict-free ds_read_b32 rate; nlist 0 = the flat index, exact_ms = DenseIndex.search",
                           "builds": builds, "rows": rows}, f, indent=1)

    if a.once is None:
        exact = dense.DenseIndex(docs)
        exact_ids = exact.search(q_all, k)[1]                    # per query: the same lists whatever the batch
        if 0 not in ints(a.nlist):
            del exact
        torch.cuda.empty_cache()
    for nlist_arg in ints(a.nlist):
        nlist = nlist_arg or None
        cent, t_coarse = clock(lambda: ivf.train_centroids(docs, nlist)) if nlist else (None, 0.0)
        list_of = ivf.assign(docs, cent) if nlist else None
        book4, t_book4 = clock(lambda: ivfpq.train_codebook(docs, list_of, cent, m, 4))
        fs, t_fs = clock(lambda: pqfs.PQFSIndex(docs, nlist, m, centroids=cent, codebook=book4))
        if a.once == "fs":
            q = q_all[:nqs[0]].contiguous()
            fs.search_scan(q, k, fs.clamp_nprobe(ints(a.nprobe)[0]))
            torch.cuda.synchronize()
            fs.search_scan(q, k, fs.clamp_nprobe(ints(a.nprobe)[0]))
            torch.cuda.synchronize()
            return
        pa, t_a = clock(lambda: ivfpq.IVFPQIndex(docs, nlist, m, 4, centroids=cent, codebook=book4))
        if a.once == "a":
            q = q_all[:nqs[0]].contiguous()
            pa.search_scan(q, k, pa.clamp_nprobe(ints(a.nprobe)[0]))
            torch.cuda.synchronize()
            pa.search_scan(q, k, pa.clamp_nprobe(ints(a.nprobe)[0]))
            torch.cuda.synchronize()
            return
        same_codes = bool(torch.equal(fs.codes, dense.pq4_pack(pa.codes)))
        others = {}
        b = {"nlist": nlist_arg, "train_coarse_s": t_coarse, "fs_train_codebook_s": t_book4, "fs_add_s": t_fs, "a_add_s": t_a,
             "fs_code_bytes": fs.codes.numel(), "a_code_bytes": pa.codes.numel(), "fs_codes_are_a_codes_packed": same_codes}
        for name, (mm, bits) in (("b", (m // 2, 8)), ("c", (m, 8))):
            if nlist is None:
                break
            book, t_book = clock(lambda: ivfpq.train_codebook(docs, list_of, cent, mm, bits))
            others[name], t_add = clock(lambda: ivfpq.IVFPQIndex(docs, nlist, mm, bits, centroids=cent, codebook=book))
            b.update({f"{name}_train_codebook_s": t_book, f"{name}_add_s": t_add, f"{name}_code_bytes": others[name].codes.numel()})
        sizes = fs.offsets[1:] - fs.offsets[:-1]
        b.update({"list_rows_min": int(sizes.min()), "list_rows_max": int(sizes.max())})
        builds.append(b)
        print(json.dumps(b), flush=True)
        save()
        for nprobe in (ints(a.nprobe) if nlist else [1]):
            for nq in nqs:
                q = q_all[:nq].contiguous()
                row = {"nlist": nlist_arg, "nprobe": nprobe, "nq": nq, "k": k}
                names = ["fs", "a"] + list(others)
                index = {"fs": fs, "a": pa, **others}
                fns = [lambda n=n: index[n].search_scan(q, k, nprobe) for n in names]
                if nlist is None:
                    names.append("exact")
                    fns.append(lambda: exact.search(q, k))
                times = dict(zip(names, timed(fns)))
                got = {n: index[n].search_scan(q, k, nprobe) for n in names if n != "exact"}
                row["a_same_bits"] = bool(torch.equal(got["fs"][1], got["a"][1]) and
                                          torch.equal(got["fs"][0].view(torch.int32), got["a"][0].view(torch.int32)))
                for n in names:
                    row[f"{n}_ms"] = round(times[n] * 1e3, 4)
                    if n not in ("fs", "exact"):
                        row[f"{n}_over_fs"] = round(times[n] / times["fs"], 2)
                    if n in ("fs", "b", "c"):
                        row[f"{n}_recall"] = recall(got[n][1], exact_ids[:nq])
                if nlist is None:
                    row["exact_over_fs"] = round(times["exact"] / times["fs"], 3)
                    scanned = nq * docs.shape[0]
                else:
                    probe = dense.ivf_scan_topk(q, fs.centroids, fs.centroid_offsets, None, nlist,
                                                torch.zeros((nq, 1), dtype=torch.int32, device=dev), nprobe)[1].cpu()
                    scanned = int(sizes[probe].sum())
                row["scanned_rows"] = scanned
                row["fs_lds_gather_fraction"] = round(scanned * m / times["fs"] / LDS_GATHER_PEAK, 4)
                row["a_lds_gather_fraction"] = round(scanned * m / times["a"] / LDS_GATHER_PEAK, 4)
                row["query_tiles"] = -(-nq // dense.pqfs_scan_query_tile(nq, nprobe, k, dim, m, fs.n_lists, fs.max_list_len))
                rows.append(row)
                print(json.dumps(row), flush=True)
                save()
        del fs, pa, others
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
