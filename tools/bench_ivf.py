"""IVF-Flat (faiss_search.py --param IVF<n>,Flat) at C2 size on the synthetic corpus: build time, then per regime the device
scan (IVFFlatIndex.search_scan) against the host loop over lists (search_lists) in one process -- same bits checked, median of
3 timed windows after a warm-up, the two paths alternating -- with recall vs exact, the exact search's own time
(DenseIndex.search), the replayed graph's latency for up to 32 queries, and the rate at which the scan call reads the rows of
the probed lists.
  python tools/bench_ivf.py [nlist,...] [nprobe,...] [--nq 1,8,32,6980] [--k 1000] [--docs N] [--out table.json]
--build times the build instead (index.train + index.add): per nlist (default 100,4096) the four phases -- k-means, labelling
the whole corpus, list layout, list-major row copy -- through the kernels of csrc/ivf_build.hip and through the torch
composition they replaced (MEVI_IVF_BUILD=host), in one process, alternating, 3 windows each after a warm-up, device
synchronisation around the host clock; labels, offsets, ids and centroids of the two paths are checked to be equal.
  python tools/bench_ivf.py --build [nlist,...] [--docs N] [--out profiles/ivf_build_c2.json]"""
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


MFMA_F32_PEAK = 157.3e12    # FLOP/s of v_mfma_f32_32x32x2_f32 on 256 CUs at 2.4 GHz


def windows(fns, n=3):
    """[(median, min, max) seconds, last result] per function: one warm-up call each, then n single-call windows, taking turns."""
    out = [fn() for fn in fns]
    laps = [[] for _ in fns]
    for _ in range(n):
        for j, fn in enumerate(fns):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out[j] = fn()
            torch.cuda.synchronize()
            laps[j].append(time.perf_counter() - t)
    return [((statistics.median(x), min(x), max(x)), o) for x, o in zip(laps, out)]


def on_path(path, fn):
    def run():
        old = os.environ.get("MEVI_IVF_BUILD")
        os.environ["MEVI_IVF_BUILD"] = path
        try:
            return fn()
        finally:
            if old is None:
                del os.environ["MEVI_IVF_BUILD"]
            else:
                os.environ["MEVI_IVF_BUILD"] = old
    return run


def build_table(a):
    """The four phases of IVFFlatIndex.__init__ per nlist and path."""
    from mevi_amd import ops

    dev = torch.device("cuda:0")
    docs = bench.gen_shard(0, a.docs, dev, a.docs)
    n, dim = docs.shape
    rows = []
    for nlist in ints(a.nlist):
        ns = min(n, ivf.MAX_POINTS_PER_CENTROID * nlist)
        pad = -(-nlist // dense.IVF_ASSIGN_COLS) * dense.IVF_ASSIGN_COLS
        (t_dev, cent), (t_host, cent_h) = windows([on_path("device", lambda: ivf.train_centroids(docs, nlist)),
                                                   on_path("host", lambda: ivf.train_centroids(docs, nlist))])
        same = {"centroids": bool(torch.equal(cent.view(torch.int32), cent_h.view(torch.int32)))}
        phases = {"train": (t_dev, t_host, ivf.NITER * 2.0 * ns * pad * dim, ivf.NITER * 2.0 * ns * dim * 4)}
        del cent_h
        (t_dev, lab), (t_host, lab_h) = windows([on_path("device", lambda: ivf.assign(docs, cent)), on_path("host", lambda: ivf.assign(docs, cent))])
        same["labels"] = bool(torch.equal(lab, lab_h))
        phases["assign"] = (t_dev, t_host, 2.0 * n * pad * dim, n * dim * 4.0)
        del lab_h
        (t_dev, lay), (t_host, lay_h) = windows([on_path("device", lambda: ivf.build_lists(lab, nlist)), on_path("host", lambda: ivf.build_lists(lab, nlist))])
        same["offsets"] = bool(torch.equal(lay[0], lay_h[0]) and lay[3] == lay_h[3])
        same["ids"] = bool(torch.equal(lay[2], lay_h[2]))
        phases["layout"] = (t_dev, t_host, 0.0, n * (4.0 + 8.0))
        order = lay[2]
        del lay_h
        # the row copy: the kernel path is mevi_gather_rows_f32, the host path the advanced indexing the index uses
        (t_dev, moved), (t_host, moved_h) = windows([lambda: ops.gather_rows(docs, order), lambda: docs[order].contiguous()])
        same["rows"] = bool(torch.equal(moved.view(torch.int32), moved_h.view(torch.int32)))
        phases["copy"] = (t_dev, t_host, 0.0, 2.0 * n * dim * 4)
        del moved, moved_h
        for name, (td, th, flop, nbytes) in phases.items():
            row = {"nlist": nlist, "phase": name, "flop": flop, "bytes": nbytes}
            for path, t in (("device", td), ("host", th)):
                row[path] = {"median_s": round(t[0], 6), "min_s": round(t[1], 6), "max_s": round(t[2], 6)}
            row["device_tflops"] = round(flop / td[0] / 1e12, 2)
            row["device_mfma_fraction"] = round(flop / td[0] / MFMA_F32_PEAK, 4)
            row["device_hbm_fraction"] = round(nbytes / td[0] / HBM_PEAK, 4)
            # the rule of DESIGN 4.1g: the kernel path stays unless its median exceeds the host's by more than the host's own spread
            row["device_kept"] = bool(td[0] <= th[0] + (th[2] - th[1]))
            rows.append(row)
            print(json.dumps(row), flush=True)
        print(json.dumps({"nlist": nlist, "equal": same}), flush=True)
        rows.append({"nlist": nlist, "equal": same})
        if a.out:
            with open(a.out, "w") as f:
                json.dump({"docs": n, "dim": dim, "niter": ivf.NITER, "hbm_peak_bytes_per_s": HBM_PEAK, "mfma_f32_peak_flop_per_s": MFMA_F32_PEAK,
                           "note": "flop = 2 * rows * nlist padded to 128 * dim (x 25 iterations for train), bytes = the rows read once "
                                   "(labels in and ids out for layout, rows in and out for copy); copy: device = mevi_gather_rows_f32, "
                                   "host = docs[order]; 3 single-call windows per path after a warm-up, the paths alternating",
                           "rows": rows}, f, indent=1)
        del cent, lab, lay, order
        torch.cuda.empty_cache()


def recall(ids, exact_ids):
    rec = {}
    n = ids.shape[0]
    for a in range(0, n, 256):
        for c, v in ivf.recall_report(ids[a:a + 256], exact_ids[a:a + 256]).items():
            rec[c] = rec.get(c, 0.0) + v * min(256, n - a) / n
    return {str(c): round(v, 4) for c, v in rec.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("nlist", nargs="?", default=None)
    ap.add_argument("nprobe", nargs="?", default="1,4,16")
    ap.add_argument("--nq", default=f"1,8,32,{bench.N_QUERIES}")
    ap.add_argument("--k", type=int, default=bench.TOPK)
    ap.add_argument("--docs", type=int, default=bench.N_DOCS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.nlist is None:
        a.nlist = "100,4096" if a.build else "100"
    if a.build:
        return build_table(a)
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
