"""Scalar-quantised indexes (faiss_search.py --param SQ8 / SQ4 / IVF<n>,SQ8 / IVF<n>,SQ4) at C2 size on the synthetic corpus, in
one process: per index the build times (IVF-Flat: the whole build; SQ: coarse k-means, range training, add = assign + lists +
encode) and the bytes of codes, then per (nprobe, query count) the SQ search (SQIndex.search: coarse call +
mevi_sq_scan_topk_f32) beside the IVF-Flat device scan of the SAME lists and probes (IVFFlatIndex.search_scan; for a flat index
mevi_ivf_scan_topk_f32 over the corpus as one list) and the exact search (DenseIndex.search) -- median of 3 timed windows after a
warm-up, the paths taking turns (tools/bench_ivf.py: timed) --, recall of both against the exact search, and the rate of the
scan's matrix work against the f32 MFMA peak.
  python tools/bench_sq.py [spec;...] [--nq 1,32,6980] [--k 1000] [--docs N] [--out profiles/sq_c2.json]
A spec is a factory string, then ':' and the nprobes for an IVF: 'IVF100,SQ8:1,16;IVF4096,SQ8:1,16;IVF100,SQ4:1,16;SQ8'."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from bench_ivf import HBM_PEAK, MFMA_F32_PEAK, ints, recall, timed  # noqa: E402
from mevi_amd import dense, ivf, sq  # noqa: E402

DEFAULT = "IVF100,SQ8:1,16;IVF4096,SQ8:1,16;IVF100,SQ4:1,16;SQ8"


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("specs", nargs="?", default=DEFAULT)
    ap.add_argument("--nq", default=f"1,32,{bench.N_QUERIES}")
    ap.add_argument("--k", type=int, default=bench.TOPK)
    ap.add_argument("--docs", type=int, default=bench.N_DOCS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    docs = bench.gen_shard(0, a.docs, dev, a.docs)
    nd, dim = docs.shape
    nqs = ints(a.nq)
    q_all = bench.gen_queries(max(nqs), dev, a.docs)
    k = a.k
    exact_index = dense.DenseIndex(docs).prepare_small()
    exact_ids = exact_index.search(q_all, k)[1]                  # per query: the same lists whatever the batch
    exact_ms = {}
    for nq in nqs:
        q = q_all[:nq].contiguous()
        exact_ms[nq] = round(timed([lambda: exact_index.search(q, k)])[0] * 1e3, 4)
        print(f"exact search, {nq} queries: {exact_ms[nq]} ms", flush=True)
    rows, builds = [], []

    def save():
        if a.out:                                                # after every row: a long table survives a short limit
            with open(a.out, "w") as f:
                json.dump({"docs": nd, "dim": dim, "k": k, "hbm_peak_bytes_per_s": HBM_PEAK, "mfma_f32_peak_flop_per_s": MFMA_F32_PEAK,
                           "note": "sq_ms / flat_ms = the whole search (coarse + grouping + scan + select) of SQIndex.search / the IVF-Flat "
                                   "device scan of the same lists and probes, exact_ms = DenseIndex.search; median of 3 windows after a "
                                   "warm-up, the paths taking turns; scanned_rows = rows of the probed lists summed over the queries; "
                                   "sq_mfma_fraction = 2 * scanned_rows * dim / sq_ms / the f32 MFMA peak (padding of pair tiles not "
                                   "counted); sq_code_bytes_per_s = bytes of the DISTINCT probed lists' codes / sq_ms",
                           "exact_ms": exact_ms, "builds": builds, "rows": rows}, f, indent=1)

    for spec in a.specs.split(";"):
        name, _, probes = spec.partition(":")
        nlist, bits = sq.parse_factory(name)
        b = {"index": name.strip(), "flat_bytes": nd * dim * 4}
        if nlist is None:
            flat, cent = None, None
            one_list = torch.tensor([0, nd], dtype=torch.int64, device=dev)
            b["sq_train_coarse_s"] = 0.0
        else:
            b["flat_build_s"], flat = clock(lambda: ivf.IVFFlatIndex(docs, nlist))
            b["sq_train_coarse_s"], cent = clock(lambda: ivf.train_centroids(docs, nlist))     # the same seed: the centroids of `flat`
        t_range, rng = clock(lambda: sq.train_range(docs, ivf.assign(docs, cent) if cent is not None else None, cent))
        t_add, index = clock(lambda: sq.SQIndex(docs, nlist, bits, centroids=cent, vmin=rng[0], vdiff=rng[1]))
        sizes = index.offsets[1:] - index.offsets[:-1]
        b.update({"sq_train_range_s": round(t_range, 3), "sq_add_s": round(t_add, 3), "code_bytes": index.codes.numel(),
                  "same_lists": bool(flat is None or torch.equal(index.ids, flat.ids)), "list_rows_min": int(sizes.min()),
                  "list_rows_max": int(sizes.max())})
        b = {key: (round(v, 3) if isinstance(v, float) else v) for key, v in b.items()}
        builds.append(b)
        print(json.dumps(b), flush=True)
        save()
        for nprobe in (ints(probes) if probes else [1]):
            for nq in nqs:
                q = q_all[:nq].contiguous()
                zero = torch.zeros((nq, 1), dtype=torch.int32, device=dev)
                row = {"index": name.strip(), "nprobe": nprobe, "nq": nq, "k": k, "exact_ms": exact_ms[nq]}
                if flat is None:
                    def flat_fn():
                        return dense.ivf_scan_topk(q, docs, one_list, None, nd, zero, k)
                    scanned, distinct = nq * nd, nd
                else:
                    def flat_fn():
                        return flat.search_scan(q, k, nprobe)
                    probe = dense.ivf_scan_topk(q, index.centroids, index.centroid_offsets, None, nlist, zero, nprobe)[1].cpu()
                    scanned, distinct = int(sizes[probe].sum()), int(sizes[torch.unique(probe)].sum())
                t_sq, t_flat = timed([lambda: index.search(q, k, nprobe), flat_fn])
                row.update({"sq_ms": round(t_sq * 1e3, 4), "flat_ms": round(t_flat * 1e3, 4), "flat_over_sq": round(t_flat / t_sq, 2),
                            "sq_over_exact": round(t_sq * 1e3 / exact_ms[nq], 2),
                            "sq_recall": recall(index.search(q, k, nprobe)[1], exact_ids[:nq]),
                            "flat_recall": recall(flat_fn()[1], exact_ids[:nq]), "scanned_rows": scanned,
                            "sq_mfma_fraction": round(2.0 * scanned * dim / t_sq / MFMA_F32_PEAK, 4),
                            "sq_code_bytes_per_s": round(distinct * dim * bits / 8 / t_sq, 0),
                            "query_tiles": -(-nq // dense.sq_scan_query_tile(nq, nprobe, k, dim, bits, index.n_lists, index.max_list_len))})
                rows.append(row)
                print(json.dumps(row), flush=True)
                save()
        del flat, index
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
