"""Variable-depth NCI beam search at the C3 shape: 6980 queries, 10 beams, K = 30, ids of at most 6 codes, a synthetic
k30_c30-style tree (hierarchical k-means ids: lengths 4 .. 6) over 8.8 M ids, t5-base-shaped synthetic weights.

  timeout -k 10 500 python tools/bench_varbeam.py --out profiles/varbeam_c3.json &&
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -o varbeam -- python tools/bench_varbeam.py --ids 2000000 --queries 2048 &&
  timeout 60 python tools/bench_varbeam.py --share-from DIR/<host>/varbeam_kernel_stats.csv     (no GPU: reads the stats file)

Options: [--ids N] [--queries N] [--batch N] [--out file.json].  Every GPU step runs under its own time limit, the steps
chained with && so that nothing starts after one of them failed.

Reports the host tree build (seconds), the variable-depth search (queries/s) and, measured in the same process on the same
model, the fixed-depth search over the shared-sons tree (M = 6, K = 30) it is to be compared with; --share-from adds
the share of kernel time spent in beam_step_var / beam_finalize_var."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

M, K, R = 6, 30, 10


def synthetic_ids(n, rng):
    """[n, 6] codes + lengths: 20 % of the ids end after 4 codes, 60 % after 5, 20 % after 6."""
    lengths = rng.choice([4, 5, 6], size=n, p=[0.2, 0.6, 0.2])
    return rng.integers(0, K, size=(n, M)), lengths


def kernel_share(path):
    total, var = 0.0, {}
    with open(path) as f:
        for row in csv.DictReader(f):
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
            total += ns
            if "beam_step_var" in row["Name"] or "beam_finalize_var" in row["Name"]:
                var[row["Name"].split("(")[0][-40:]] = ns
    return {"kernel_ns_total": total, "var_kernels_ns": var, "beam_step_var_share": sum(var.values()) / total if total else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, default=8841823)
    ap.add_argument("--queries", type=int, default=6980)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--out", default=None)
    ap.add_argument("--share-from", default=None)
    a = ap.parse_args()
    if a.share_from:
        print(json.dumps(kernel_share(a.share_from)))
        return
    import torch

    import synth
    from mevi_amd import nci

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    codes, lengths = synthetic_ids(a.ids, rng)
    t = time.perf_counter()
    tree = nci.RaggedPrefixTree(codes, K, dev, lengths=lengths, levels=M + 1)
    build_s = time.perf_counter() - t
    model = synth.build(dev, M, K, a.batch)[0]
    ids, mask = synth.query_ids(a.queries, dev, rng)

    def run(**kw):
        return [model.generate(ids[b:b + a.batch], mask[b:b + a.batch], num_beams=R, **kw)[0] for b in range(0, a.queries, a.batch)]

    out = {"shape": {"queries": a.queries, "batch": a.batch, "beams": R, "K": K, "max_codes": M, "ids": a.ids,
                     "distinct_ids": tree.n_paths, "nodes_per_level": tree.n_nodes}, "tree_build_s": round(build_s, 2)}
    for name, kw in (("fixed_depth", {}), ("variable_depth", {"decode_tree": tree})):
        run(**kw)                                   # warm-up: prefix tables, kernel caches
        torch.cuda.synchronize()
        best = None
        for _ in range(3):
            t = time.perf_counter()
            run(**kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        out[name + "_queries_per_s"] = round(a.queries / best, 1)
        out[name + "_ms"] = round(best * 1e3, 2)
    out["variable_over_fixed_time"] = round(out["variable_depth_ms"] / out["fixed_depth_ms"], 4)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
