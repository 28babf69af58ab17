"""Variable-depth NCI beam search at the C3 shape: 6980 queries, 10 beams, K = 30, ids of at most 6 codes, a synthetic
k30_c30-style tree (hierarchical k-means ids: lengths 4 .. 6) over 8.8 M ids, t5-base-shaped synthetic weights.

  timeout -k 10 500 python tools/bench_varbeam.py --out profiles/varbeam_c3.json &&
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -o varbeam -- python tools/bench_varbeam.py --ids 2000000 --queries 2048 &&
  timeout 60 python tools/bench_varbeam.py --share-from DIR/<host>/varbeam_kernel_stats.csv     (no GPU: reads the stats file)

  timeout -k 10 500 python tools/bench_varbeam.py --beams 100 --depth 8 --ids 2000000 --queries 1024 --batch 128 --variable-only   (pure-NCI shape)
  timeout -k 10 120 python tools/bench_varbeam.py --steps-only --depth 8     (the beam-step kernel alone, at --step-beams 1,4,10,32,64,100)

Options: [--ids N] [--queries N] [--batch N] [--beams R] [--depth M] [--steps-only] [--step-beams R,R,...] [--variable-only]
[--out file.json].  --depth M = ids of at most M codes (lengths M - 2 .. M), M + 1 decoder positions (more than 8: the
9 .. 16-key cached attention).  Every GPU step runs under its own time limit, the steps chained with && so that nothing
starts after one of them failed.

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

K = 30


def synthetic_ids(n, rng, M=6):
    """[n, M] codes + lengths: 20 % of the ids end after M - 2 codes, 60 % after M - 1, 20 % after M."""
    lengths = rng.choice([M - 2, M - 1, M], size=n, p=[0.2, 0.6, 0.2])
    return rng.integers(0, K, size=(n, M)), lengths


def step_times(dev, M, nq, rng, beam_counts, reps=20):
    """Per-launch time of mevi_beam_step_var_f32 alone at (nq queries, K = 30, T = M + 2, step p = 2 of a three-level tree,
    random logits) for every beam count of `beam_counts`."""
    import torch

    from mevi_amd import hip, nci

    T, p = M + 2, 2
    codes, lengths = synthetic_ids(200000, rng, M)
    tree = nci.RaggedPrefixTree(codes, K, dev, lengths=lengths, levels=M + 1)
    n_nodes = tree.base[p].numel()
    out, fn = {}, "mevi_beam_step_var_f32"
    for beams in beam_counts:
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)                   # noqa: E731
        logits = torch.randn((nq * beams, K + 1), device=dev) * 2
        scores = -torch.rand((nq, beams), device=dev).cumsum(1)
        node = torch.randint(0, n_nodes, (nq, beams), device=dev, dtype=torch.int32)
        prefix, anc = i32(nq, beams, T), i32(nq * beams, p)
        len_pow = torch.tensor([float(l) ** 0.8 for l in range(T + 1)], dtype=torch.float64).to(dev)
        pool = (torch.zeros((nq, beams), dtype=torch.float64, device=dev), i32(nq, beams), i32(nq, beams), i32(nq, beams, T), i32(nq, 4))
        res = (torch.empty((nq, beams), device=dev), i32(nq, beams), i32(nq, beams), i32(nq, beams), i32(nq, beams, T), i32(nq * beams, p + 1))
        call = lambda: hip.check(getattr(hip.lib(), fn)(                                     # noqa: E731
            hip.ptr(logits), hip.ptr(scores), hip.ptr(node), hip.ptr(prefix), hip.ptr(anc), nq, beams, K, p, T, hip.ptr(tree.mask[p]),
            hip.ptr(tree.base[p]), hip.ptr(tree.ends[p]), n_nodes, hip.ptr(len_pow), *(hip.ptr(t) for t in pool),
            *(hip.ptr(t) for t in res), hip.stream_ptr()), fn)
        call()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            for t in pool:
                t.zero_()
            call()
        ev[1].record()
        torch.cuda.synchronize()
        with_reset = ev[0].elapsed_time(ev[1])
        ev[0].record()
        for _ in range(reps):
            for t in pool:
                t.zero_()
        ev[1].record()
        torch.cuda.synchronize()
        out[f"R{beams}_us"] = round((with_reset - ev[0].elapsed_time(ev[1])) / reps * 1e3, 1)
    return out


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
    ap.add_argument("--beams", type=int, default=10)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--step-beams", default="1,4,10,32,64,100", help="beam counts --steps-only times")
    ap.add_argument("--variable-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--share-from", default=None)
    a = ap.parse_args()
    if a.share_from:
        print(json.dumps(kernel_share(a.share_from)))
        return
    import torch

    import synth
    from mevi_amd import nci

    M, R = a.depth, a.beams
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    if a.steps_only:
        out = {"shape": {"queries": a.batch, "K": K, "max_codes": M},
               "beam_step": step_times(dev, M, a.batch, rng, [int(r) for r in a.step_beams.split(",")])}
        print(json.dumps(out))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
        return
    codes, lengths = synthetic_ids(a.ids, rng, M)
    t = time.perf_counter()
    tree = nci.RaggedPrefixTree(codes, K, dev, lengths=lengths, levels=M + 1)
    build_s = time.perf_counter() - t
    model = synth.build(dev, M, K, a.batch)[0]
    ids, mask = synth.query_ids(a.queries, dev, rng)

    def run(**kw):
        return [model.generate(ids[b:b + a.batch], mask[b:b + a.batch], num_beams=R, **kw)[0] for b in range(0, a.queries, a.batch)]

    out = {"shape": {"queries": a.queries, "batch": a.batch, "beams": R, "K": K, "max_codes": M, "ids": a.ids,
                     "distinct_ids": tree.n_paths, "nodes_per_level": tree.n_nodes}, "tree_build_s": round(build_s, 2)}
    for name, kw in (("fixed_depth", {}), ("variable_depth", {"decode_tree": tree}))[1 if a.variable_only else 0:]:
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
    if not a.variable_only:
        out["variable_over_fixed_time"] = round(out["variable_depth_ms"] / out["fixed_depth_ms"], 4)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
