#!/usr/bin/env python3
"""PQ encode (csrc/pq_encode.hip) of the C2 corpus (8,841,823 x 768 f32) at (M, K) = (4, 32), (4, 256) and (32, 256).
Codes are checked against the exact RQ kernel run per column slice with a one-level codebook on a sample of rows
(the same arithmetic: they must be identical); GB/s = (4 N dim + 4 N M) bytes / time.
  python tools/bench_pq.py [rows] [out.json]"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from mevi_amd import rq  # noqa: E402

SAMPLE = 1 << 17
REPS = 3

dev = torch.device("cuda", 0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else bench.N_DOCS
docs = bench.gen_shard(0, n, dev, n)
g = torch.Generator(device=dev).manual_seed(11)
out = {"rows": n, "dim": bench.DIM, "device": torch.cuda.get_device_name(0), "reps": REPS}
for M, K in ((4, 32), (4, 256), (32, 256)):
    dsub = bench.DIM // M
    # sub-centroids drawn from the corpus's own slices (+ noise), so codes spread over the whole codebook
    pick = torch.randint(n, (M, K), device=dev, generator=g)
    cb = torch.stack([docs[pick[j], j * dsub:(j + 1) * dsub] for j in range(M)])
    cb = (cb + 0.01 * torch.randn(cb.shape, device=dev, generator=g)).contiguous()
    rq.pq_encode(docs[:1 << 16], cb)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(REPS):
        codes = rq.pq_encode(docs, cb)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) / REPS * 1e3
    byts = 4.0 * n * bench.DIM + 4.0 * n * M
    lane_ops = 2.0 * n * M * K * dsub                    # one subtract + one fma per (row, centroid, k)
    rows = torch.randperm(n, device=dev, generator=g)[:min(SAMPLE, n)]
    xs = docs[rows]
    exact = torch.stack([rq.rq_encode(xs[:, j * dsub:(j + 1) * dsub].contiguous(), cb[j:j + 1], mode="exact")[:, 0]
                         for j in range(M)], 1)
    res = {"ms": round(ms, 2), "gb_per_s": round(byts / ms / 1e6, 1), "valu_tlane_ops_per_s": round(lane_ops / ms / 1e9, 1),
           "sample_rows": int(rows.numel()), "sample_identical_to_exact_rq_per_slice": bool(torch.equal(codes[rows], exact)),
           "distinct_codes_level0": int(torch.unique(codes[:, 0]).numel())}
    out["pq_%dx%d" % (M, K)] = res
    print(json.dumps({("pq_%dx%d" % (M, K)): res}), flush=True)
    del codes, cb, xs, exact
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
