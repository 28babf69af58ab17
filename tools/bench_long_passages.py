#!/usr/bin/env python3
"""The passage tower at t5-base shapes at 128, 384 and 512 tokens per passage (gen_doc_embedding --doc_length N), in
tokens per second on one GPU.  128 tokens run the kernels they always ran (the reference figure); longer passages run the
block-streaming attention (mevi_amd/csrc/attention_long.hip).  Lengths are ragged the way tools/bench_passage.py draws them
(mean 0.55 N, right-padded), the same number of padded tokens at every N.
  python tools/bench_long_passages.py [--tokens 128,384,512] [--padded-tokens 262144] [--pass-tokens 65536] [--steps 3]
Per-kernel times (the two long kernels per layer at 512 tokens):
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_long_passages.py --tokens 512 --steps 1
One JSON line per length."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mevi_amd import hip, t5  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", default="128,384,512")
ap.add_argument("--padded-tokens", type=int, default=262144, help="padded tokens per measurement (2048 passages of 128)")
ap.add_argument("--pass-tokens", type=int, default=65536, help="padded tokens per device pass (512 passages of 128)")
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
args = ap.parse_args()

hip.require_gpu()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
d, ff, H, NL = 768, 3072, 12, 12


def rn(*shape, s=1.0):
    return torch.randn(shape, device=dev, generator=g) * s


W = {"shared.weight": rn(32128, d)}
for stack, dec in (("encoder", False), ("decoder", True)):
    for l in range(NL):
        p = f"{stack}.block.{l}.layer"
        for nm in "qkvo":
            W[f"{p}.0.SelfAttention.{nm}.weight"] = rn(d, d, s=d ** -0.5)
        W[f"{p}.0.layer_norm.weight"] = torch.ones(d, device=dev)
        i = 1
        if dec:
            for nm in "qkvo":
                W[f"{p}.1.EncDecAttention.{nm}.weight"] = rn(d, d, s=d ** -0.5)
            W[f"{p}.1.layer_norm.weight"] = torch.ones(d, device=dev)
            i = 2
        W[f"{p}.{i}.DenseReluDense.wi.weight"] = rn(ff, d, s=d ** -0.5)
        W[f"{p}.{i}.DenseReluDense.wo.weight"] = rn(d, ff, s=ff ** -0.5)
        W[f"{p}.{i}.layer_norm.weight"] = torch.ones(d, device=dev)
    W[f"{stack}.block.0.layer.0.SelfAttention.relative_attention_bias.weight"] = rn(32, H)
    W[f"{stack}.final_layer_norm.weight"] = torch.ones(d, device=dev)

for N in (int(x) for x in args.tokens.split(",")):
    n = max(1, args.padded_tokens // N)
    tower = t5.TwinTower(W, device=dev, num_layers=NL, num_decoder_layers=NL, batch_size=max(1, args.pass_tokens // N))
    rng = np.random.default_rng(0)
    ids = np.zeros((n, N), np.int64)
    mask = np.zeros((n, N), np.int64)
    for i in range(n):
        L = int(np.clip(rng.normal(0.55 * N, 0.23 * N), 8, N))
        ids[i, :L - 1] = rng.integers(3, 32100, size=L - 1)
        ids[i, L - 1] = 1
        mask[i, :L] = 1
    mask[0] = 1                                      # one passage fills the window
    ids[0] = rng.integers(3, 32100, size=N)
    psg = {"input_ids": torch.from_numpy(ids).to(dev), "attention_mask": torch.from_numpy(mask).to(dev)}
    for _ in range(args.warmup):
        tower.encode_passage(psg)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        t = time.perf_counter()
        out = tower.encode_passage(psg)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    assert bool(torch.isfinite(out).all())
    med = statistics.median(ms)
    real = int(mask.sum())
    print(json.dumps({"tokens_per_passage": N, "passages": n, "real_tokens": real, "longest": int(mask.sum(1).max()),
                      "ms": round(med, 2), "ms_all": [round(x, 2) for x in ms], "real_tokens_per_s": round(real / med * 1e3),
                      "padded_tokens_per_s": round(n * N / med * 1e3), "passages_per_s": round(n / med * 1e3, 1)}), flush=True)
    del tower
