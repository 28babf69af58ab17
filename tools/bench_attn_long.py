#!/usr/bin/env python3
"""ops.attention_long alone on padded [nb, S, 12 x 64] operands with the bias table, full lengths, against the f32
matrix cores' bound for its three products (Q.K^T twice, P.V), and the one-block f32 kernel at 128 tokens beside it.
  python tools/bench_attn_long.py"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mevi_amd import hip, ops
if os.environ.get("MEVI_PROBE_LIB"):
    hip.LIB = os.path.abspath(os.environ["MEVI_PROBE_LIB"])
dev = torch.device("cuda:0")
def t(fn, n=5):
    fn(); torch.cuda.synchronize()
    a = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - a) / n * 1e3
H = 12
for nb, S in ((128, 512), (170, 384), (512, 129)):
    qkv = torch.randn((nb, S, 3 * 768), device=dev)
    bias = torch.randn((H, S, S), device=dev)
    ms = t(lambda: ops.attention_long(qkv[:, :, :768], qkv[:, :, 768:1536], qkv[:, :, 1536:], H, bias=bias))
    nblk = -(-S // 128)
    mfma_ms = nb * H * nblk * nblk * 384 * 4 * 64 / 1024 / 2.4e9 * 1e3
    print(f"long nb {nb} S {S}: {ms:.3f} ms  (f32 MFMA bound at 2.4 GHz {mfma_ms:.3f} ms, {6*S*S*64*H*nb/ms/1e9:.1f} TFLOP/s incl. 2nd QK)")
nb, S = 2048, 128
qkv = torch.randn((nb, S, 3 * 768), device=dev)
bias = torch.randn((H, S, S), device=dev)
ms = t(lambda: ops.attention(qkv[:, :, :768], qkv[:, :, 768:1536], qkv[:, :, 1536:], H, bias=bias))
print(f"one-block f32 kernel nb {nb} S {S}: {ms:.3f} ms (bound {nb*H*256*4*64/1024/2.4e9*1e3:.3f} ms) route {hip.attn_route_name(ops.attention_route(qkv[:, :, :768], qkv[:, :, 768:1536], qkv[:, :, 1536:], H, bias=bias))}")
ms = t(lambda: ops.attention_long(qkv[:, :, :768], qkv[:, :, 768:1536], qkv[:, :, 1536:], H, bias=bias))
print(f"long kernel on the same: {ms:.3f} ms")
