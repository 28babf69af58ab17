#!/usr/bin/env python3
"""mevi_query_pool_f32 at C4 scale (--query_encoder nci): 6980 queries x R = 10 beams, d = 768, S = 32 encoder rows,
M + 1 = 5 decoder positions, every qtower x accum the eval scripts use.  Prints one JSON line per mode with the median
event time and the bytes the kernel must move (encoder once per query + the beams' decoder rows + the output).
Kernel times for the record come from `rocprofv3 --kernel-trace --stats -- python tools/bench_qpool.py`."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mevi_amd import ops  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--queries", type=int, default=6980)
    p.add_argument("--beams", type=int, default=10)
    p.add_argument("--seq", type=int, default=32)
    p.add_argument("--positions", type=int, default=5)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--reps", type=int, default=20)
    a = p.parse_args()
    dev = torch.device("cuda")
    B, R, S, T, d = a.queries, a.beams, a.seq, a.positions, a.dim
    g = torch.Generator(device=dev).manual_seed(0)
    enc = torch.randn((B, S, d), device=dev, generator=g)
    mask = (torch.arange(S, device=dev)[None, :] < torch.randint(4, S + 1, (B, 1), device=dev, generator=g)).long()
    steps = torch.randn((T, B * R, d), device=dev, generator=g)
    # ancestors as a beam search leaves them: position t of beam row i sits in some row of query i // R at step t
    anc = ((torch.arange(B * R, device=dev) // R)[:, None] * R
           + torch.randint(0, R, (B * R, T), device=dev, generator=g)).to(torch.int32).contiguous()
    tab = torch.randn((32 * 6 + 2, d), device=dev, generator=g)
    ids = torch.randint(0, tab.shape[0], (B * R,), device=dev, generator=g)
    w = torch.randn(d, device=dev, generator=g) * 0.05
    out = torch.empty((B * R, d), device=dev)
    for qtower, accum in [("encmask_dec", "attenpool"), ("enc_dec", "maxpool"), ("encmask_dec", "avgpool"),
                          ("encmask_dec_emb", "attenpool")]:
        mode = ops.qpool_mode(qtower, accum)
        run = lambda: ops.query_pool(mode, R, enc=enc, mask=mask, dec=(steps, anc), emb_ids=ids, emb_table=tab,  # noqa: E731
                                     atten_w=w, atten_b=0.1, out=out)
        for _ in range(3):
            run()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        nbytes = 4 * (B * S * d + B * R * T * d + B * R * d)
        print(json.dumps(dict(qtower=qtower, accum=accum, queries=B, beams=R, seq=S, positions=T, dim=d,
                              median_ms=round(times[len(times) // 2], 4), min_ms=round(times[0], 4),
                              gbytes=round(nbytes / 1e9, 3), gb_per_s=round(nbytes / 1e6 / times[len(times) // 2], 1))))


if __name__ == "__main__":
    main()
