"""--pq_type opq at C2 size (8,841,823 x 768, tools/synth.py's ance_scale corpus) at (M, bits) = (4, 5) and (32, 8), in one process:
  initialize   ProductQuantization('opq').initialize without a file: the rotation trainer, the rotated sample, its k-means;
  encode       the cluster codes of the whole corpus, both ways, taking turns (median of 3 windows after a warm-up, tools/bench_ivf.py:
               timed) -- fused = mevi_opq_encode_f32, one launch; steps = the composition of the two existing kernels
               (mevi_opq_rotate_rows_f32 then mevi_pq_encode_f32, unchanged since the parent) in chunks of ivfpq.ENCODE_CHUNK rows --
               with the peak extra device memory of each and a bit comparison of the codes;
  topk         get_topk_document_mapping at C = 3 (a chunk rotated, then the fused 'pq' beam encode).
  python tools/bench_opq_clusters.py [--shapes 4x5,32x8] [--docs N] [--niter 50] [--out profiles/opq_clusters_c2.json]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import synth  # noqa: E402
from bench_ivf import timed  # noqa: E402
from mevi_amd import ivfpq, opq, rq  # noqa: E402

F32_MATRIX_PEAK = 157.3e12              # FLOP/s of v_mfma_f32_32x32x2_f32 on 256 CUs at 2.4 GHz


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, round(time.perf_counter() - t, 3)


def peak_extra_bytes(fn):
    """Bytes the allocator handed out above what was live before the call."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, int(torch.cuda.max_memory_allocated() - before)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4x5,32x8")
    ap.add_argument("--docs", type=int, default=bench.N_DOCS)
    ap.add_argument("--niter", type=int, default=opq.NITER)
    ap.add_argument("--topk", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["MEVI_OPQ_NITER"] = str(a.niter)
    dev = torch.device("cuda:0")
    docs, _ = synth.corpus("ance_scale", dev, a.docs)
    n, dim = docs.shape
    table = {"docs": n, "dim": dim, "niter": a.niter, "encode_chunk": ivfpq.ENCODE_CHUNK, "default": rq.OPQ_ENCODE_DEFAULT,
             "f32_matrix_peak_flops": F32_MATRIX_PEAK,
             "note": "fused_ms / steps_ms = the codes of the whole corpus by mevi_opq_encode_f32 / by rotate + encode in chunks, median of "
                     "3 windows after a warm-up, taking turns; *_peak_fraction = 2 n dim^2 / s / the f32 matrix peak; *_extra_bytes = "
                     "peak device memory above the corpus, R and the codebook (the codes themselves included); initialize_s = "
                     "rotation training + rotated sample + its k-means; topk_s = get_topk_document_mapping at C = topk",
             "rows": []}
    for shape in a.shapes.split(","):
        M, bits = (int(v) for v in shape.split("x"))
        pq = rq.ProductQuantization("opq", M, bits, "l2", dim, pq_init_method="faiss", device=dev)
        _, t_init = clock(lambda: pq.initialize(None, docs, rank=0, seed=41))
        row = {"M": M, "bits": bits, "dsub": dim // M, "initialize_s": t_init, "train": dict(opq.LAST_TRAIN)}
        R, cb = pq.rotate, pq.codebook
        fused, row["fused_extra_bytes"] = peak_extra_bytes(lambda: rq.opq_encode(docs, R, cb, mode="fused"))
        steps, row["steps_extra_bytes"] = peak_extra_bytes(lambda: rq.opq_encode(docs, R, cb, mode="steps"))
        row["codes_bit_equal"] = bool(torch.equal(fused, steps))
        row["clusters"] = int(torch.unique(fused, dim=0).shape[0])
        del fused, steps
        t_f, t_s = timed([lambda: rq.opq_encode(docs, R, cb, mode="fused"), lambda: rq.opq_encode(docs, R, cb, mode="steps")])
        flops = 2.0 * n * dim * dim
        row.update(fused_ms=round(t_f * 1e3, 3), steps_ms=round(t_s * 1e3, 3), fused_over_steps=round(t_f / t_s, 3),
                   fused_peak_fraction=round(flops / t_f / F32_MATRIX_PEAK, 4), steps_peak_fraction=round(flops / t_s / F32_MATRIX_PEAK, 4))
        pq.get_topk_document_mapping(docs[:ivfpq.ENCODE_CHUNK], 0, 1, a.topk)      # warm-up
        _, row["topk_s"] = clock(lambda: pq.get_topk_document_mapping(docs, 0, 1, a.topk))
        table["rows"].append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(table, f, indent=1)


if __name__ == "__main__":
    main()
