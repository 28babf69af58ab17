"""OPQ in front of PQ (faiss_search.py --param OPQ<m>,[IVF<n>,]PQ<m> / ...PQ<m>x4fs) at C2 size on the synthetic corpora of
tools/synth.py, in one process.  Per corpus the rotation is trained once (M = m) and the corpus rotation is timed both ways, in
chunks as the build does it:
  fused  mevi_opq_rotate_rows_f32: gather + GEMM + centroid subtraction in one launch;
  steps  MEVI_OPQ_ROTATE=steps: gather, ops.linear, gather of crot, subtract (the same bits);
with the fraction of the f32 matrix peak each reaches.  Per (nlist, code kind) two indexes over the same centroids and lists take
turns: the OPQ index and the same index without OPQ (the parent's code path); per (nprobe, query count): ms of the whole search
(median of 3 timed windows after a warm-up, tools/bench_ivf.py: timed), the ms of the added nq x dim x dim GEMM alone,
recall@1/10/1000 of both against the exact search, and the bytes of codes.  nlist 0 is the flat index.
  python tools/bench_opq.py [nlist,...] [nprobe,...] [--corpus ance_scale,iid] [--codes pq8,fs] [--m 64] [--nq 1,8,32,6980]
                            [--k 1000] [--docs N] [--niter 50] [--out table.json]"""
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
from bench_ivf import ints, recall, timed  # noqa: E402
from mevi_amd import dense, ivf, ivfpq, opq, ops, pqfs  # noqa: E402

F32_MATRIX_PEAK = 157.3e12              # FLOP/s of v_mfma_f32_32x32x2_f32 on 256 CUs at 2.4 GHz


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, round(time.perf_counter() - t, 3)


def rotate_corpus(docs, rows, list_of, crot, R, mode):
    """Seconds of rotating every row chunk by chunk, as ivfpq.encode does it (the rotated chunk is dropped)."""
    def run():
        for a in range(0, docs.shape[0], ivfpq.ENCODE_CHUNK):
            if rows is None:
                dense.opq_rotate_rows(docs[a:a + ivfpq.ENCODE_CHUNK], None, None, None, R, mode=mode)
            else:
                dense.opq_rotate_rows(docs, rows[a:a + ivfpq.ENCODE_CHUNK], list_of, crot, R, mode=mode)
    run()                                                        # warm-up: kernels loaded, the allocator has its blocks
    return clock(run)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("nlist", nargs="?", default="100,4096,0")
    ap.add_argument("nprobe", nargs="?", default="1,4,16")
    ap.add_argument("--corpus", default="ance_scale,iid")
    ap.add_argument("--codes", default="pq8,fs")
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--nq", default=f"1,8,32,{bench.N_QUERIES}")
    ap.add_argument("--k", type=int, default=bench.TOPK)
    ap.add_argument("--docs", type=int, default=bench.N_DOCS)
    ap.add_argument("--niter", type=int, default=opq.NITER)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nqs, k, m = ints(a.nq), a.k, a.m
    table = {"docs": a.docs, "m": m, "k": k, "niter": a.niter, "f32_matrix_peak_flops": F32_MATRIX_PEAK,
             "note": "opq_ms / plain_ms = the whole search (rotation GEMM + coarse + scan + select) of the OPQ index and of the same "
                     "index without OPQ over the same centroids and lists, median of 3 windows after a warm-up, taking turns; "
                     "rotate_queries_ms = the added nq x dim x dim GEMM alone; rotate_*_s = rotating the whole corpus chunk by chunk "
                     "(fused kernel / composition of existing calls), *_peak_fraction = 2 n dim^2 / s / the f32 matrix peak; "
                     "train_device_s / train_svd_s = the rotation trainer's device part and host float64 SVDs; nlist 0 = the flat index",
             "corpora": [], "builds": [], "rows": []}

    def save():
        if a.out:                                                # after every row: a long table survives a short limit
            with open(a.out, "w") as f:
                json.dump(table, f, indent=1)

    for kind in a.corpus.split(","):
        docs, info = synth.corpus(kind, dev, a.docs)
        dim = docs.shape[1]
        q_all = synth.corpus_queries(kind, docs, max(nqs), info)[0]
        exact_ids = dense.DenseIndex(docs).search(q_all, k)[1]
        torch.cuda.empty_cache()
        (R, errors), t_train = clock(lambda: opq.train_rotation(docs, m, niter=a.niter))
        flops = 2.0 * docs.shape[0] * dim * dim
        c = {"corpus": kind, "dim": dim, "train_s": t_train, "train_device_s": round(opq.LAST_TRAIN["device_s"], 3),
             "train_svd_s": round(opq.LAST_TRAIN["svd_s"], 3), "error_first": errors[0], "error_last": errors[-1]}
        for mode in ("fused", "steps"):
            c[f"rotate_{mode}_s"] = rotate_corpus(docs, None, None, None, R, mode)
            c[f"rotate_{mode}_peak_fraction"] = round(flops / max(c[f"rotate_{mode}_s"], 1e-9) / F32_MATRIX_PEAK, 4)
        table["corpora"].append(c)
        print(json.dumps(c), flush=True)
        save()
        for nlist_arg in ints(a.nlist):
            nlist = nlist_arg or None
            cent, t_coarse = clock(lambda: ivf.train_centroids(docs, nlist)) if nlist else (None, 0.0)
            gathered = {}
            if nlist:                                            # the IVF build's form of the step: gathered rows, centroids subtracted
                list_of = ivf.assign(docs, cent)
                ids = ivf.build_lists(list_of, nlist)[2]
                crot = ops.linear(cent, R)
                gathered = {f"rotate_gathered_{mode}_s": rotate_corpus(docs, ids, list_of, crot, R, mode) for mode in ("fused", "steps")}
                del list_of, ids, crot
            for code in a.codes.split(","):
                fs, nbits = code == "fs", (4 if code == "fs" else int(code[2:]))
                plain_cls = (lambda **kw: pqfs.PQFSIndex(docs, nlist, m, centroids=cent, **kw)) if fs else (
                    lambda **kw: ivfpq.IVFPQIndex(docs, nlist, m, nbits, centroids=cent, **kw))
                plain, t_plain = clock(plain_cls)
                rot, t_rot = clock(lambda: opq.OPQIndex(docs, m, nlist, m, nbits, fs, R=R, centroids=cent))
                b = {"corpus": kind, "nlist": nlist_arg, "codes": code, "train_coarse_s": t_coarse, "plain_build_s": t_plain,
                     "opq_build_s": t_rot, "code_bytes": rot.codes.numel(), "plain_code_bytes": plain.codes.numel(), **gathered}
                table["builds"].append(b)
                print(json.dumps(b), flush=True)
                save()
                for nprobe in (ints(a.nprobe) if nlist else [1]):
                    for nq in nqs:
                        q = q_all[:nq].contiguous()
                        t_o, t_p, t_g = timed([lambda: rot.search_scan(q, k, nprobe), lambda: plain.search_scan(q, k, nprobe),
                                               lambda: ops.linear(q, R)])
                        row = {"corpus": kind, "nlist": nlist_arg, "codes": code, "nprobe": nprobe, "nq": nq, "k": k,
                               "opq_ms": round(t_o * 1e3, 4), "plain_ms": round(t_p * 1e3, 4), "opq_over_plain": round(t_o / t_p, 3),
                               "rotate_queries_ms": round(t_g * 1e3, 4),
                               "opq_recall": recall(rot.search_scan(q, k, nprobe)[1], exact_ids[:nq]),
                               "plain_recall": recall(plain.search_scan(q, k, nprobe)[1], exact_ids[:nq])}
                        table["rows"].append(row)
                        print(json.dumps(row), flush=True)
                        save()
                del plain, rot
                torch.cuda.empty_cache()
        del docs, q_all, exact_ids
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
