"""The fused beam encode (`ProductQuantization.beam_search` -> mevi_rq_beam_encode_f32) against the per-level composition it
replaces (`_beam_search_steps`, driven 65 536 rows at a time as `get_topk_document_mapping` drove it) on one MI355X.

Corpus: the bench's synthetic corpus (bench.gen_shard), codebooks TRAINED on a strided sample of it (residual k-means for
'rq', per-subspace k-means for 'pq').  Shapes: rq (4, 32) R = 3, rq (3, 256) R = 3, pq (4, 32) R = 3, rq (4, 32) R = 10.

Both paths run in ONE process, alternating window by window; a window is one pass over the whole corpus with the device
synchronised before and after; the figure is the median of `--windows` windows after a warm-up pass of each path.  Before
anything is timed the labels and the probability bits of the two paths are compared over the whole corpus.  Per shape the
record also holds `get_topk_document_mapping` end to end on the device-resident corpus (one call and one copy back, against
the composition's batches with a copy back each) and the fused call's share of the f32 VALU rate: the algorithmic lane-ops
2 * n * chains * K * chain length (one subtraction and one fma per (row, centroid, k); chains = 1 + (M - 1) * R score rows
per document for 'rq', M for 'pq') over the call's time, against 78.6 T lane-ops/s.

    python tools/bench_rq_beam.py [--docs N] [--windows 5] [--out profiles/rq_beam_encode.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402
from chain_c4 import sync_time  # noqa: E402
from mevi_amd import hip, rq  # noqa: E402

bench.late_imports()          # bench.py binds torch / numpy lazily: its corpus generator needs them

SHAPES = (("rq", 4, 32, 3), ("rq", 3, 256, 3), ("pq", 4, 32, 3), ("rq", 4, 32, 10))
VALU_PEAK = 78.6e12           # f32 lane-ops per second
STEPS_BATCH = 1 << 16         # get_topk_document_mapping's default batch: how the composition is driven over a corpus


def trained(kind, docs, M, K, sample=200_000):
    step = max(1, docs.shape[0] // sample)
    train = rq.train_rq_codebook if kind == "rq" else rq.train_pq_codebook
    book, _ = train(docs[::step][:sample].contiguous(), M, K, seed=1, n_init=1, max_iter=10)
    obj = rq.ProductQuantization(kind, M, int(np.log2(K)), emb_size=docs.shape[1], device=docs.device)
    obj.load_codebook(book)
    return obj


def steps_pass(obj, docs, R, out_l, out_p):
    for s in range(0, docs.shape[0], STEPS_BATCH):
        lab, pr = obj._beam_search_steps(docs[s:s + STEPS_BATCH], R, True)
        out_l[s:s + STEPS_BATCH] = lab
        out_p[s:s + STEPS_BATCH] = pr


def medians(paths, n_windows):
    for fn in paths.values():
        sync_time(fn)
    ms = {name: [] for name in paths}
    for _ in range(n_windows):
        for name, fn in paths.items():
            ms[name].append(sync_time(fn)[0] * 1e3)
    return {name: round(float(np.median(v)), 2) for name, v in ms.items()}, {name: [round(x, 2) for x in v] for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=bench.N_DOCS)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rq_beam_encode.json"))
    args = ap.parse_args()
    assert args.windows >= 3
    hip.require_gpu()
    dev = torch.device("cuda:0")
    os.environ.pop("MEVI_RQ_BEAM", None)
    docs = bench.gen_shard(0, args.docs, dev, args.docs)
    n, dim = docs.shape
    rec = {"workload": f"top-R code paths of the corpus {n} x {dim}, trained codebooks; fused = one mevi_rq_beam_encode_f32 call, "
                       f"steps = the per-level composition in batches of {STEPS_BATCH} rows",
           "statistic": f"median of {args.windows} windows per path after one warm-up pass, paths alternating, device synchronised "
                        "around each window; ms per pass over the corpus", "rows": []}
    for kind, M, K, R in SHAPES:
        obj = trained(kind, docs, M, K)
        assert obj.beam_search_is_fused(R)
        lab, pr = obj.beam_search(docs, R, return_proba=True)
        want_l = torch.empty_like(lab)
        want_p = torch.empty_like(pr)
        steps_pass(obj, docs, R, want_l, want_p)
        torch.cuda.synchronize()
        row = {"pq_type": kind, "M": M, "K": K, "R": R,
               "tile_docs": int(hip.lib().mevi_rq_beam_encode_tile_docs(dim, M, K, R, int(kind == "pq"))),
               "label_rows_differing": int((lab != want_l).any(-1).any(-1).sum().item()),
               "proba_bits_differing": int((pr.view(torch.int32) != want_p.view(torch.int32)).sum().item())}
        del lab, pr
        row["ms"], row["ms_windows"] = medians({"steps": lambda: steps_pass(obj, docs, R, want_l, want_p),
                                                "fused": lambda: obj.beam_search(docs, R, return_proba=True)}, args.windows)
        del want_l, want_p

        def mapping(mode):
            if mode == "steps":
                os.environ["MEVI_RQ_BEAM"] = "steps"
            try:
                return obj.get_topk_document_mapping(docs, 0, 1, R)
            finally:
                os.environ.pop("MEVI_RQ_BEAM", None)

        same = torch.equal(mapping("fused"), mapping("steps"))
        e2e, e2e_w = medians({"steps": lambda: mapping("steps"), "fused": lambda: mapping("fused")}, 3)
        row["topk_document_mapping_ms"], row["topk_document_mapping_ms_windows"], row["topk_document_mapping_identical"] = e2e, e2e_w, same
        chains = M if kind == "pq" else 1 + (M - 1) * R
        lane_ops = 2.0 * n * chains * K * (dim // M if kind == "pq" else dim)
        row["steps_over_fused"] = round(row["ms"]["steps"] / row["ms"]["fused"], 2)
        row["fused_T_lane_ops_per_s"] = round(lane_ops / (row["ms"]["fused"] * 1e-3) / 1e12, 2)
        row["fused_share_of_f32_valu"] = round(lane_ops / (row["ms"]["fused"] * 1e-3) / VALU_PEAK, 3)
        row["fused_x_read_TB_per_s"] = round(4.0 * n * dim / (row["ms"]["fused"] * 1e-3) / 1e12, 3)
        print(json.dumps(row), flush=True)
        rec["rows"].append(row)
    rec["all_identical"] = all(r["label_rows_differing"] == 0 and r["proba_bits_differing"] == 0 and r["topk_document_mapping_identical"]
                               for r in rec["rows"])
    rec["fused_no_slower_in_every_row"] = all(r["ms"]["fused"] <= r["ms"]["steps"] for r in rec["rows"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({"all_identical": rec["all_identical"], "fused_no_slower_in_every_row": rec["fused_no_slower_in_every_row"],
                      "out": args.out}))
    return 0 if rec["all_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
