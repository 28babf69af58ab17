"""Beam encoding of the residual-quantiser indexes (MEVI_RQINDEX_BEAM, mevi_rq_errbeam_step_f32) measured, in one process, on the
`ance_scale` corpus of tools/synth.py at C2 size.  Three parts (--parts):
  kernel  the fused step against the composition it replaces (MEVI_RQINDEX_BEAM_STEP=steps: mevi_rq_neg_dist_f32 -> torch.sort of the
          packed keys -> mevi_gather_sub_f32) on identical inputs at (B, K, dim) = (5, 256, 768) and (16, 256, 768): ms per call (median
          of 3 windows after a warm-up, the two taking turns: tools/bench_ivf.py: timed), outputs compared bit for bit, and the step's
          rate in (row, centroid, column) sub+fma pairs per second beside the packed-f32 VALU issue peak
  index   per shape (--shapes RQ64x8,RQ32x8,IVF100,RQ64x8 separated by ';') one greedy-trained codebook, then per beam (--beams): add
          seconds, code_mse (mean squared reconstruction error of the stored codes: the last level's err[:, 0]; at beam 1 the walk's own,
          timed apart from the greedy add), recall@10 / @1000 against the exact search at --nq queries of a k = 1000 search, and behind
          ',RFlat' at k_factor 4 for k = 10 and k = 1000
  train   MEVI_RQINDEX_TRAIN_BEAM=5 against 1 on the first shape: training seconds, beam_mse, then code_mse and recall under beam-5 encoding
  python tools/bench_rqindex_beam.py [--docs N] [--nq 6980] [--parts kernel,index,train] [--shapes ...] [--beams 1,2,5,16] [--out table.json]
"""
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
from mevi_amd import dense, ivf, refine, rqindex  # noqa: E402

PK_F32_LANE_OPS = 256 * 4 * 32 * 2.4e9      # v_pk_* f32 lane operations per second: 256 CUs x 4 SIMDs x 16 lanes x 2 (packed) at 2.4 GHz


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, round(time.perf_counter() - t, 3)


def kernel_rows(docs, rows_total=1 << 17):
    """The step against the composition at B = L = 5 and 16 on 2^17 rows: B consecutive corpus rows stand for a document's B residual
    rows and 256 corpus rows for the centroids (the arithmetic does not depend on the values; equal rows would only add ties)."""
    out = []
    dim, K = docs.shape[1], 256
    cent = docs[torch.randperm(docs.shape[0], device=docs.device, generator=torch.Generator(device=docs.device).manual_seed(7))[:K]].contiguous()
    for B in (5, 16):
        n = rows_total // B
        res_in = docs[:n * B].view(n, B, dim).contiguous()
        res_out = torch.empty((n, B, dim), dtype=torch.float32, device=docs.device)
        ws = torch.empty(dense.rq_errbeam_step_workspace_bytes(n, dim, K, B, B), dtype=torch.uint8, device=docs.device)
        fused = lambda: dense.rq_errbeam_step(res_in, cent, B, res_out=res_out, workspace=ws)              # noqa: E731
        steps = lambda: rqindex.beam_step_composed(res_in, cent, B, res_out=res_out)                         # noqa: E731
        a = [t.clone() for t in fused()]
        b = steps()
        torch.cuda.synchronize()
        same = all(torch.equal(x, y) if x.dtype == torch.uint8 else torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
        t_fused, t_steps = timed([fused, steps], min_window=0.3)
        pairs = n * B * K * dim
        row = {"part": "kernel", "B": B, "L": B, "K": K, "dim": dim, "docs": n, "tile_docs": dense.rq_errbeam_step_tile_docs(dim, K, B, B),
               "fused_ms": round(t_fused * 1e3, 3), "steps_ms": round(t_steps * 1e3, 3), "fused_over_steps": round(t_fused / t_steps, 4),
               "bit_identical": bool(same), "pairs_per_s": round(pairs / t_fused, 0),
               "share_of_pk_f32_issue_peak": round(2 * pairs / t_fused / PK_F32_LANE_OPS, 4)}
        out.append(row)
    return out


def measure(index, docs, q, exact):
    """recall of a k = 1000 search (its @10 is that of its first ten) and behind ',RFlat' at k_factor 4 for k = 10 and k = 1000."""
    nprobe = 1
    ids = index.search(q, 1000, nprobe)[1]
    row = {"recall": recall(ids, exact)}
    ref = refine.RefineIndex(index, docs)
    row["rflat4_k10"] = recall(ref.search(q, 10, nprobe, k_factor=4)[1], exact[:, :10])
    row["rflat4_k1000"] = recall(ref.search(q, 1000, nprobe, k_factor=4)[1], exact)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=bench.N_DOCS)
    ap.add_argument("--nq", type=int, default=bench.N_QUERIES)
    ap.add_argument("--parts", default="kernel,index,train")
    ap.add_argument("--shapes", default="RQ64x8;RQ32x8;IVF100,RQ64x8")
    ap.add_argument("--beams", default="1,2,5,16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for name in ("MEVI_RQINDEX_BEAM", "MEVI_RQINDEX_TRAIN_BEAM", "MEVI_RQINDEX_BEAM_STEP"):
        os.environ.pop(name, None)
    dev = torch.device("cuda:0")
    parts, shapes = a.parts.split(","), [s for s in a.shapes.split(";") if s]
    docs, info = synth.corpus("ance_scale", dev, a.docs)
    table = {"docs": a.docs, "dim": docs.shape[1], "corpus": "ance_scale", "nq": a.nq,
             "note": "add_s = RQIndex(...) with given centroids and codebook (lists + encode); code_mse = mean over all rows of the stored "
                     "path's squared reconstruction error; recall vs the exact search, keys = cut-offs of a k = 1000 search; rflat4 = behind "
                     "',RFlat' at k_factor 4; kernel rows: see the tool's docstring", "rows": []}

    def emit(row):
        table["rows"].append(row)
        print(json.dumps(row), flush=True)
        if a.out:                                                # after every row: a long table survives a short limit
            with open(a.out, "w") as f:
                json.dump(table, f, indent=1)

    if "kernel" in parts:
        for row in kernel_rows(docs):
            emit(row)
    if "index" not in parts and "train" not in parts:
        return
    q = synth.corpus_queries("ance_scale", docs, a.nq, info)[0]
    exact = dense.DenseIndex(docs).search(q, 1000)[1]
    torch.cuda.empty_cache()
    for s, shape in enumerate(shapes):
        nlist, M, nbits = rqindex.parse_factory(shape)
        cent = ivf.train_centroids(docs, nlist) if nlist else None
        list_of = ivf.assign(docs, cent) if cent is not None else None
        stats, greedy5 = {}, None
        book, t_train = clock(lambda: rqindex.train_codebook(docs, list_of, cent, M, nbits, stats=stats))
        if "index" in parts:
            for beam in ints(a.beams):
                index, t_add = clock(lambda: rqindex.RQIndex(docs, nlist, M, nbits, centroids=cent, codebook=book, beam=beam))
                row = {"part": "index", "index": shape, "beam": beam, "train_codebook_s": t_train, "add_s": t_add,
                       "code_mse": index.encode_stats.get("code_mse")}
                if beam == 1:                                    # the greedy codes' error by the walk's own route (same codes), timed apart
                    st = {}
                    _, row["walk_beam1_s"] = clock(lambda: rqindex.encode_walk(docs, None if nlist is None else index.ids, index.list_of,
                                                                               cent, book, 1, stats=st))
                    row["code_mse"] = st["code_mse"]
                row.update(measure(index, docs, q, exact))
                emit(row)
                if beam == 5:
                    greedy5 = row
                del index
                torch.cuda.empty_cache()
        if "train" in parts and s == 0:
            os.environ["MEVI_RQINDEX_TRAIN_BEAM"] = "5"
            stats5 = {}
            book5, t5 = clock(lambda: rqindex.train_codebook(docs, list_of, cent, M, nbits, stats=stats5))
            del os.environ["MEVI_RQINDEX_TRAIN_BEAM"]
            for name, bk, t, st in (("greedy", book, t_train, stats), ("beam5", book5, t5, stats5)):
                if name == "greedy" and greedy5 is not None:     # measured above: the same codebook, the same beam
                    emit({"part": "train", "trainer": name, "encode_beam": 5, "train_last_level_mse": st["level_mse"][-1], "beam_mse": None,
                          **{k: v for k, v in greedy5.items() if k not in ("part", "beam")}})
                    continue
                index, t_add = clock(lambda: rqindex.RQIndex(docs, nlist, M, nbits, centroids=cent, codebook=bk, beam=5))
                row = {"part": "train", "index": shape, "trainer": name, "encode_beam": 5, "train_codebook_s": t, "add_s": t_add,
                       "train_last_level_mse": st["level_mse"][-1], "beam_mse": st.get("beam_mse"), "code_mse": index.encode_stats["code_mse"]}
                row.update(measure(index, docs, q, exact))
                emit(row)
                del index
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
