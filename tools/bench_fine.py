"""The device fine stage (`FineStage.topk`, `FineStage.topk_graph`: mevi_fine_topk_f32) against `FineStage.rerank` on one MI355X.

Index: the bench's synthetic corpus (bench.gen_shard) under a TRAINED RQ codebook, built as tools/chain_c4.run builds it with
codebook='trained' (residual k-means on a strided 1 M-row sample, rq_encode, ClusterIndex.from_codes).  Every query's beam is
R = 10 distinct clusters of the index drawn uniformly, so a query has ~10 N / clusters candidates, the chain's figure.

    1 / 8 / 32 queries    topk eager and topk_graph against rerank
    6980 queries          topk against rerank
    k = 100 and 1000

Both paths run in ONE process, alternating window by window; a window is `calls` calls with the device synchronised before and
after; the figure is the median of `--windows` windows after a warm-up window of each path.  `rerank` gets the beam codes as the
host array the chain hands it, `topk` as the device tensor it is built for.  Before anything is timed the first k entries of
every one of rerank's lists (and its ndoc) are compared with topk's rows bit for bit.

    python tools/bench_fine.py [--docs N] [--windows 5] [--out profiles/fine_topk.json]

`--agg` measures the modes of mevi_fine_topk_agg_f32 instead (same corpus, codebook, windows and medians; default output
profiles/fine_topk_agg.json), `rerank` with the same arguments against `topk` / `topk_graph`:

    merge_add_c3           aggregate='add' on the multi-cluster index of C = 3 (pq.get_topk_document_mapping ->
                           ClusterIndex.from_topk_labels: every document in the clusters of its 3 best code paths)
    weights                beam_weights alone (log-probabilities) on the single-cluster index
    merge_add_c3_weights   both together
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
from mevi_amd import fine, ops, rq  # noqa: E402

bench.late_imports()          # bench.py binds torch / numpy lazily: its corpus generator needs them

M, K, R = 4, 32, 10
FLT_MAX = float(np.finfo(np.float32).max)


def build_stage(n_docs, dev, multi=0):
    """The single-cluster stage and its setup times; with `multi` = C also the stage over the multi-cluster index of C."""
    docs = bench.gen_shard(0, n_docs, dev, n_docs)
    step = max(1, n_docs // 1_000_000)
    t_train, (codebook, _) = sync_time(lambda: rq.train_rq_codebook(docs[::step][:1_000_000].contiguous(), M, K, seed=1, n_init=3,
                                                                    max_iter=40))
    t_enc, codes = sync_time(lambda: rq.rq_encode(docs, codebook))
    index = rq.ClusterIndex.from_codes(codes.cpu().numpy(), K)
    setup = {"train_codebook_s": round(t_train, 2), "rq_encode_ms": round(t_enc * 1e3, 1)}
    if not multi:
        return fine.FineStage(docs, index), setup
    pq = rq.ProductQuantization("rq", M, int(np.log2(K)), emb_size=docs.shape[1], device=dev)
    pq.load_codebook(codebook)
    t_topk, labels = sync_time(lambda: pq.get_topk_document_mapping(docs, 0, 1, multi))
    setup["topk_document_mapping_s"] = round(t_topk, 2)
    return fine.FineStage(docs, index), fine.FineStage(docs, rq.ClusterIndex.from_topk_labels(labels.numpy(), K)), setup


def draw(stage, nq, rng, dev):
    """(query embeddings, beam codes as a host array, the same codes on the device)."""
    keys = stage.index.keys
    picked = keys[np.stack([rng.choice(len(keys), size=R, replace=False) for _ in range(nq)])]
    codes = np.stack([picked // K ** (M - 1 - j) % K for j in range(M)], axis=-1).astype(np.int64)
    g = torch.Generator(device=dev).manual_seed(int(rng.integers(1 << 30)))
    q = (0.05 * torch.randn((nq, bench.DIM), device=dev, generator=g) + 0.02).contiguous()
    return q, codes, torch.from_numpy(codes).to(dev)


def identical(lists, ndoc, got, k):
    """rerank's lists cut to k against topk's rows: ids, score bits, ndoc (and, after a merge, the unique count against the
    list's length); returns the number of rows that differ."""
    s, i, n = (t.cpu().numpy() for t in got[:3])
    if len(got) == 4 and got[3] is not None:
        n = np.where(got[3].cpu().numpy() == np.array([len(ids) for ids, _ in lists]), n, -1)     # a wrong count fails ndoc's check
    bad = 0
    for b, (ids, sc) in enumerate(lists):
        m = min(k, len(ids))
        ok = (np.array_equal(i[b, :m], ids[:m]) and np.array_equal(s[b, :m].view(np.uint32), np.asarray(sc[:m], np.float32).view(np.uint32))
              and (i[b, m:] == -1).all() and (s[b, m:] == -FLT_MAX).all() and int(n[b]) == int(ndoc[b]))
        bad += not ok
    return bad


def windows(paths, calls, n_windows):
    """{name: median ms per call}: one warm-up window of every path, then n_windows rounds that run the paths in turn."""
    for fn in paths.values():
        sync_time(lambda: [fn() for _ in range(calls)])
    ms = {name: [] for name in paths}
    for _ in range(n_windows):
        for name, fn in paths.items():
            ms[name].append(sync_time(lambda: [fn() for _ in range(calls)])[0] * 1e3 / calls)
    return {name: round(float(np.median(v)), 4) for name, v in ms.items()}, {name: [round(x, 4) for x in v] for name, v in ms.items()}


C_MULTI = 3


def main_agg(args):
    """The merge and weight modes: rerank(...) against topk(...) / topk_graph(...) with the same arguments."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    single, multi, setup = build_stage(args.docs, dev, multi=C_MULTI)
    modes = (("merge_add_c3", multi, "add", False), ("weights", single, None, True), ("merge_add_c3_weights", multi, "add", True))
    rec = {"workload": f"fine stage, merge and weight modes: corpus {args.docs} x {bench.DIM}, trained RQ ({M},{K}) codebook, R = {R} "
                       f"distinct clusters per query; the multi-cluster index lists every document in the clusters of its {C_MULTI} best "
                       "code paths",
           "statistic": f"median of {args.windows} windows per path after one warm-up window, paths alternating, device synchronised "
                        "around each window; ms per call", "setup": setup, "index": {}, "rows": []}
    for name, stage in (("single", single), ("multi", multi)):
        sizes = np.diff(stage.index.offsets)
        rec["index"][name] = {"clusters": len(sizes), "mean": round(float(sizes.mean()), 2), "max": int(sizes.max()),
                              "max_cand": stage.max_candidates(R)}
    for nq, calls in ((1, 50), (8, 50), (32, 30), (6980, 2)):
        draws = {id(stage): draw(stage, nq, rng, dev) for stage in (single, multi)}
        w = torch.log(torch.rand((nq, R), device=dev, generator=torch.Generator(device=dev).manual_seed(nq)) * 0.9 + 0.05)
        for mode, stage, aggregate, weighted in modes:
            q, codes_h, codes_d = draws[id(stage)]
            kw = dict(aggregate=aggregate, beam_weights=w if weighted else None)
            for k in (100, 1000):
                lists, ndoc = stage.rerank(q, codes_h, **kw)
                row = {"mode": mode, "queries": nq, "k": k, "calls_per_window": calls, "candidates_per_query": float(np.mean(ndoc)),
                       "candidates_max": int(np.max(ndoc)), "listed_per_query": float(np.mean([len(ids) for ids, _ in lists])),
                       "rows_differing_topk": identical(lists, ndoc, stage.topk(q, codes_d, k, **kw), k)}
                paths = {"rerank": lambda: stage.rerank(q, codes_h, **kw), "topk": lambda: stage.topk(q, codes_d, k, **kw)}
                if nq <= fine.TOPK_GRAPH_MAX_QUERIES:
                    graph = stage.topk_graph(nq, R, k, aggregate=aggregate, weighted=weighted)
                    keys_d = stage.beam_keys(codes_d)
                    row["rows_differing_topk_graph"] = identical(lists, ndoc, graph.run(q, keys_d, kw["beam_weights"]), k)
                    paths["topk_graph"] = lambda: graph.run(q, keys_d, kw["beam_weights"])
                row["ms"], row["ms_windows"] = windows(paths, calls, args.windows)
                row["rerank_over_topk"] = round(row["ms"]["rerank"] / row["ms"]["topk"], 2)
                print(json.dumps(row), flush=True)
                rec["rows"].append(row)
    rec["all_rows_identical"] = all(r["rows_differing_topk"] == 0 and r.get("rows_differing_topk_graph", 0) == 0 for r in rec["rows"])
    rec["topk_no_slower_than_rerank_in_every_row"] = all(r["ms"]["topk"] <= r["ms"]["rerank"] for r in rec["rows"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({"all_rows_identical": rec["all_rows_identical"],
                      "topk_no_slower_than_rerank_in_every_row": rec["topk_no_slower_than_rerank_in_every_row"], "out": args.out}))
    return 0 if rec["all_rows_identical"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=bench.N_DOCS)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--agg", action="store_true", help="the merge and weight modes of mevi_fine_topk_agg_f32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.windows >= 3
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "fine_topk_agg.json" if args.agg else "fine_topk.json")
    if args.agg:
        return main_agg(args)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    stage, setup = build_stage(args.docs, dev)
    sizes = np.diff(stage.index.offsets)
    rec = {"workload": f"fine stage: corpus {args.docs} x {bench.DIM}, trained RQ ({M},{K}) codebook, {len(sizes)} clusters (mean "
                       f"{sizes.mean():.2f}, max {int(sizes.max())} documents), R = {R} distinct clusters per query",
           "statistic": f"median of {args.windows} windows per path after one warm-up window, paths alternating, device synchronised "
                        "around each window; ms per call", "setup": setup, "max_cand": stage.max_candidates(R), "rows": []}
    for nq, calls in ((1, 50), (8, 50), (32, 30), (6980, 2)):
        q, codes_h, codes_d = draw(stage, nq, rng, dev)
        for k in (100, 1000):
            lists, ndoc = stage.rerank(q, codes_h)
            row = {"queries": nq, "k": k, "calls_per_window": calls, "candidates_per_query": float(np.mean(ndoc)),
                   "candidates_max": int(np.max(ndoc)), "query_tile": ops.fine_topk_query_tile(nq, R, k, bench.DIM, rec["max_cand"]),
                   "rows_differing_topk": identical(lists, ndoc, stage.topk(q, codes_d, k), k)}
            paths = {"rerank": lambda: stage.rerank(q, codes_h), "topk": lambda: stage.topk(q, codes_d, k)}
            if nq <= fine.TOPK_GRAPH_MAX_QUERIES:
                graph = stage.topk_graph(nq, R, k)
                keys_d = stage.beam_keys(codes_d)
                row["rows_differing_topk_graph"] = identical(lists, ndoc, graph.run(q, keys_d), k)
                paths["topk_graph"] = lambda: graph.run(q, keys_d)
            row["ms"], row["ms_windows"] = windows(paths, calls, args.windows)
            row["rerank_over_topk"] = round(row["ms"]["rerank"] / row["ms"]["topk"], 2)
            gathered = float(np.sum(ndoc)) * bench.DIM * 4
            row["topk_gathered_TB_per_s"] = round(gathered / (row["ms"]["topk"] * 1e-3) / 1e12, 3)
            print(json.dumps(row), flush=True)
            rec["rows"].append(row)
    rec["all_rows_identical"] = all(r["rows_differing_topk"] == 0 and r.get("rows_differing_topk_graph", 0) == 0 for r in rec["rows"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({"all_rows_identical": rec["all_rows_identical"], "out": args.out}))
    return 0 if rec["all_rows_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
