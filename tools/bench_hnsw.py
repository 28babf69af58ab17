"""HNSW<M> (faiss_search.py --param HNSW<M>, mevi_amd/hnsw.py) against the exact search at C2 size on the clustered synthetic
corpus (tools/synth.py), in one process: the build seconds per phase (kNN lists, links, entry rows, upper levels), then per entry
(strided rows / upper levels, the same level-0 graph and the same queries), per (k, efSearch, query count) the index search
(HNSWIndex.search: entry scan [+ descent] + mevi_graph_search_topk_f32) against DenseIndex.search on the same queries -- median
of 3 timed windows after a warm-up, the two taking turns (tools/bench_ivf.py: timed) --, recall against the exact lists, steps
and rows scored per query (the u32 the walk and the descent leave in their workspaces), the bytes of rows gathered per second,
and the replayed graph's latency for up to 32 queries.  Settings whose ef = max(efSearch, k) is the same run the same walk and
are measured once.  --ef-upper / --width-upper take lists: the first of each serves the whole table, the other combinations are
measured at the first (k, efSearch) only.
  python tools/bench_hnsw.py [--m 32] [--m256] [--k 10,100,1000] [--ef 16,64,256] [--nq 1,8,32,6980] [--docs N] [--width 1]
                             [--entry strided,levels] [--ef-upper 32] [--width-upper 1] [--out table.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import synth  # noqa: E402
from bench_ivf import HBM_PEAK, ints, recall, timed  # noqa: E402
from mevi_amd import dense, hnsw  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--m256", action="store_true", help="M = 256, the reference README's HNSW256")
    ap.add_argument("--k", default="10,100,1000")
    ap.add_argument("--ef", default="16,64,256")
    ap.add_argument("--nq", default=f"1,8,32,{bench.N_QUERIES}")
    ap.add_argument("--docs", type=int, default=bench.N_DOCS)
    ap.add_argument("--width", type=int, default=1)
    ap.add_argument("--entry", default="strided", help="strided, levels or both: measured in this order on one level-0 graph")
    ap.add_argument("--ef-upper", default=str(hnsw.N_SEEDS), help="list sizes of the upper levels' walks")
    ap.add_argument("--width-upper", default="1", help="widths of the upper levels' walks")
    ap.add_argument("--corpus", default="clustered", choices=synth.CORPUS_KINDS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    M = 256 if a.m256 else a.m
    entries = [e.strip() for e in a.entry.split(",")]
    assert entries and all(e in hnsw.ENTRIES for e in entries), a.entry
    dev = torch.device("cuda:0")
    docs, info = synth.corpus(a.corpus, dev, a.docs)
    dim = docs.shape[1]
    nqs, ks = ints(a.nq), ints(a.k)
    uppers = [(e, w) for e in ints(a.ef_upper) for w in ints(a.width_upper)]
    q_all = synth.corpus_queries(a.corpus, docs, max(nqs), info)[0]
    exact = dense.DenseIndex(docs)
    exact_ids = exact.search(q_all, max(ks))[1]                  # per query: the same lists whatever the batch
    build, indexes = {}, {}
    for e in entries:                                            # one level-0 graph: the second index takes the first's
        first = next(iter(indexes.values()), None)
        indexes[e] = hnsw.HNSWIndex(docs, M, knn=first and first.knn, graph=first and first.graph, timing=build, entry=e,
                                    ef_upper=uppers[0][0], width_upper=uppers[0][1])
        build[f"{e}_entry_s"] = build.pop("entry_s")
        build[f"{e}_graph_bytes"] = indexes[e].graph_bytes()
        build[f"{e}_is"] = indexes[e].entry_name()
    index = indexes[entries[0]]
    build = {k_: round(v, 2) if isinstance(v, float) else v for k_, v in build.items()}
    build.update(M=M, degree=2 * M, corpus_bytes=docs.numel() * 4, links_per_row_mean=round(float((index.graph >= 0).sum(1).float().mean()), 2))
    print(json.dumps(build), flush=True)
    rows = []

    def save():
        if a.out:                                                # after every row: a long table survives a short limit
            with open(a.out, "w") as f:
                json.dump({"docs": a.docs, "dim": dim, "corpus": a.corpus, "M": M, "width": a.width, "hbm_peak_bytes_per_s": HBM_PEAK,
                           "note": "hnsw_ms / exact_ms = the whole search of HNSWIndex.search (entry scan [+ descent] + walk) / "
                                   "DenseIndex.search, median of 3 windows after a warm-up, taking turns; rows_scored = rows whose chain the "
                                   "walk ran, per query (mean); descent_rows_scored = the same for the upper levels' descent (carried seeds "
                                   "not counted; the exhaustive scan of the top level or of the strided rows is in neither); "
                                   "gathered_bytes_per_s = (rows_scored + descent_rows_scored) * dim * 4 * nq / hnsw_ms",
                           "build": build, "rows": rows}, f, indent=1)

    def measure(index, k, ef_search, nq, upper):
        index.set_upper(*upper)
        ef, width, max_steps = index.plan(k, ef_search, a.width)
        q = q_all[:nq].contiguous()
        steps = torch.zeros(nq, dtype=torch.int32, device=dev)
        ws = torch.empty(dense.graph_search_workspace_bytes(nq, dim, 2 * M, index.walk_nseed, k, ef, width, max_steps), dtype=torch.uint8,
                         device=dev)
        levels = index.entry == "levels"
        dsteps = torch.zeros(nq, dtype=torch.int32, device=dev) if levels else None
        dws = torch.empty(dense.graph_descend_workspace_bytes(*index.descend_shape(nq)), dtype=torch.uint8, device=dev) if levels else None
        i_h = index.search(q, k, ef_search, a.width, steps=steps, workspace=ws, descent_steps=dsteps, descent_workspace=dws)[1]
        torch.cuda.synchronize()
        scored = ws[:4 * nq].view(torch.int32).double()
        dscored = dws[:4 * nq].view(torch.int32).double() if levels else torch.zeros(nq, dtype=torch.float64, device=dev)
        t_h, t_e = timed([lambda: index.search(q, k, ef_search, a.width), lambda: exact.search(q, k)])
        st = steps.double()
        row = {"entry": index.entry, "k": k, "efSearch": ef_search, "ef": ef, "nq": nq, "hnsw_ms": round(t_h * 1e3, 4),
               "exact_ms": round(t_e * 1e3, 4), "speedup": round(t_e / t_h, 2), "recall": recall(i_h, exact_ids[:nq, :k]),
               "steps_mean": round(float(st.mean()), 1), "steps_max": int(st.max()), "hit_max_steps": int((steps >= max_steps).sum()),
               "rows_scored": round(float(scored.mean()), 1),
               "gathered_bytes_per_s": round(float(scored.sum() + dscored.sum()) * dim * 4 / t_h, 0)}
        if levels:
            row.update(ef_upper=upper[0], width_upper=upper[1], descent_steps_mean=round(float(dsteps.double().mean()), 1),
                       descent_steps_max=int(dsteps.max()), descent_rows_scored=round(float(dscored.mean()), 1))
        if nq <= hnsw.GRAPH_MAX_QUERIES:
            g = index.search_graph(nq, k, ef_search, a.width)
            (t_graph,) = timed([lambda: g.run(q)])
            row["hnsw_graph_ms"] = round(t_graph * 1e3, 4)
            row["graph_same_bits"] = bool(torch.equal(g.run(q)[1], i_h))
            del g
        rows.append(row)
        print(json.dumps(row), flush=True)
        save()

    save()
    done = set()
    for k in ks:
        for ef_search in ints(a.ef):
            ef = index.plan(k, ef_search, a.width)[0]
            if (k, ef) in done:
                continue
            for nq in nqs:
                for e in entries:
                    # an index that fell back to the strided rows is measured once, as what it is
                    if indexes[e].entry != e:
                        continue
                    for upper in (uppers if not done and e == "levels" else uppers[:1]):
                        measure(indexes[e], k, ef_search, nq, upper)
            done.add((k, ef))


if __name__ == "__main__":
    main()
