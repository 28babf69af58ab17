"""The NCI baseline end to end -- `main.py --mode eval` without --document_encoder -- on a miniature corpus: EvalRun from
the argv against a host restatement.  The beams come from tests/varbeam_ref.py driven by the torch-fp32 oracle model
(`oracle_search`, as the base-shape test of test_varbeam_gpu.py), cut at eos; the ranks are the reference's `d.index(gt)`
over the gt ids cut to max_output_length - 2 codes (MEVI/main_models.py:815-831, 3722-3780); the figures those of
handle_infer_results with `length is None` (:4100-4201).  Beams may differ from the restatement's only by swaps inside a
near-tie (oracle score gap < 4e-4, `near_tie_swaps`), at most 1 % of them, scores within 2e-4: the bounds of that test."""
import os
import pickle

import numpy as np
import pytest
import torch

import varbeam_ref as vr
from test_e2e_gpu import FakeTokenizer

pytestmark = pytest.mark.gpu
K, R, CUT, SEED = 6, 40, 8, 0
TOL_TIE, TOL_SCORE = 4e-4, 2e-4


def pure_case(seed=SEED):
    """Seeded weights (d 64, two 64-wide heads, two layers each), 300 documents with ids of 2 .. 10 codes over K = 6 (every
    fifth document repeats an earlier id; ids longer than 8 codes collide after the cut), 12 queries."""
    from test_t5_gpu import _seeded_nci_weights

    torch.manual_seed(seed)
    W, cfg = _seeded_nci_weights(CUT, K, 64, 128, 2)
    rng = np.random.default_rng(seed)
    ids = []
    for doc in range(300):
        if doc % 5 == 4:
            ids.append(ids[int(rng.integers(0, doc))])
        else:
            n = int(rng.integers(2, 11))
            ids.append(tuple(int(c) for c in rng.integers(0, K, size=2)) + tuple(int(c) for c in rng.integers(0, 3, size=n - 2)))
    mapping = {doc: "-".join(map(str, c)) if doc % 2 else tuple(c) for doc, c in enumerate(ids)}
    queries = [" ".join(f"w{rng.integers(0, 50)}" for _ in range(rng.integers(3, 12))) + f" q{i}" for i in range(12)]
    gts = [[int(x) for x in rng.choice(300, size=1 + i % 3, replace=False)] for i in range(len(queries))]
    return W, cfg, ids, mapping, queries, gts


def restated_beams(W, cfg, ids, queries, dtype=np.float32):
    enc = FakeTokenizer(1000).batch_encode_plus(queries)
    paths = sorted({c[:CUT] for c in ids})
    return vr.oracle_search(W, cfg, enc["input_ids"], enc["attention_mask"], R, paths, dtype=dtype)


def beam_lists(decoded):
    """Token rows -> code lists cut at eos (decode_token + `dd[0:ii]`, MEVI/main_models.py:117-136, 3722-3726)."""
    out = []
    for row in decoded:
        eos = list(row).index(1)
        out.append([int(t) - 2 - p * K for p, t in enumerate(row[1:eos])])
    return out


@pytest.fixture(scope="module")
def pure(tmp_path_factory):
    d = tmp_path_factory.mktemp("pure_nci")
    W, cfg, ids, mapping, queries, gts = pure_case()
    want, want_s, want_l = restated_beams(W, cfg, ids, queries)
    d64, s64, _ = restated_beams(W, cfg, ids, queries, dtype=np.float64)
    cap = len(want_s) // 100
    own = vr.near_tie_swaps(want, d64, s64, R, TOL_TIE)
    print("f32 vs f64 restatement: beams in a near-tie swap", own, "of", len(want_s))
    assert own <= cap                                      # the seed: the restatement's own sensitivity stays inside the cap
    # every third query gets a gt document whose cut id the restatement returns, so that the ranks are not all None
    cut = [c[:CUT] for c in ids]
    for i in range(0, len(queries), 3):
        row = want[i * R + (7 * i) % R]
        gts[i][0] = cut.index(tuple(beam_lists([row])[0]))
    os.makedirs(d / "ckpts" / "t5-ance")
    os.makedirs(d / "origin")
    os.makedirs(d / "ids")
    torch.save({"state_dict": {"model." + k: v for k, v in W.items()}}, d / "ckpts" / "nci.ckpt")
    with open(d / "ids" / "mapping.pkl", "wb") as f:
        pickle.dump(mapping, f)
    with open(d / "origin" / "dev_mevi_dedup.tsv", "w") as f:
        for q, g in zip(queries, gts):
            f.write(f"{q}\t{','.join(map(str, g))}\n")
    return dict(dir=d, ids=ids, queries=queries, gts=gts, want=want, want_s=want_s, want_l=want_l, cap=cap)


def test_pure_nci_eval_matches_the_restatement(cuda, pure, tmp_path):
    import main
    from mevi_amd.evalrun import EvalRun, load_queries

    s, d = pure, pure["dir"]
    argv = ["--mode", "eval", "--data_dir", str(d / "origin"), "--kary", str(K), "--mapping_path", str(d / "ids" / "mapping.pkl"),
            "--id_class", "bert_k30_c30_1", "--num_return_sequences", str(R), "--adaptor_layer_num", "2", "--nci_ckpt",
            str(d / "ckpts" / "nci.ckpt"), "--ckpt_dir", str(d / "ckpts"), "--custom_save_path", str(tmp_path / "res.tsv"),
            "--embedding_path", str(d / "ids" / "no_such_corpus.bin"), "--save_hard_neg", "50", "--eval_batch_size", "4",
            "--position", "1", "--tree", "1", "--query_encoder", "nci"]
    a = main.parsers_parser(argv)
    main.check_supported(a)
    assert a.recall_num == [1, 5, 10, 20] and a.label_length_cutoff == CUT and a.max_output_length == CUT + 2
    a.metric_path = str(tmp_path / "metrics.txt")
    run = EvalRun(a, tokenizer=FakeTokenizer(1000), device=cuda)
    assert run.tower is None and run.emb is None and run.fine is None and run.fine_log is None and run.hn_log is None
    out = run.run(load_queries(a.data_dir))
    prefix = a.custom_save_path[:-4]
    assert sorted(os.listdir(tmp_path)) == ["metrics.txt", "res_coarse.tsv"]          # no _fine / _hn file
    rows = [l.rstrip("\n").split("\t") for l in open(prefix + "_coarse.tsv")]
    assert len(rows) == len(s["queries"]) and all(len(r) == 4 for r in rows)
    cut = [list(c[:CUT]) for c in s["ids"]]
    want_d = beam_lists(s["want"])
    got_tok = np.zeros_like(s["want"])
    got_d, got_s, ranks = [], [], []
    for i, (text, dcol, gcol, scol) in enumerate(rows):
        beams, gt_codes, sc = eval(dcol), eval(gcol), eval(scol)
        assert text == s["queries"][i] and gt_codes == [cut[g] for g in s["gts"][i]] and len(beams) == R == len(sc)
        for j, beam in enumerate(beams):                               # back to token rows for near_tie_swaps
            got_tok[i * R + j, 1:len(beam) + 1] = [2 + p * K + c for p, c in enumerate(beam)]
            got_tok[i * R + j, len(beam) + 1] = 1
        got_d.append(beams)
        got_s.append(sc)
        ranks.append(tuple(beams.index(g) if g in beams else None for g in gt_codes))
    swapped = vr.near_tie_swaps(got_tok, s["want"], s["want_s"], R, TOL_TIE)
    diff = np.abs(np.sort(np.array(got_s), 1) - np.sort(s["want_s"].reshape(-1, R), 1)).max()
    print("driver vs restatement: beams in a near-tie swap", swapped, "of", len(s["want_s"]), "max score diff", diff,
          "lengths", np.bincount(s["want_l"]).tolist())
    assert swapped <= s["cap"] and diff <= TOL_SCORE
    if swapped == 0:
        assert [b for q in got_d for b in q] == want_d
    assert len({len(b) for b in want_d}) > 3 and any(r is not None for rk in ranks for r in rk)
    # handle_infer_results, `length is None`: per query recall = found below k / gts, mrr = 1 / (best + 1), hit = best < k
    n = len(ranks)
    for k in a.recall_num:
        rec = mrr = hit = 0.0
        for rk in ranks:
            found = [r for r in rk if r is not None]
            if found:
                rec += sum(r < k for r in found) / len(rk)
                mrr += 1 / (min(found) + 1) if min(found) < k else 0
                hit += min(found) < k
        assert out["recall"][k] == rec / n and out["mrr"][k] == mrr / n and out["hitrate"][k] == hit / n, k
    assert out["ndoc"] is None and set(out["recall"]) == {1, 5, 10, 20} and "cluster_recall" not in out
    lines = open(a.metric_path).read().splitlines()
    assert lines == [f"{name}{k} {out[name][k]}" for name in ("recall", "mrr", "hitrate") for k in a.recall_num]
