"""`--codebook 0` end to end on a miniature corpus: the eval driver over semantic ids of different lengths against a
restatement of the reference's infer() written here with dicts (MEVI/main_models.py:815-825 gt codes, :1868 clusters keyed
by newid[:label_length_cutoff], :3924-3928 a beam's cluster = tuple(d[:eos_idx]), :3736-3780 coarse ranks, :4013-4053 fine
list).  The beams themselves come from generate(decode_tree=RaggedPrefixTree), the same call the driver makes: for the
beams this file covers the driver's bookkeeping only, the goldens G1V carry the search.  `_coarse.tsv` is compared byte
for byte.  `_fine.tsv` and the `_hn` file are compared as the existing e2e test compares them -- the same set of documents,
the same order wherever neighbouring scores are more than 1e-3 apart, scores within 2e-4 -- because the restatement's
query embeddings come from the CPU oracle tower and a numpy dot: the device's bits are out of reach for an independent
restatement, so byte equality of those two files cannot be asked of it."""
import json
import os
import pickle
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import t5 as ot5
from test_e2e_gpu import GOLD, FakeTokenizer

pytestmark = pytest.mark.gpu
L, K, R = 3, 16, 4


@pytest.fixture(scope="module")
def semantic(cuda, tmp_path_factory):
    d = tmp_path_factory.mktemp("semantic")
    g = np.load(os.path.join(GOLD, "g1_nci_M3_K16_R4.npz"))
    W = ot5.load_weights(g)
    tw = np.load(os.path.join(GOLD, "g2_t5_tower.npz"))
    TW, tcfg = ot5.load_weights(tw), json.loads(str(tw["cfg"]))
    os.makedirs(d / "ckpts" / "t5-ance")
    os.makedirs(d / "origin")
    os.makedirs(d / "ids")
    torch.save({"state_dict": {"model." + k: v for k, v in W.items()}}, d / "ckpts" / "nci.ckpt")
    torch.save(TW, d / "ckpts" / "t5-ance" / "pytorch_model.bin")
    json.dump(dict(d_model=32, d_ff=64, num_heads=4, d_kv=8, num_layers=2, num_decoder_layers=2),
              open(d / "ckpts" / "t5-ance" / "config.json", "w"))
    rng = np.random.default_rng(11)
    N, dim = 900, 32
    emb = rng.standard_normal((N, dim)).astype(np.float32)
    emb.tofile(d / "ids" / "docemb.bin")
    mapping = {}
    for doc in range(N):                       # ids of 1 .. 5 codes (longer than the cutoff too), strings and tuples
        codes = [int(c) for c in rng.integers(0, 5, size=int(rng.integers(1, 6)))]
        mapping[doc] = "-".join(map(str, codes)) if doc % 2 else tuple(codes)
    with open(d / "ids" / "mapping.pkl", "wb") as f:
        pickle.dump(mapping, f)
    queries = [" ".join(f"w{rng.integers(0, 50)}" for _ in range(rng.integers(3, 12))) + f" q{i}" for i in range(21)]
    gts = [[int(x) for x in rng.choice(N, size=1 + i % 2, replace=False)] for i in range(len(queries))]
    # every third query gets a gt document from a cluster its search actually returns, so that ranks are not all None
    from mevi_amd import nci

    cfg = json.loads(str(g["cfg"]))
    cfg.pop("beams")
    model = nci.NCIModel(nci.load_npz_weights(g), device=cuda, **cfg)
    cut = [tuple(int(c) for c in (v.split("-") if isinstance(v, str) else v))[:L] for v in mapping.values()]
    tree = nci.RaggedPrefixTree(cut, K, cuda, levels=L + 1)
    enc = FakeTokenizer(512).batch_encode_plus(queries)
    dec = model.generate(enc["input_ids"], enc["attention_mask"], num_beams=R, decode_tree=tree)[0].cpu().numpy()
    for i in range(0, len(queries), 3):
        row = dec[i * R + (i // 3) % R]
        beam = tuple(int(t) - 2 - p * K for p, t in enumerate(row[1:list(row).index(1)]))
        gts[i][0] = cut.index(beam)
    with open(d / "origin" / "dev_mevi_dedup.tsv", "w") as f:
        for q, g_ in zip(queries, gts):
            f.write(f"{q}\t{','.join(map(str, g_))}\n")
    return dict(dir=d, emb=emb, mapping=mapping, queries=queries, gts=gts, TW=TW, tcfg=tcfg, N=N)


def cli_args(s, tmp_path, level):
    import main

    d = s["dir"]
    argv = ["--mode", "eval", "--data_dir", str(d / "origin"), "--codebook", "0", "--label_length_cutoff", str(L), "--kary", str(K),
            "--mapping_path", str(d / "ids" / "mapping.pkl"), "--id_class", "bert_k30_c30_1", "--document_encoder", "ance",
            "--query_encoder", "twin", "--recall_level", level, "--num_return_sequences", str(R), "--adaptor_layer_num", "2",
            "--nci_ckpt", str(d / "ckpts" / "nci.ckpt"), "--ckpt_dir", str(d / "ckpts"), "--embedding_path",
            str(d / "ids" / "docemb.bin"), "--custom_save_path", str(tmp_path / f"res_{level}.tsv"), "--save_hard_neg", "50",
            "--eval_batch_size", "4", "--max_output_length", "10", "--position", "1", "--tree", "1"]
    a = main.parsers_parser(argv)
    main.check_supported(a)
    a.metric_path = str(tmp_path / f"metrics_{level}.txt")
    return a


def restated_infer(s, cuda, level):
    """(coarse file text, per query (cluster docs, query embedding)): everything after the beam search, with dicts."""
    from mevi_amd import nci

    ids_of = {doc: [int(c) for c in (v.split("-") if isinstance(v, str) else v)] for doc, v in s["mapping"].items()}
    doc_cluster = {}
    for doc in range(s["N"]):
        doc_cluster.setdefault(tuple(ids_of[doc][:L]), []).append(doc)
    g = np.load(os.path.join(GOLD, "g1_nci_M3_K16_R4.npz"))
    cfg = json.loads(str(g["cfg"]))
    cfg.pop("beams")
    model = nci.NCIModel(nci.load_npz_weights(g), device=cuda, **cfg)
    tree = nci.RaggedPrefixTree([tuple(v) for v in ids_of.values()], K, cuda, cutoff=L, levels=L + 1)
    enc = FakeTokenizer(512).batch_encode_plus(s["queries"])
    dec, scores, _, _, _ = model.generate(enc["input_ids"], enc["attention_mask"], num_beams=R, decode_tree=tree)
    dec = dec.cpu().numpy().reshape(len(s["queries"]), R, L + 2)
    scores = np.array(scores).reshape(len(s["queries"]), R)
    qemb = ot5.tower_encode(s["TW"], s["tcfg"], enc["input_ids"], enc["attention_mask"]).numpy()
    lines, per_query = [], []
    for i, q in enumerate(s["queries"]):
        d = []
        for row in dec[i]:
            eos = list(row).index(1)
            d.append([int(t) - 2 - p * K for p, t in enumerate(row[1:eos])])
        gt_codes = [ids_of[g_][:L] for g_ in s["gts"][i]]
        lines.append(f"{q}\t{d}\t{gt_codes}\t{scores[i].tolist()}\n")
        per_query.append(([doc for beam in d for doc in doc_cluster.get(tuple(beam), [])], qemb[i],
                          tuple(d.index(g_) if g_ in d else None for g_ in gt_codes)))
    return "".join(lines), per_query


@pytest.mark.parametrize("level", ["both", "coarse"])
def test_eval_driver_over_semantic_ids_matches_restated_infer(cuda, semantic, tmp_path, level):
    from mevi_amd.evalrun import EvalRun, load_queries

    s = semantic
    a = cli_args(s, tmp_path, level)
    run = EvalRun(a, tokenizer=FakeTokenizer(512), device=cuda)
    out = run.run(load_queries(a.data_dir))
    prefix = a.custom_save_path[:-4]
    want_coarse, per_query = restated_infer(s, cuda, level)
    assert open(prefix + "_coarse.tsv").read() == want_coarse                     # bytes: ragged beam lists, gt codes, scores
    lens = {len(beam) for line in want_coarse.splitlines() for beam in eval(line.split("\t")[1])}
    assert len(lens) > 1, "fixture should return beams of different lengths"
    nd = sum(len(docs) for docs, _, _ in per_query)
    assert nd > 100 and abs(out["ndoc"] - nd / len(per_query)) < 1e-9
    if level == "coarse":
        assert not os.path.exists(prefix + "_fine.tsv")
        hits = [r for _, _, ranks in per_query for r in ranks]
        assert abs(out["recall"][1] - np.mean([np.mean([r == 0 for r in ranks]) for _, _, ranks in per_query])) < 1e-12
        assert any(r is not None for r in hits)
        return
    fine = [l.rstrip("\n").split("\t") for l in open(prefix + "_fine.tsv")]
    hn = [l.rstrip("\n").split("\t") for l in open(f"{prefix}_hn{a.save_hard_neg}.tsv")]
    for i, (docs, q, _) in enumerate(per_query):
        got = eval(fine[i][1])
        assert fine[i][0] == s["queries"][i] and sorted(got) == sorted(docs) and eval(fine[i][2]) == s["gts"][i]
        if docs:
            ref = s["emb"][docs] @ q
            order = np.argsort(-ref, kind="stable")
            got_s = np.array([float(x) for x in hn[i][3].split(",")])
            assert np.abs(got_s - ref[order][:len(got_s)]).max() <= 2e-4
            gaps = np.abs(np.diff(ref[order]))
            firm = np.concatenate([[True], gaps > 1e-3]) & np.concatenate([gaps > 1e-3, [True]])
            assert all(got[j] == docs[order[j]] for j in np.nonzero(firm)[0])
    assert "ndocs@cluster4" in open(a.metric_path).read()


def test_more_beams_than_distinct_ids_is_refused(cuda, semantic, tmp_path):
    from mevi_amd.evalrun import EvalRun

    s = semantic
    a = cli_args(s, tmp_path, "both")
    few = {doc: (doc % 3,) for doc in range(s["N"])}
    with open(tmp_path / "few.pkl", "wb") as f:
        pickle.dump(few, f)
    a.mapping_path = str(tmp_path / "few.pkl")
    with pytest.raises(SystemExit, match="num_return_sequences"):
        EvalRun(a, tokenizer=FakeTokenizer(512), device=cuda)
