"""--query_encoder nci on the MI355X: generate(output_dec_hidden=True) and the pool kernel mevi_query_pool_f32 against
the reference's goldens (G1Q), the kernel's stated bounds on random and strained inputs, and the eval driver end to end
against a restatement from the oracle pieces."""
import glob
import json
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import qemb_ref  # noqa: E402
from oracle import t5 as ot5  # noqa: E402

pytestmark = pytest.mark.gpu
QTOWERS = ("enc_dec", "encmask_dec", "encmask", "dec", "encmask_dec_emb", "enc_dec_emb")
ACCUMS = ("maxpool", "avgpool", "attenpool")
G1Q = sorted(glob.glob(os.path.join(GOLD, "g1q_*.npz")))
IDS = [os.path.basename(p)[:-4] for p in G1Q]


def _model(g, w, cuda):
    from mevi_amd import nci

    cfg = json.loads(str(g["cfg"]))
    R = cfg.pop("beams")
    model = nci.NCIModel(nci.load_npz_weights(w), device=cuda, **cfg)
    tree = nci.PrefixTree(g["paths"], cfg["M"], cfg["K"], cuda) if "paths" in g.files else None
    return model, tree, cfg, R


@pytest.mark.parametrize("path", G1Q, ids=IDS)
def test_dec_hidden_matches_the_reference_in_its_row_order(cuda, path):
    g, w = qemb_ref.load_golden(path)
    model, tree, cfg, R = _model(g, w, cuda)
    ids, mask = torch.from_numpy(g["input_ids"]), torch.from_numpy(g["attention_mask"])
    plain = model.generate(ids, mask, num_beams=R, decode_tree=tree)
    assert plain[3] is None
    for graph in (False, True, True):           # graph: the first call runs eagerly, the second captures and replays
        dec, scores, enc, dh = model.generate(ids, mask, num_beams=R, decode_tree=tree, graph=graph, output_dec_hidden=True)
        assert np.array_equal(dec.cpu().numpy(), g["decoded"])
        assert torch.equal(dec, plain[0]) and scores == plain[1]       # the flag changes no existing output
        got = dh.dense().cpu().numpy()
        assert got.shape == g["dec_hidden"].shape
        assert np.abs(got - g["dec_hidden"]).max() <= 5e-5, (graph, float(np.abs(got - g["dec_hidden"]).max()))


def test_generate_without_the_flag_is_unchanged(cuda):
    """the default path returns what it returned before: G1's goldens bit for bit on tokens, slot 4 None."""
    from mevi_amd import nci

    for path in sorted(glob.glob(os.path.join(GOLD, "g1_nci_*.npz"))):
        g = np.load(path)
        cfg = json.loads(str(g["cfg"]))
        R = cfg.pop("beams")
        model = nci.NCIModel(nci.load_npz_weights(g), device=cuda, **cfg)
        out = model.generate(torch.from_numpy(g["input_ids"]), torch.from_numpy(g["attention_mask"]), num_beams=R)
        assert np.array_equal(out[0].cpu().numpy(), g["decoded"]) and out[3] is None
        assert np.abs(np.array(out[1]) - g["scores"]).max() <= 1e-5


def _pool(qtower, accum, R, enc, mask, dec, emb_ids, emb_table, w=None, b=0.0):
    """ops.query_pool on host arrays; dec f32 [B*R, T, d] is laid out as per-step rows with an identity ancestor table."""
    from mevi_amd import ops

    dev = torch.device("cuda")
    steps = anc = None
    if dec is not None:
        n, T, d = dec.shape
        steps = torch.from_numpy(np.ascontiguousarray(dec.transpose(1, 0, 2))).to(dev)
        anc = torch.arange(n, dtype=torch.int32, device=dev)[:, None].repeat(1, T).contiguous()
    out = ops.query_pool(ops.qpool_mode(qtower, accum), R, enc=torch.from_numpy(enc).to(dev), mask=torch.from_numpy(mask),
                         dec=None if dec is None else (steps, anc), emb_ids=torch.from_numpy(emb_ids),
                         emb_table=torch.from_numpy(emb_table).to(dev),
                         atten_w=None if w is None else torch.from_numpy(np.asarray(w, np.float32)).to(dev), atten_b=b)
    return out.cpu().numpy()


@pytest.mark.parametrize("path", G1Q, ids=IDS)
def test_query_pool_matches_the_reference(cuda, path):
    g, w = qemb_ref.load_golden(path)
    R = json.loads(str(g["cfg"]))["beams"]
    tab = w["w.decode_embeddings.weight"]
    for qt in QTOWERS:
        for acc in ACCUMS:
            got = _pool(qt, acc, R, g["enc_hidden"], g["attention_mask"], g["dec_hidden"], g["decoded"][:, -2], tab,
                        g["attenpool_weight"], float(g["attenpool_bias"][0]))
            ref = g[f"qemb_{qt}_{acc}"]
            assert np.abs(got - ref).max() <= 5e-5, (qt, acc, float(np.abs(got - ref).max()))


def _check_bounds(qt, acc, R, enc, mask, dec, ids, tab, w, b):
    got = _pool(qt, acc, R, enc, mask, dec, ids, tab, w, b)
    emb = tab[ids]
    if acc == "maxpool":
        ref = qemb_ref.clus_repr(qt, acc, enc, mask, dec, emb, R)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (qt, "maxpool must be bit-identical")
    else:
        exact, bound = qemb_ref.exact_and_bound(qt, acc, enc, mask, dec, emb, R, w, b)
        err = np.abs(got.astype(np.float64) - exact)
        assert np.all(err <= bound), (qt, acc, float((err / bound).max()))


def _inputs(rng, B, S, R, T, d, V=50, lens=None):
    enc = rng.standard_normal((B, S, d)).astype(np.float32)
    mask = np.zeros((B, S), np.int64)
    for q in range(B):
        mask[q, :(lens[q] if lens is not None else rng.integers(1, S + 1))] = 1
    dec = rng.standard_normal((B * R, T, d)).astype(np.float32)
    tab = rng.standard_normal((V, d)).astype(np.float32)
    ids = rng.integers(0, V, B * R).astype(np.int64)
    w = (rng.standard_normal(d) * 0.5).astype(np.float32)
    return enc, mask, dec, ids, tab, w, 0.25


@pytest.mark.parametrize("qt", QTOWERS + ("enc", "emb", "dec_emb"))
@pytest.mark.parametrize("acc", ACCUMS)
def test_query_pool_bounds_on_random_inputs(cuda, qt, acc):
    rng = np.random.default_rng(hash((qt, acc)) % 1000)
    for (B, S, R, T, d) in [(3, 32, 10, 5, 64), (2, 7, 4, 4, 36), (1, 1, 1, 1, 4), (5, 20, 3, 9, 132)]:
        _check_bounds(qt, acc, R, *_inputs(rng, B, S, R, T, d))


@pytest.mark.parametrize("acc", ACCUMS)
def test_query_pool_bounds_on_strained_inputs(cuda, acc):
    rng = np.random.default_rng(7)
    # one valid token per query
    enc, mask, dec, ids, tab, w, b = _inputs(rng, 4, 32, 10, 5, 64, lens=[1, 1, 1, 1])
    for qt in ("encmask", "encmask_dec", "encmask_dec_emb"):
        _check_bounds(qt, acc, 10, enc, mask, dec, ids, tab, w, b)
    # pad rows holding the maximum: plain enc must pool them, encmask must not
    enc2 = enc.copy()
    enc2[:, 1:] = np.abs(enc2[:, 1:]) + 50.0
    for qt in ("enc_dec", "encmask_dec", "enc"):
        _check_bounds(qt, acc, 10, enc2, mask, dec, ids, tab, w, b)
    # all-negative valid rows (encmask maxpool: the max is negative, the padded rows' 0 * h must not win)
    enc3 = -np.abs(enc) - 1.0
    dec3 = -np.abs(dec) - 1.0
    for qt in ("encmask", "encmask_dec"):
        _check_bounds(qt, acc, 10, enc3, mask, dec3, ids, tab, w, b)
    # large scores: attenpool must rescale the encoder's partial softmax to each beam's running maximum
    w4 = w * 40.0
    _check_bounds("encmask_dec_emb", acc, 10, enc, np.ones_like(mask), dec, ids, tab, w4, b)


def test_query_pool_at_the_envelope(cuda):
    """d = 768, S = 512, R = 64, T = 9 (the LDS tables at their largest)."""
    rng = np.random.default_rng(11)
    enc, mask, dec, ids, tab, w, b = _inputs(rng, 2, 512, 64, 9, 768)
    w = w / 8
    for acc in ACCUMS:
        for qt in ("encmask_dec_emb", "enc_dec"):
            _check_bounds(qt, acc, 64, enc, mask, dec, ids, tab, w, b)


def test_query_pool_refuses_outside_its_envelope(cuda):
    from mevi_amd import hip, ops

    e = torch.zeros((1, 513, 8), device=cuda)
    with pytest.raises(hip.MeviHipError):
        ops.query_pool(ops.qpool_mode("enc", "maxpool"), 1, enc=e)
    with pytest.raises(ValueError):
        ops.qpool_mode("ori_dec", "maxpool")


# ---------------------------------------------------------------- the eval driver end to end
def _presort_generate(W, cfg, ids, mask, beams, length_penalty=0.8):
    """oracle.t5.nci_generate, keeping the beams in the order they enter the final step: (post-sort decoded, pre-sort
    prefixes i64 [B*R, M+1])."""
    M, K = cfg["M"], cfg["K"]
    enc = ot5.encoder(W, cfg, ids, mask)
    out, pre = [], []
    for b in range(ids.shape[0]):
        e, m = enc[b:b + 1], mask[b:b + 1]
        prefix, score = torch.zeros((1, 1), dtype=torch.long), torch.zeros(1)
        for p in range(M):
            n = prefix.shape[0]
            logits = ot5.nci_last_logits(W, cfg, prefix, e.expand(n, -1, -1), m.expand(n, -1))
            cand = (score[:, None] + F.log_softmax(logits, dim=-1)[:, 2 + p * K: 2 + (p + 1) * K]).reshape(-1)
            top = torch.topk(cand, min(beams, cand.numel()))
            prefix = torch.cat([prefix[top.indices // K], (2 + p * K + top.indices % K)[:, None]], 1)
            score = top.values
        n = prefix.shape[0]
        logits = ot5.nci_last_logits(W, cfg, prefix, e.expand(n, -1, -1), m.expand(n, -1))
        res = (score + F.log_softmax(logits, dim=-1)[:, 1]).double() / (M + 1) ** length_penalty
        order = torch.argsort(-res, stable=True)
        out.append(torch.cat([prefix[order], torch.ones((n, 1), dtype=torch.long)], 1))
        pre.append(prefix)
    return torch.cat(out), torch.cat(pre), enc


@pytest.fixture(scope="module")
def mini(tmp_path_factory):
    from test_e2e_gpu import _build_mini

    return _build_mini(tmp_path_factory.mktemp("marco_nci"), "g1_nci_M4_K32_R10.npz", 4, 5, 10)


CASES = {
    "encmask_dec-attenpool-infer_ckpt": ("encmask_dec", "attenpool", []),
    "enc_dec-maxpool-nci_ckpt": ("enc_dec", "maxpool", []),
    "encmask_dec-attenpool-doc_multiclus2": ("encmask_dec", "attenpool", ["--doc_multiclus", "2"]),
    "enc_dec-maxpool-timing_infer_step": ("enc_dec", "maxpool", ["--timing_infer_step", "100"]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_eval_driver_query_encoder_nci(cuda, mini, tmp_path, case, monkeypatch):
    import main
    from mevi_amd.evalrun import EvalRun, load_queries
    from test_e2e_gpu import FakeTokenizer

    qtower, accum, extra = CASES[case]
    a0 = mini["args"]
    d = mini["W"]["shared.weight"].shape[1]
    rng = np.random.default_rng(3)
    aw = torch.from_numpy((rng.standard_normal((1, d)) * 2.0).astype(np.float32))
    ab = torch.tensor([0.1])
    ckpt = ["--nci_ckpt", a0.nci_ckpt]
    if accum == "attenpool":
        whole = {"model." + k: v for k, v in mini["W"].items()}
        whole["pq.codebook"] = torch.from_numpy(mini["C"])
        whole["attenpool_weight.weight"], whole["attenpool_weight.bias"] = aw, ab
        torch.save({"state_dict": whole}, tmp_path / "whole.ckpt")
        ckpt = ["--infer_ckpt", str(tmp_path / "whole.ckpt")]
    argv = ["--mode", "eval", "--dataset", "marco", "--document_encoder", "ance", "--recall_level", "both", "--codebook", "1",
            "--pq_type", "rq", "--subvector_num", "4", "--subvector_bits", "5", "--num_return_sequences", "10",
            "--adaptor_layer_num", "2", "--eval_batch_size", "4", "--query_encoder", "nci", "--qtower", qtower,
            "--query_embed_accum", accum, "--data_dir", a0.data_dir, "--ckpt_dir", a0.ckpt_dir,
            "--embedding_path", a0.embedding_path, "--pq_path", a0.pq_path, "--pq_cluster_path", a0.pq_cluster_path,
            "--custom_save_path", str(tmp_path / "out.tsv")] + ckpt + extra
    a = main.parsers_parser(argv)
    main.check_supported(a)
    a.metric_path = str(tmp_path / "m.txt")
    monkeypatch.chdir(tmp_path)
    run = EvalRun(a, tokenizer=FakeTokenizer(512), device=cuda)
    assert run.tower is None
    run.run(load_queries(a.data_dir))
    coarse = [l.rstrip("\n").split("\t") for l in open(tmp_path / "out_coarse.tsv")]
    fine = [l.rstrip("\n").split("\t") for l in open(tmp_path / "out_fine.tsv")]
    assert os.path.getsize(a.metric_path) > 0
    # ---- restatement: oracle beam search, reference decoder states in pre-sort order, numpy clus_repr, f64 dots
    R, M, K = 10, 4, 32
    enc_t = FakeTokenizer(512).batch_encode_plus(mini["queries"])
    ids, mask = enc_t["input_ids"], enc_t["attention_mask"]
    dec, pre, enc = _presort_generate(mini["W"], mini["cfg"], ids, mask, R)
    B = ids.shape[0]
    dh = torch.cat([ot5.decoder(mini["W"], mini["cfg"], pre[q * R:(q + 1) * R], enc[q:q + 1].expand(R, -1, -1),
                                mask[q:q + 1].expand(R, -1)) for q in range(B)]).numpy()
    emb_rows = mini["W"]["decode_embeddings.weight"].numpy()[dec[:, -2].numpy()]
    qemb = qemb_ref.clus_repr(qtower, accum, enc.numpy(), mask.numpy(), dh, emb_rows, R, aw.numpy(), float(ab[0]))
    codes = ot5.decode_token(dec, K).view(B, R, M).numpy()
    E = mini["emb"].astype(np.float64)
    nd = 0
    for i, q in enumerate(mini["queries"]):
        assert coarse[i][0] == fine[i][0] == q
        assert eval(coarse[i][1]) == codes[i].tolist()
        occ = [(doc, float(E[doc] @ qemb[i * R + j].astype(np.float64)))
               for j, c in enumerate(codes[i].tolist()) for doc in run.index.lookup(c).tolist()]
        if run.aggregate is None:
            ids_, ref = [o[0] for o in occ], np.array([o[1] for o in occ])
        else:       # --doc_multiclus: one entry per document, its per-beam scores summed (or their maximum)
            acc = {}
            for doc, s_ in occ:
                acc[doc] = acc.get(doc, 0.0) + s_ if run.aggregate == "add" else max(acc.get(doc, -np.inf), s_)
            ids_, ref = list(acc), np.array(list(acc.values()))
        got = eval(fine[i][1])
        assert sorted(got) == sorted(ids_)
        nd += len(got)
        if len(ids_):
            order = np.argsort(-ref, kind="stable")
            gaps = np.abs(np.diff(ref[order]))
            firm = np.concatenate([[True], gaps > 1e-3]) & np.concatenate([gaps > 1e-3, [True]])
            assert all(got[k] == ids_[order[k]] for k in np.nonzero(firm)[0]), (case, i)
    assert nd > 50
