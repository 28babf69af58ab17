"""--query_encoder nci on the host: the eval driver's flag checks, and the numpy restatement of T5FineTuner.clus_repr
(tests/qemb_ref.py) against the reference's own query embeddings (goldens G1Q, tools/capture_goldens_qemb.py)."""
import glob
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import qemb_ref  # noqa: E402
from test_host_cpu import EVAL_ARGV  # noqa: E402

QTOWERS = ("enc_dec", "encmask_dec", "encmask", "dec", "encmask_dec_emb", "enc_dec_emb")
ACCUMS = ("maxpool", "avgpool", "attenpool")
G1Q = sorted(glob.glob(os.path.join(GOLD, "g1q_*.npz")))

# marco_eval_nci_rq.sh with --query_encoder nci: --save_hard_neg must go (the reference asserts twin for it)
NCI_ARGV = EVAL_ARGV + ["--query_encoder", "nci", "--save_hard_neg", "0"]


def _nci_argv(*extra, drop=()):
    argv = list(NCI_ARGV)
    for flag in drop:
        i = argv.index(flag)
        del argv[i:i + 2]
    return argv + list(extra)


def test_check_supported_accepts_query_encoder_nci():
    import main

    # attenpool reads its projection from a whole-model checkpoint
    a = main.parsers_parser(_nci_argv("--infer_ckpt", "D/ckpts/whole.ckpt"))
    main.check_supported(a)
    assert a.query_encoder == "nci" and a.qtower == "encmask_dec" and a.query_embed_accum == "attenpool"
    assert not any(f in ("--qtower", "--query_embed_accum") for f, _ in a.ignored_flags)
    # the reference's defaults enc_dec / maxpool with the NCI checkpoint alone
    d = main.parsers_parser(_nci_argv(drop=("--qtower", "--query_embed_accum")))
    main.check_supported(d)
    assert (d.qtower, d.query_embed_accum) == ("enc_dec", "maxpool")
    for qt in ("enc", "encmask", "dec", "emb", "dec_emb", "encmask_dec_emb", "enc_dec_emb", "dec_encmask"):
        for acc in ("maxpool", "avgpool", "AttenPool"):
            main.check_supported(main.parsers_parser(_nci_argv("--qtower", qt, "--query_embed_accum", acc,
                                                               "--infer_ckpt", "w.ckpt")))
    # twin runs keep ignoring both flags
    t = main.parsers_parser(EVAL_ARGV)
    main.check_supported(t)
    assert ("--qtower", "encmask_dec") in t.ignored_flags


@pytest.mark.parametrize("extra, word", [
    (["--qtower", "ori_dec", "--infer_ckpt", "w.ckpt"], "reserve_decoder"),
    (["--qtower", "enc_decx", "--infer_ckpt", "w.ckpt"], "--qtower"),
    (["--query_embed_accum", "sumpool", "--infer_ckpt", "w.ckpt"], "--query_embed_accum"),
    (["--save_hard_neg", "5", "--infer_ckpt", "w.ckpt"], "--save_hard_neg"),
    (["--eval_all_documents", "1", "--recall_level", "fine", "--knn_topk_by_step", "1", "--infer_ckpt", "w.ckpt"],
     "--eval_all_documents"),
    (["--query_embedding_path", "q.bin", "--infer_ckpt", "w.ckpt"], "--query_embedding_path"),
    ([], "--infer_ckpt"),              # attenpool with --nci_ckpt only: an untrained projection
    (["--query_encoder", "bm25"], "--query_encoder"),
])
def test_check_supported_refuses_what_nci_cannot_run(extra, word):
    import main

    with pytest.raises(SystemExit, match=word):
        main.check_supported(main.parsers_parser(_nci_argv(*extra)))


def test_golden_cases_exist():
    assert len(G1Q) >= 3
    for p in G1Q:
        g, w = qemb_ref.load_golden(p)
        assert any(k.startswith("w.") for k in w.files) and np.array_equal(g["decoded"], w["decoded"])
        assert all(f"qemb_{qt}_{acc}" in g.files for qt in QTOWERS for acc in ACCUMS)
        assert (g["attention_mask"] == 0).any()
        R = json.loads(str(g["cfg"]))["beams"]
        M = json.loads(str(g["cfg"]))["M"]
        pre, post = g["presort_prefix"].reshape(-1, R, M + 1), g["decoded"][:, :M + 1].reshape(-1, R, M + 1)
        assert (pre != post).any(), "the golden must contain a query whose final sort moves its beams"
        # the same beams, only reordered
        for a_, b_ in zip(pre, post):
            assert sorted(map(tuple, a_)) == sorted(map(tuple, b_))


@pytest.mark.parametrize("path", G1Q, ids=[os.path.basename(p)[:-4] for p in G1Q])
@pytest.mark.parametrize("qtower", QTOWERS)
@pytest.mark.parametrize("accum", ACCUMS)
def test_numpy_clus_repr_matches_the_reference(path, qtower, accum):
    g, w = qemb_ref.load_golden(path)
    R = json.loads(str(g["cfg"]))["beams"]
    emb = w["w.decode_embeddings.weight"][g["decoded"][:, -2]]
    got = qemb_ref.clus_repr(qtower, accum, g["enc_hidden"], g["attention_mask"], g["dec_hidden"], emb, R,
                             g["attenpool_weight"], g["attenpool_bias"][0])
    ref = g[f"qemb_{qtower}_{accum}"]
    if accum == "maxpool":
        assert np.array_equal(got, ref)
    else:
        assert np.abs(got - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max())
        exact, bound = qemb_ref.exact_and_bound(qtower, accum, g["enc_hidden"], g["attention_mask"], g["dec_hidden"], emb, R,
                                                g["attenpool_weight"], g["attenpool_bias"][0])
        assert np.all(np.abs(ref - exact) <= bound), "the reference's own f32 result lies inside the stated bound"
