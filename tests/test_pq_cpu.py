"""CPU: --pq_type pq on the command line, and the product-quantisation goldens (tools/capture_goldens_pq.py) pinned to the
oracle's arithmetic -- per-slice encode, concatenated reconstruct and the 'pq' beam step restated in numpy."""
import glob
import os

import numpy as np
import pytest

import pq_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PQ_GOLDENS = sorted(glob.glob(os.path.join(GOLD, "g4p_pq_*.npz")))

EVAL = """--mode eval --dataset marco --document_encoder ance --recall_level both --codebook 1 --subvector_num 4
--subvector_bits 5 --query_encoder twin --num_return_sequences 10 --pq_path D/ance/pqcodebook4_5.pt
--pq_cluster_path D/ance/pqclus4_5.pkl --nci_ckpt D/ckpts/nci.ckpt --data_dir D/origin --ckpt_dir D/ckpts
--embedding_path D/ance/docemb.bin --custom_save_path D/ance/nci_result_pq45_top10.tsv""".split()
GEN = """--mode train --only_gen_rq 1 --codebook 1 --subvector_num 4 --subvector_bits 5 --document_encoder ance
--pq_path D/ance/pqcodebook4_5.pt --pq_cluster_path D/ance/pqclus4_5.pkl --data_dir D/origin --ckpt_dir D/ckpts
--document_path D/ance/all_document --embedding_path D/ance/docemb.bin""".split()


@pytest.mark.parametrize("argv", [EVAL, GEN], ids=["eval", "only_gen_rq"])
def test_check_supported_accepts_pq_type_pq(argv):
    import main

    for extra in (["--pq_type", "pq"], ["--pq_type", "rq"], []):   # the parser's default is 'pq' (MEVI/main.py:551)
        a = main.parsers_parser(argv + extra)
        main.check_supported(a)
        assert a.pq_type == (extra[1] if extra else "pq")
    with pytest.raises(SystemExit):           # opq: the rotation only comes from a faiss index file
        main.check_supported(main.parsers_parser(argv + ["--pq_type", "opq"]))


def test_pq_keeps_the_other_refusals():
    import main

    with pytest.raises(SystemExit):
        main.check_supported(main.parsers_parser(EVAL + ["--pq_type", "pq", "--pq_dist_mode", "ip"]))
    with pytest.raises(SystemExit):
        main.check_supported(main.parsers_parser(EVAL + ["--pq_type", "pq", "--rq_topk_score", "last"]))
    with pytest.raises(SystemExit):
        main.check_supported(main.parsers_parser(["--mode", "train", "--pq_type", "pq", "--data_dir", "x"]))


def test_goldens_cover_the_requested_shapes():
    shapes = {tuple(np.load(p)["C"].shape[:2]) + (np.load(p)["X"].shape[1],) for p in PQ_GOLDENS}
    assert {(4, 32, 64), (8, 256, 64)} <= shapes
    assert all(os.path.getsize(p) < 1 << 20 for p in PQ_GOLDENS)


@pytest.mark.parametrize("path", PQ_GOLDENS, ids=os.path.basename)
def test_goldens_pinned_by_per_slice_oracle(path):
    g = np.load(path)
    X, C = g["X"], g["C"]
    M, K, dsub = C.shape
    codes = pq_ref.pq_encode(X, C)
    assert pq_ref.codes_agree(codes, g["codes"], pq_ref.near_tie_sets(X, C))
    # the per-slice oracle is one level of the RQ oracle: a PQ code never reads columns past M * dsub
    Y = X.copy()
    Y[:, M * dsub:] = 1e30
    assert np.array_equal(pq_ref.pq_encode(Y, C), codes)
    # reconstruct = concatenation (pq.get_reconstruct_vector), bit for bit
    assert np.array_equal(pq_ref.reconstruct(g["codes"][:32], C), g["reconstruct32"])
    # cluster dict of get_document_cluster: keys sorted, documents in append order
    from oracle import rq as orq

    cluster, _ = orq.cluster_dict(g["codes"])
    keys = [tuple(k) for k in g["cluster_keys"].tolist()]
    assert sorted(cluster) == keys and [d for k in keys for d in cluster[k]] == g["cluster_docs"].tolist()
    assert [len(cluster[k]) for k in keys] == g["cluster_sizes"].tolist()


@pytest.mark.parametrize("path", PQ_GOLDENS, ids=os.path.basename)
def test_goldens_pinned_by_numpy_pq_beam_step(path):
    g = np.load(path)
    for R in (5, 10):
        lab, sc = pq_ref.beam_search(g["X"][:64], g["C"], R)
        assert pq_ref.beams_agree(lab, sc, g[f"beam{R}_labels"], g[f"beam{R}_scores"])


def test_pq_beam_step_is_not_the_rq_step():
    """The restatement scores every level on the row's own slice (no residual hand-down) and repeats it per beam."""
    g = np.load(os.path.join(GOLD, "g4p_pq_5_4_44.npz"))
    X, C = g["X"][:8], g["C"]
    lab, sc = pq_ref.beam_search(X, C, 5)
    _, nd = pq_ref.pq_encode(X, C, return_neg_dist=True)
    p = np.exp(nd - nd.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    want = np.prod(np.take_along_axis(p[:, None], lab[..., None].astype(np.int64), -1)[..., 0], axis=-1)
    assert np.allclose(sc, want, rtol=1e-5, atol=0)
