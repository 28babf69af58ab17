"""GPU: ProductQuantization('opq') against the reference's goldens (tests/golden/g4o_opq_*.npz), its training / file handling,
and --pq_type opq --pq_init_method faiss end to end (offline index build and the eval driver with multi-cluster documents)
against the CPU restatements of tests/opq_clusters_ref.py."""
import glob
import os
import pickle
import subprocess
import sys
from argparse import Namespace
from collections import defaultdict

import numpy as np
import pytest
import torch

import opq_cases as oc
import opq_clusters_ref as oref
import pq_ref
from oracle import t5 as ot5
from test_e2e_gpu import FakeTokenizer, _build_mini
from test_pq_gpu import _firm, _lines, _reference_side

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
OPQ_GOLDENS = sorted(glob.glob(os.path.join(GOLD, "g4o_opq_*.npz")))
assert len(OPQ_GOLDENS) == 3


def _quantiser(g, cuda):
    from mevi_amd import rq

    M, K, _ = g["C"].shape
    pq = rq.ProductQuantization("opq", M, int(np.log2(K)), "l2", g["X"].shape[1], device=cuda)
    pq.load_codebook(g["C"])
    pq.load_rotation(g["R"])
    return pq


@pytest.mark.parametrize("path", OPQ_GOLDENS, ids=os.path.basename)
def test_codes_clusters_and_reconstruct_match_reference_golden(cuda, path, monkeypatch):
    monkeypatch.delenv("MEVI_OPQ_ENCODE", raising=False)
    g = np.load(path)
    X = g["X"]
    pq = _quantiser(g, cuda)
    _, idx = pq.forward(torch.from_numpy(X).to(cuda))[:2]
    got = idx.cpu().numpy()
    assert np.array_equal(got, g["codes"])                                   # the rotation is exact: bit-equal codes
    assert np.array_equal(got, oref.encode(X, g["R"], g["C"]))
    monkeypatch.setenv("MEVI_OPQ_ENCODE", "steps")
    assert np.array_equal(pq.forward(torch.from_numpy(X).to(cuda))[1].cpu().numpy(), got)
    monkeypatch.setenv("MEVI_OPQ_ENCODE", "fused")
    assert np.array_equal(pq.forward(torch.from_numpy(X).to(cuda))[1].cpu().numpy(), got)
    monkeypatch.delenv("MEVI_OPQ_ENCODE")
    cluster, mapping = pq.get_document_cluster(X, 0, 1, return_mapping=True)
    keys = [tuple(k) for k in g["cluster_keys"].tolist()]
    assert sorted(cluster) == keys and [d for k in keys for d in cluster[k]] == g["cluster_docs"].tolist()
    assert all(mapping[i] == tuple(g["codes"][i].tolist()) for i in range(len(X)))
    parts = [pq.get_document_cluster(X, r, 3, as_index=True) for r in range(3)]
    assert sum(len(p.doc_ids) for p in parts) == len(X) and parts[2].doc_ids.min() == 2 * (len(X) // 3)
    rec = pq.get_reconstruct_vector(torch.from_numpy(g["codes"][:32]).to(cuda))
    assert np.array_equal(rec.cpu().numpy(), g["reconstruct32"])            # concatenation @ rotate, exact


@pytest.mark.parametrize("path", OPQ_GOLDENS, ids=os.path.basename)
def test_beam_search_matches_reference_golden(cuda, path):
    g = np.load(path)
    pq = _quantiser(g, cuda)
    got = {}
    for R in (5, 10):
        lab, sc = pq.beam_search(torch.from_numpy(g["X"][:64]), R, return_proba=True)
        lab, sc = lab.cpu().numpy(), sc.cpu().numpy()
        got[R] = lab
        # the tolerance tests/test_pq_gpu.py holds the 'pq' beams to: labels equal wherever the reference's scores are apart,
        # scores within 1e-6
        assert pq_ref.beams_agree(lab, sc, g[f"beam{R}_labels"], g[f"beam{R}_scores"])
        assert pq_ref.beams_agree(lab, sc, *oref.beam_search(g["X"][:64], g["R"], g["C"], R))
        assert np.array_equal(lab, g[f"beam{R}_labels"])
    topk = pq.get_topk_document_mapping(g["X"], 0, 1, 5, batch_size=100)                      # host rows, in batches
    assert np.array_equal(topk[:64].numpy(), got[5])
    on_dev = pq.get_topk_document_mapping(torch.from_numpy(g["X"]).to(cuda), 0, 1, 5)         # device rows, rotated in chunks
    assert torch.equal(on_dev, topk)


def test_initialize_trains_saves_and_loads(cuda, tmp_path, monkeypatch):
    from mevi_amd import rq

    monkeypatch.setenv("MEVI_OPQ_NITER", "2")
    M, bits, dim, n = 8, 4, 32, 700
    x = oc.outlier_rows(11, n, dim)
    path = str(tmp_path / "opqcodebook8_4.pt")
    pq = rq.ProductQuantization("opq", M, bits, "l2", dim, pq_init_method="faiss", device=cuda)
    pq.initialize(path, torch.from_numpy(x).to(cuda), rank=0, seed=41)
    saved = torch.load(path, map_location="cpu")
    assert sorted(saved) == ["codebook", "rotate"]
    assert tuple(saved["codebook"].shape) == (M, 1 << bits, dim // M) and tuple(saved["rotate"].shape) == (dim, dim)
    Rd = saved["rotate"].double().numpy()
    assert np.abs(Rd @ Rd.T - np.eye(dim)).max() <= 1e-5
    assert np.isfinite(saved["codebook"].numpy()).all()
    other = rq.ProductQuantization("opq", M, bits, "l2", dim, device=cuda)
    other.initialize(path, rank=0)                           # no embeddings needed: the file exists
    assert torch.equal(other.codebook, pq.codebook) and torch.equal(other.rotate, pq.rotate)
    assert torch.equal(other.codebook.cpu(), saved["codebook"]) and torch.equal(other.rotate.cpu(), saved["rotate"])
    codes = pq.forward(torch.from_numpy(x).to(cuda))[1].cpu().numpy()
    assert np.array_equal(codes, oref.encode(x, saved["rotate"].numpy(), saved["codebook"].numpy()))
    again = rq.ProductQuantization("opq", M, bits, "l2", dim, device=cuda)
    again.initialize(None, torch.from_numpy(x).to(cuda), rank=0, seed=41)     # deterministic, and nothing to save to
    assert torch.equal(again.rotate, pq.rotate) and torch.equal(again.codebook, pq.codebook)
    with pytest.raises(ValueError, match="256"):
        rq.ProductQuantization("opq", M, bits, "l2", dim, device=cuda).initialize(None, torch.from_numpy(x[:255]).to(cuda), rank=0)
    with pytest.raises(AssertionError):                       # the reference's k-means path asserts pq_type != 'opq' (pq.py:553)
        pq.unsupervised_update_codebook_manually(x, 41)


def test_rotation_pays_on_outlier_dimensions(cuda, monkeypatch):
    """The corpus and shape of tests/test_opq_index_gpu.py::test_trainer_on_the_device, at the trainer's default iterations: the
    reconstruction error of the 'opq' quantiser is at most 0.75 x that of 'pq' trained on the same rows (float64 restatement on
    the CPU, two seeds: 0.50 and 0.51)."""
    from mevi_amd import rq

    monkeypatch.delenv("MEVI_OPQ_NITER", raising=False)
    M, bits, dim, n = 8, 4, 32, 4096
    x = oc.outlier_rows(3, n, dim)
    xt = torch.from_numpy(x).to(cuda)
    err = {}
    for kind in ("opq", "pq"):
        pq = rq.ProductQuantization(kind, M, bits, "l2", dim, device=cuda)
        pq.initialize(None, xt, rank=0, seed=5)
        rec = pq.get_reconstruct_vector(pq.forward(xt)[1])
        err[kind] = float(((xt.double() - rec.double()) ** 2).sum().item()) / n
    print(f"reconstruction error opq {err['opq']:.5g} / pq {err['pq']:.5g} = {err['opq'] / err['pq']:.3f}")
    assert err["opq"] <= 0.75 * err["pq"], err


# ----------------------------------------------------------------------------------------------- end to end
M_, BITS_, K_, R_, DIM_ = 4, 5, 32, 10, 32


@pytest.fixture(scope="module")
def mini_opq(tmp_path_factory):
    """_build_mini with a corpus that is product-quantised behind a rotation: doc = (concatenated sub-centroids of a code path +
    noise) rotated back, over the beam code paths the model emits and random ones."""
    from mevi_amd import opq

    mini = _build_mini(tmp_path_factory.mktemp("marco_opq"), "g1_nci_M4_K32_R10.npz", M_, BITS_, R_)
    d = mini["dir"]
    rng = np.random.default_rng(23)
    enc = FakeTokenizer(512).batch_encode_plus(mini["queries"])
    dec, _, _ = ot5.nci_generate(mini["W"], mini["cfg"], enc["input_ids"], enc["attention_mask"], R_)
    beam_codes = ot5.decode_token(dec, K_).numpy()
    C = rng.standard_normal((M_, K_, DIM_ // M_)).astype(np.float32)
    Rm = opq.random_rotation(DIM_, 9).astype(np.float32)
    paths = np.concatenate([np.repeat(beam_codes[::3], 6, axis=0), rng.integers(0, K_, size=(2000, M_))])
    rng.shuffle(paths)
    N = len(paths)
    emb = ((pq_ref.reconstruct(paths, C) + 0.05 * rng.standard_normal((N, DIM_))) @ Rm.astype(np.float64)).astype(np.float32)
    emb.tofile(d / "ance" / "opqdocemb.bin")
    pq_path = d / "ance" / f"opqcodebook{M_}_{BITS_}.pt"
    torch.save({"codebook": torch.from_numpy(C), "rotate": torch.from_numpy(Rm)}, pq_path)
    a = Namespace(**vars(mini["args"]))
    a.pq_type, a.pq_init_method = "opq", "faiss"
    a.embedding_path = str(d / "ance" / "opqdocemb.bin")
    a.pq_path, a.pq_cluster_path = str(pq_path), str(d / "ance" / f"opqclus{M_}_{BITS_}.pkl")
    a.custom_save_path = str(d / "ance" / "nci_result_opq45_top10.tsv")
    gts = [[int(x) for x in rng.choice(N, size=1 + i % 2, replace=False)] for i in range(len(mini["queries"]))]
    with open(d / "origin" / "dev_mevi_dedup.tsv", "w") as f:
        for q, g_ in zip(mini["queries"], gts):
            f.write(f"{q}\t{','.join(map(str, g_))}\n")
    a.save_hard_neg = N
    codes = oref.encode(emb, Rm, C)
    assert (codes == paths).all(1).mean() > 0.9 and (pq_ref.pq_encode(emb, C) != codes).any(1).mean() > 0.9
    return dict(mini, args=a, emb=emb, C=C, R=Rm, N=N, gts=gts, codes=codes)


def test_offline_index_build_opq_cli_and_reuse(cuda, mini_opq, tmp_path):
    """`main.py --mode train --only_gen_rq 1 --pq_type opq --pq_init_method faiss`: no file -> the rotation and the codebook are
    trained and saved together; the pickles and the sidecar are the CPU restatement given the saved pair; a second build (in
    process) infers dim from the file's rotation and reuses everything."""
    from mevi_amd.indexbuild import build_index
    from oracle import rq as orq

    mini, a0 = mini_opq, mini_opq["args"]
    pq_path, clus = str(tmp_path / "opqcodebook4_5.pt"), str(tmp_path / "opqclus4_5.pkl")
    argv = [sys.executable, os.path.join(ROOT, "main.py"), "--mode", "train", "--only_gen_rq", "1", "--codebook", "1",
            "--pq_type", "opq", "--pq_init_method", "faiss", "--n_gpu", "1", "--subvector_num", str(M_), "--subvector_bits", str(BITS_),
            "--document_encoder", "ance", "--ckpt_dir", a0.ckpt_dir, "--data_dir", a0.data_dir,
            "--document_path", str(tmp_path / "all_document"), "--embedding_path", a0.embedding_path,
            "--pq_path", pq_path, "--pq_cluster_path", clus]
    r = subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT, MEVI_OPQ_NITER="2"), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "OPQ rotation: niter 2" in r.stdout
    saved = torch.load(pq_path, map_location="cpu")
    C, Rm = saved["codebook"].numpy(), saved["rotate"].numpy()
    assert C.shape == (M_, K_, DIM_ // M_) and Rm.shape == (DIM_, DIM_) and np.isfinite(C).all()
    assert np.abs(Rm.astype(np.float64) @ Rm.astype(np.float64).T - np.eye(DIM_)).max() <= 1e-5
    codes = oref.encode(mini["emb"], Rm, C)
    cluster, mapping = orq.cluster_dict(codes)
    map_path = clus.replace("clus", "mapping")
    assert pickle.load(open(clus, "rb")) == cluster and pickle.load(open(map_path, "rb")) == mapping
    from mevi_amd.metrics import mapping_sidecar

    assert np.array_equal(np.load(mapping_sidecar(map_path)), codes)
    stamps = {p: os.stat(p).st_mtime_ns for p in (pq_path, clus, map_path)}
    a = Namespace(**vars(a0))
    a.pq_path, a.pq_cluster_path, a.document_path = pq_path, clus, str(tmp_path / "all_document")
    n_docs, dim, nclus = build_index(a, device=cuda)
    assert (n_docs, dim, nclus) == (mini["N"], DIM_, len(cluster))
    assert stamps == {p: os.stat(p).st_mtime_ns for p in stamps}
    bare = str(tmp_path / "bare.pt")
    torch.save(saved["codebook"], bare)
    a.pq_path = bare
    with pytest.raises(SystemExit, match="rotation"):
        build_index(a, device=cuda)


def test_eval_driver_opq_with_multi_cluster_documents(cuda, mini_opq, tmp_path):
    """--pq_type opq --pq_init_method faiss --doc_multiclus 3: the pickles are the rotated encode, documents sit in the clusters of
    their top-3 code paths of the rotated rows; a document reached through several beams is listed once with its scores summed."""
    import shutil

    from mevi_amd.evalrun import EvalRun, load_queries
    from oracle import rq as orq

    mini = mini_opq
    a = Namespace(**vars(mini["args"]))
    shutil.copy(a.pq_path, tmp_path / "opqcodebook4_5.pt")
    a.pq_path, a.pq_cluster_path = str(tmp_path / "opqcodebook4_5.pt"), str(tmp_path / "opqclus4_5.pkl")
    a.custom_save_path, a.metric_path = str(tmp_path / "mc.tsv"), str(tmp_path / "mc_m.txt")
    a.doc_multiclus, a.multiclus_score_aggr = 3, "add"
    tok, codes, _, qemb = _reference_side(mini)
    out = EvalRun(a, tokenizer=tok, device=cuda).run(load_queries(a.data_dir))
    cluster, mapping = orq.cluster_dict(mini["codes"])
    assert pickle.load(open(a.pq_cluster_path, "rb")) == cluster          # the fused rotate + encode wrote the pickles
    assert pickle.load(open(a.pq_cluster_path.replace("clus", "mapping"), "rb")) == mapping
    labels, _ = oref.beam_search(mini["emb"], mini["R"], mini["C"], 3)
    got_labels = torch.load(str(tmp_path / "opqtopk34_5.pt")).numpy()
    assert got_labels.shape == labels.shape and (got_labels != labels).any(axis=(1, 2)).mean() < 0.01   # near-tie paths only
    assert (got_labels[:, 0] == mini["codes"]).all(1).mean() > 0.99                                      # path 0 = the encode
    multi = defaultdict(list)
    for i, paths in enumerate(got_labels.tolist()):
        for p_ in paths:
            multi[tuple(p_)].append(i)
    assert pickle.load(open(tmp_path / "opqmulticlus34_5.pkl", "rb")) == dict(multi)
    coarse, hn = _lines(a.custom_save_path[:-4] + "_coarse.tsv"), _lines(f"{a.custom_save_path[:-4]}_hn{a.save_hard_neg}.tsv")
    nd = repeats = 0
    for i in range(len(mini["queries"])):
        assert eval(coarse[i][1]) == codes[i].tolist()
        assert eval(coarse[i][2]) == [got_labels[g].tolist() for g in mini["gts"][i]]
        docs = [x for c in codes[i].tolist() for x in multi.get(tuple(c), [])]
        nd += len(docs)
        if not docs:
            continue
        u, cnt = np.unique(docs, return_counts=True)
        repeats += int((cnt > 1).sum())
        want = (mini["emb"][u] @ qemb[i]) * cnt
        got_docs = [int(x) for x in hn[i][2].split(",")]
        got_s = np.array([float(x) for x in hn[i][3].split(",")])
        order = np.argsort(-want, kind="stable")
        assert sorted(got_docs) == u.tolist() and np.abs(got_s - want[order]).max() <= 5e-4
        firm = _firm(want[order], 2e-3)
        assert all(got_docs[j] == int(u[order[j]]) for j in np.nonzero(firm)[0])
    assert nd > 50 and repeats > 5, "fixture should populate beam clusters and reach some documents through several beams"
    assert abs(out["ndoc"] - nd / len(mini["queries"])) < 1e-9
