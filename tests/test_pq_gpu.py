"""GPU: product-quantisation encode (mevi_pq_encode_f32) bit for bit against the per-slice oracle, the 'pq'
ProductQuantization against the reference's goldens (tests/golden/g4p_pq_*.npz), and --pq_type pq end to end
(offline index build and the eval driver) against CPU restatements from the oracle pieces."""
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

import pq_ref
from oracle import t5 as ot5
from test_e2e_gpu import FakeTokenizer, _build_mini

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PQ_GOLDENS = sorted(glob.glob(os.path.join(GOLD, "g4p_pq_*.npz")))


def _gpu_codes(x, cb, cuda):
    from mevi_amd import rq

    c = rq.pq_encode(torch.from_numpy(np.ascontiguousarray(x)).to(cuda), torch.from_numpy(cb).to(cuda))
    torch.cuda.synchronize()
    return c.cpu().numpy()


@pytest.mark.parametrize("n,M,K,dsub,extra", [
    (0, 4, 32, 16, 0),
    (1, 2, 16, 8, 0),
    (1, 32, 256, 24, 0),       # the parser's default shape (32 x 8 bits over 768)
    (1000, 1, 2, 768, 0),
    (129, 2, 256, 4, 4),       # trailing columns past M * dsub
    (300, 3, 16, 36, 8),       # dsub not a multiple of the 32-wide k slab
    (517, 4, 32, 192, 0),      # the scripts' M x K over 768
    (1000, 8, 256, 96, 0),
    (777, 32, 256, 24, 0),
    (2049, 32, 2, 4, 12),
    (333, 8, 32, 68, 0),
    (130, 4, 256, 40, 0),
])
def test_kernel_bit_identical_to_per_slice_oracle(cuda, n, M, K, dsub, extra):
    rng = np.random.default_rng(n * 7 + M * 3 + K + dsub)
    x = rng.standard_normal((n, M * dsub + extra)).astype(np.float32)
    cb = rng.standard_normal((M, K, dsub)).astype(np.float32)
    got = _gpu_codes(x, cb, cuda)
    assert got.shape == (n, M) and np.array_equal(got, pq_ref.pq_encode(x, cb))


def test_ties_far_rows_and_nan_rows(cuda):
    rng = np.random.default_rng(3)
    M, K, dsub = 4, 32, 16
    cb = rng.integers(-2, 3, size=(M, K, dsub)).astype(np.float32)
    cb[:, 7] = cb[:, 3]                     # duplicated centroids: exact distance ties, lowest index wins
    cb[:, 30] = cb[:, 11]
    cb[2, 20:] = cb[2, 19]
    x = rng.integers(-4, 5, size=(700, M * dsub)).astype(np.float32)
    x[10] = 1e17                            # far from every centroid, distances finite
    x[11] = -1e20                           # distances overflow to +inf everywhere: code 0
    x[12, :dsub] = np.nan                   # a NaN slice: code 0 for that subspace only
    x[13] = np.nan
    x[14, 5] = np.inf
    got = _gpu_codes(x, cb, cuda)
    assert np.array_equal(got, pq_ref.pq_encode(x, cb))
    assert not np.isin(got, [7, 30]).any() and not (got[:, 2] > 19).any()
    assert (got[11] == 0).all() and got[12, 0] == 0 and (got[13] == 0).all()


def test_unsupported_shapes_are_refused(cuda):
    from mevi_amd import hip

    L = hip.lib()
    x = torch.zeros((64, 1024), device=cuda)
    cb = torch.zeros(1 << 20, device=cuda)
    codes = torch.zeros((64, 64), dtype=torch.int32, device=cuda)

    def call(n, dim, M, K, dsub):
        return L.mevi_pq_encode_f32(hip.ptr(x), n, dim, hip.ptr(cb), M, K, dsub, hip.ptr(codes), hip.stream_ptr())

    for n in (0, 64):
        assert call(n, 1024, 4, 257, 16) == -2          # K > 256
        assert call(n, 1024, 33, 32, 16) == -2          # M > 32
        assert call(n, 1024, 4, 32, 6) == -2            # dsub % 4
        assert call(n, 1022, 2, 32, 8) == -2            # dim % 4
        assert call(n, 1024, 4, 32, 257) == -1          # M * dsub > dim
    assert call(0, 1024, 32, 256, 32) == 0 and call(64, 1024, 32, 256, 32) == 0
    torch.cuda.synchronize()
    from mevi_amd import rq

    with pytest.raises(hip.MeviHipError):
        rq.pq_encode(torch.zeros((4, 1028), device=cuda), torch.zeros((4, 300, 256), device=cuda))


@pytest.mark.parametrize("path", PQ_GOLDENS, ids=os.path.basename)
def test_codes_and_clusters_match_reference_golden(cuda, path):
    from mevi_amd import rq

    g = np.load(path)
    X, C = g["X"], g["C"]
    M, K, dsub = C.shape
    got = _gpu_codes(X, C, cuda)
    assert np.array_equal(got, pq_ref.pq_encode(X, C))
    assert pq_ref.codes_agree(got, g["codes"], pq_ref.near_tie_sets(X, C))
    pq = rq.ProductQuantization("pq", M, int(np.log2(K)), "l2", X.shape[1], device=cuda)
    assert tuple(pq.codebook.shape) == (M, K, X.shape[1] // M)
    pq.load_codebook(C)
    with pytest.raises(AssertionError):
        pq.load_codebook(np.zeros((M, K, X.shape[1]), np.float32))
    cluster, mapping = pq.get_document_cluster(X, 0, 1, return_mapping=True)
    keys = [tuple(k) for k in g["cluster_keys"].tolist()]
    assert sorted(cluster) == keys and [d for k in keys for d in cluster[k]] == g["cluster_docs"].tolist()
    assert all(mapping[i] == tuple(g["codes"][i].tolist()) for i in range(len(X)))
    parts = [pq.get_document_cluster(X, r, 3, as_index=True) for r in range(3)]   # rows // nrank, last rank the rest
    assert sum(len(p.doc_ids) for p in parts) == len(X) and parts[2].doc_ids.min() == 2 * (len(X) // 3)
    _, idx = pq.forward(torch.from_numpy(X).to(cuda))[:2]
    assert np.array_equal(idx.cpu().numpy(), got)
    rec = pq.get_reconstruct_vector(torch.from_numpy(g["codes"][:32]).to(cuda))
    assert np.array_equal(rec.cpu().numpy(), g["reconstruct32"])            # concatenation, exact


@pytest.mark.parametrize("path", PQ_GOLDENS, ids=os.path.basename)
def test_beam_search_matches_reference_golden(cuda, path):
    from mevi_amd import rq

    g = np.load(path)
    M, K, _ = g["C"].shape
    pq = rq.ProductQuantization("pq", M, int(np.log2(K)), "l2", g["X"].shape[1], device=cuda)
    pq.load_codebook(g["C"])
    got = {}
    for R in (5, 10):
        lab, sc = pq.beam_search(torch.from_numpy(g["X"][:64]), R, return_proba=True)
        lab, sc = lab.cpu().numpy(), sc.cpu().numpy()
        got[R] = lab
        # labels equal wherever the reference's scores are apart, scores within 1e-6 (exact near-ties as sets)
        assert pq_ref.beams_agree(lab, sc, g[f"beam{R}_labels"], g[f"beam{R}_scores"])
        assert pq_ref.beams_agree(lab, sc, *pq_ref.beam_search(g["X"][:64], g["C"], R))
    topk = pq.get_topk_document_mapping(g["X"], 0, 1, 5, batch_size=100)
    assert np.array_equal(topk[:64].numpy(), got[5])


def test_training_is_deterministic_and_improves_on_its_initialisation(cuda):
    from mevi_amd import rq

    rng = np.random.default_rng(8)
    M, K, dim, n = 4, 16, 32, 3000
    dsub = dim // M
    centres = rng.standard_normal((M, K, dsub)).astype(np.float32)
    x = np.concatenate([centres[j][rng.integers(0, K, n)] for j in range(M)], 1)
    x = (x + 0.3 * rng.standard_normal((n, dim))).astype(np.float32)
    xt = torch.from_numpy(x).to(cuda)
    books = []
    for _ in range(2):
        pq = rq.ProductQuantization("pq", M, 4, "l2", dim, device=cuda)
        pq.unsupervised_update_codebook_manually(x, seed=41)
        books.append((pq.codebook.cpu().numpy(), pq.last_preds))
    assert np.array_equal(books[0][0], books[1][0]) and np.array_equal(books[0][1], books[1][1])
    C, preds = books[0]
    assert C.shape == (M, K, dsub) and preds.shape == (n, M) and preds.dtype == np.int64
    assert np.array_equal(preds, pq_ref.pq_encode(x, C))      # last_preds = the codes of the returned codebook
    other = rq.ProductQuantization("pq", M, 4, "l2", dim, device=cuda)
    other.unsupervised_update_codebook_manually(x, seed=42)
    assert not np.array_equal(other.codebook.cpu().numpy(), C)
    for j in range(M):                                        # subspace j = k-means(slice j, seed + j)
        sl = xt[:, j * dsub:(j + 1) * dsub].contiguous()
        cj, _, _ = rq.kmeans(sl, K, seed=41 + j)
        assert torch.equal(cj.cpu(), torch.from_numpy(C[j]))
        init, _, _ = rq.kmeans(sl, K, seed=41 + j, max_iter=0)    # the centres the full-data Lloyd run starts from

        def err(book):
            c = pq_ref.pq_encode(x[:, j * dsub:(j + 1) * dsub], book[None])[:, 0]
            return float(((x[:, j * dsub:(j + 1) * dsub].astype(np.float64) - book[c]) ** 2).sum())

        assert err(C[j]) <= err(init.cpu().numpy())


# ----------------------------------------------------------------------------------------------- end to end
M_, BITS_, K_, R_, DIM_ = 4, 5, 32, 10, 32


@pytest.fixture(scope="module")
def mini_pq(tmp_path_factory):
    """_build_mini with a product-quantised corpus: doc = concatenated sub-centroids of a code path + noise, over the
    beam code paths the model emits and random ones."""
    mini = _build_mini(tmp_path_factory.mktemp("marco_pq"), "g1_nci_M4_K32_R10.npz", M_, BITS_, R_)
    d = mini["dir"]
    rng = np.random.default_rng(17)
    enc = FakeTokenizer(512).batch_encode_plus(mini["queries"])
    dec, _, _ = ot5.nci_generate(mini["W"], mini["cfg"], enc["input_ids"], enc["attention_mask"], R_)
    beam_codes = ot5.decode_token(dec, K_).numpy()
    C = rng.standard_normal((M_, K_, DIM_ // M_)).astype(np.float32)
    paths = np.concatenate([np.repeat(beam_codes[::3], 6, axis=0), rng.integers(0, K_, size=(2000, M_))])
    rng.shuffle(paths)
    N = len(paths)
    emb = (pq_ref.reconstruct(paths, C) + 0.05 * rng.standard_normal((N, DIM_))).astype(np.float32)
    emb.tofile(d / "ance" / "pqdocemb.bin")
    torch.save(torch.nn.Parameter(torch.from_numpy(C)), d / "ance" / f"pqcodebook{M_}_{BITS_}.pt")
    a = Namespace(**vars(mini["args"]))
    a.pq_type = "pq"
    a.embedding_path = str(d / "ance" / "pqdocemb.bin")
    a.pq_path, a.pq_cluster_path = str(d / "ance" / f"pqcodebook{M_}_{BITS_}.pt"), str(d / "ance" / f"pqclus{M_}_{BITS_}.pkl")
    a.custom_save_path = str(d / "ance" / "nci_result_pq45_top10.tsv")
    gts = [[int(x) for x in rng.choice(N, size=1 + i % 2, replace=False)] for i in range(len(mini["queries"]))]
    with open(d / "origin" / "dev_mevi_dedup.tsv", "w") as f:
        for q, g_ in zip(mini["queries"], gts):
            f.write(f"{q}\t{','.join(map(str, g_))}\n")
    a.save_hard_neg = N
    return dict(mini, args=a, emb=emb, C=C, N=N, gts=gts)


def _lines(path):
    return [l.rstrip("\n").split("\t") for l in open(path)]


def _reference_side(mini, R=R_):
    tok = FakeTokenizer(512)
    enc = tok.batch_encode_plus(mini["queries"])
    dec, sc, _ = ot5.nci_generate(mini["W"], mini["cfg"], enc["input_ids"], enc["attention_mask"], R)
    codes = ot5.decode_token(dec, K_).view(len(mini["queries"]), R, M_).numpy()
    qemb = ot5.tower_encode(mini["TW"], mini["tcfg"], enc["input_ids"], enc["attention_mask"]).numpy()
    return tok, codes, sc.numpy().reshape(len(mini["queries"]), R), qemb


def _firm(ref_s, tol):
    g = np.abs(np.diff(ref_s)) > tol
    return np.concatenate([[True], g]) & np.concatenate([g, [True]])


def test_eval_driver_pq_matches_cpu_restatement(cuda, mini_pq):
    from mevi_amd.evalrun import EvalRun, load_queries

    mini, a = mini_pq, mini_pq["args"]
    tok, codes, sc, qemb = _reference_side(mini)
    out = EvalRun(a, tokenizer=tok, device=cuda).run(load_queries(a.data_dir))
    prefix = a.custom_save_path[:-4]
    coarse, fine, hn = _lines(prefix + "_coarse.tsv"), _lines(prefix + "_fine.tsv"), _lines(f"{prefix}_hn{a.save_hard_neg}.tsv")
    assert len(coarse) == len(fine) == len(hn) == len(mini["queries"])
    from oracle import rq as orq

    cluster, mapping = orq.cluster_dict(pq_ref.pq_encode(mini["emb"], mini["C"]))
    assert pickle.load(open(a.pq_cluster_path, "rb")) == cluster          # GPU PQ encode wrote the reference's pickles
    assert pickle.load(open(a.pq_cluster_path.replace("clus", "mapping"), "rb")) == mapping
    nd = 0
    for i, q in enumerate(mini["queries"]):
        assert coarse[i][0] == fine[i][0] == hn[i][0] == q
        assert eval(coarse[i][1]) == codes[i].tolist()
        assert np.abs(np.array(eval(coarse[i][3])) - sc[i]).max() <= 1e-5
        assert eval(coarse[i][2]) == [list(mapping[g]) for g in mini["gts"][i]]
        docs = [d for c in codes[i].tolist() for d in cluster.get(tuple(c), [])]
        nd += len(docs)
        got_docs = eval(fine[i][1])
        assert sorted(got_docs) == sorted(docs) and eval(fine[i][2]) == mini["gts"][i]
        if docs:
            ref = mini["emb"][docs] @ qemb[i]
            order = np.argsort(-ref, kind="stable")
            got_s = np.array([float(x) for x in hn[i][3].split(",")])
            assert np.abs(got_s - ref[order]).max() <= 2e-4
            assert [int(x) for x in hn[i][2].split(",")] == got_docs
            firm = _firm(ref[order], 1e-3)
            assert all(got_docs[j] == docs[order[j]] for j in np.nonzero(firm)[0])
        gs = np.array([float(x) for x in hn[i][1].split(",")])
        assert np.abs(gs - mini["emb"][mini["gts"][i]] @ qemb[i]).max() <= 2e-4
    assert nd > 50, "fixture should populate beam clusters"
    assert abs(out["ndoc"] - nd / len(mini["queries"])) < 1e-9


def test_eval_driver_pq_with_multi_cluster_documents(cuda, mini_pq, tmp_path):
    """--doc_multiclus 3: documents in the clusters of their top-3 'pq' code paths; a document reached through several
    beams is listed once with its scores summed."""
    import shutil

    from mevi_amd.evalrun import EvalRun, load_queries

    mini = mini_pq
    a = Namespace(**vars(mini["args"]))
    shutil.copy(a.pq_path, tmp_path / "pqcodebook4_5.pt")
    a.pq_path, a.pq_cluster_path = str(tmp_path / "pqcodebook4_5.pt"), str(tmp_path / "pqclus4_5.pkl")
    a.custom_save_path, a.metric_path = str(tmp_path / "mc.tsv"), str(tmp_path / "mc_m.txt")
    a.doc_multiclus, a.multiclus_score_aggr = 3, "add"
    tok, codes, _, qemb = _reference_side(mini)
    out = EvalRun(a, tokenizer=tok, device=cuda).run(load_queries(a.data_dir))
    labels, _ = pq_ref.beam_search(mini["emb"], mini["C"], 3)
    got_labels = torch.load(str(tmp_path / "pqtopk34_5.pt")).numpy()
    assert got_labels.shape == labels.shape and (got_labels != labels).any(axis=(1, 2)).mean() < 0.01   # near-tie paths only
    multi = defaultdict(list)
    for i, paths in enumerate(got_labels.tolist()):
        for p_ in paths:
            multi[tuple(p_)].append(i)
    assert pickle.load(open(tmp_path / "pqmulticlus34_5.pkl", "rb")) == dict(multi)
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
    assert repeats > 5, "fixture should reach some documents through several beams"
    assert abs(out["ndoc"] - nd / len(mini["queries"])) < 1e-9


def test_eval_driver_pq_with_topic_model(cuda, mini_pq, tmp_path):
    """--use_topic_model 1 --topic_score_ratio 0.3: a document scores beam_score x (0.3 <reconstruct(code(d)), emb[d]> +
    0.7 q.d), the reconstruct vector being the concatenation of the document's sub-centroids."""
    from mevi_amd.evalrun import EvalRun, load_queries

    mini, ratio = mini_pq, 0.3
    a = Namespace(**vars(mini["args"]))
    a.use_topic_model, a.topic_score_ratio = 1, ratio
    a.custom_save_path, a.metric_path = str(tmp_path / "t.tsv"), str(tmp_path / "m.txt")
    tok, codes, sc, qemb = _reference_side(mini)
    EvalRun(a, tokenizer=tok, device=cuda).run(load_queries(a.data_dir))
    from oracle import rq as orq

    codes_doc = pq_ref.pq_encode(mini["emb"], mini["C"])
    cluster, _ = orq.cluster_dict(codes_doc)
    emb, qemb = torch.from_numpy(mini["emb"]), torch.from_numpy(qemb)
    doc_proba = torch.sum(torch.from_numpy(pq_ref.reconstruct(codes_doc, mini["C"])) * emb, dim=-1)
    nci_scores = torch.tensor(sc.tolist(), dtype=torch.float32)
    hn = _lines(f"{a.custom_save_path[:-4]}_hn{a.save_hard_neg}.tsv")
    checked = 0
    for i in range(len(mini["queries"])):
        scores, docs = [], []
        for r in range(R_):
            cur = cluster.get(tuple(codes[i, r].tolist()))
            if cur is not None:
                scores.append(nci_scores[i][r].item() * (ratio * doc_proba[cur] + (1 - ratio) * (qemb[i] @ emb[cur].T)))
                docs += cur
        if not docs:
            assert hn[i][2] == ""
            continue
        ref_s, order = torch.sort(torch.cat(scores), descending=True)
        ref_d = np.array(docs)[order.numpy()]
        got_d = [int(x) for x in hn[i][2].split(",")]
        got_s = np.array([float(x) for x in hn[i][3].split(",")])
        assert sorted(got_d) == sorted(docs) and np.abs(got_s - ref_s.numpy()).max() <= 2e-4 * max(1.0, float(ref_s.abs().max()))
        firm = _firm(ref_s.numpy(), 1e-3)
        assert all(got_d[j] == int(ref_d[j]) for j in np.nonzero(firm)[0])
        checked += int(firm.sum())
    assert checked > 50


def test_offline_index_build_pq_cli(cuda, mini_pq, tmp_path):
    """`main.py --mode train --only_gen_rq 1 --pq_type pq`: no codebook file -> per-slice k-means trains one of shape
    [M, K, dim / M]; the cluster pickles are the oracle encode with that codebook."""
    from oracle import rq as orq

    mini, a0 = mini_pq, mini_pq["args"]
    pq_path, clus = str(tmp_path / "pqcodebook4_5.pt"), str(tmp_path / "pqclus4_5.pkl")
    argv = [sys.executable, os.path.join(ROOT, "main.py"), "--mode", "train", "--only_gen_rq", "1", "--codebook", "1",
            "--pq_type", "pq", "--n_gpu", "1", "--subvector_num", str(M_), "--subvector_bits", str(BITS_),
            "--document_encoder", "ance", "--ckpt_dir", a0.ckpt_dir, "--data_dir", a0.data_dir,
            "--document_path", str(tmp_path / "all_document"), "--embedding_path", a0.embedding_path,
            "--pq_path", pq_path, "--pq_cluster_path", clus]
    r = subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    C = torch.load(pq_path, map_location="cpu").detach().numpy()
    assert C.shape == (M_, K_, DIM_ // M_) and np.isfinite(C).all()
    cluster, mapping = orq.cluster_dict(pq_ref.pq_encode(mini["emb"], C))
    assert pickle.load(open(clus, "rb")) == cluster
    assert pickle.load(open(clus.replace("clus", "mapping"), "rb")) == mapping
    recon = pq_ref.reconstruct(np.array([mapping[d] for d in range(mini["N"])]), C)
    assert ((mini["emb"] - recon) ** 2).sum() < 0.2 * ((mini["emb"] - mini["emb"].mean(0)) ** 2).sum()
