"""CPU: --pq_type opq on the command line (accepted only together with --pq_init_method faiss), the rotated product-quantisation
goldens (tools/capture_goldens_opq.py) pinned to the oracle's arithmetic through tests/opq_clusters_ref.py, the header and the
binding of mevi_opq_encode_f32 with every refusal before a launch, the {"codebook", "rotate"} file of `pq_path` and the
checkpoint helper."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import opq_clusters_ref as oref
import pq_ref
from test_pq_cpu import EVAL, GEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
OPQ_GOLDENS = sorted(glob.glob(os.path.join(GOLD, "g4o_opq_*.npz")))
INVALID, UNSUPPORTED = -1, -2
FAISS = ["--pq_type", "opq", "--pq_init_method", "faiss"]


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


# ---- the command line ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [EVAL, GEN], ids=["eval", "only_gen_rq"])
def test_check_supported_matrix(argv):
    import main

    a = main.parsers_parser(argv + FAISS)
    main.check_supported(a)
    assert a.pq_type == "opq" and a.pq_init_method == "faiss"
    assert "--pq_init_method" not in [f for f, _ in a.ignored_flags]          # read, not ignored
    for extra in (["--pq_type", "opq"], ["--pq_type", "opq", "--pq_init_method", "kmeans"],
                  ["--pq_type", "opq", "--pq_init_method", "none"]):
        with pytest.raises(SystemExit) as e:
            main.check_supported(main.parsers_parser(argv + extra))
        assert "--pq_init_method" in str(e.value)                              # the message names the flag
    for refused in (["--use_topic_model", "1"], ["--eval_all_documents", "1", "--recall_level", "fine", "--knn_topk_by_step", "1"],
                    ["--subvector_num", "5"], ["--subvector_num", "384"], ["--subvector_num", "64"]):
        with pytest.raises(SystemExit):
            main.check_supported(main.parsers_parser(argv + FAISS + refused))
    main.check_supported(main.parsers_parser(argv + FAISS + ["--subvector_num", "32", "--subvector_bits", "8"]))
    for kind in ("pq", "rq"):                                                   # the other codings do not read the flag
        for method in ("faiss", "kmeans"):
            a = main.parsers_parser(argv + ["--pq_type", kind, "--pq_init_method", method])
            main.check_supported(a)
            assert ("--pq_init_method", method) in a.ignored_flags


def test_refused_ablations_cite_the_reference():
    import main

    with pytest.raises(SystemExit) as e:
        main.check_supported(main.parsers_parser(EVAL + FAISS + ["--use_topic_model", "1"]))
    assert "main_models.py:3303" in str(e.value)
    main.check_supported(main.parsers_parser(EVAL + FAISS + ["--doc_multiclus", "3"]))     # multi-cluster documents are built


# ---- the goldens -------------------------------------------------------------------------------------------------------------
def test_goldens_cover_the_requested_shapes():
    shapes = {tuple(np.load(p)["C"].shape[:2]) + np.load(p)["X"].shape[::-1] for p in OPQ_GOLDENS}
    assert shapes == {(4, 32, 64, 300), (8, 256, 64, 200), (11, 16, 44, 257)}
    assert all(os.path.getsize(p) < 1 << 20 for p in OPQ_GOLDENS)


@pytest.mark.parametrize("path", OPQ_GOLDENS, ids=os.path.basename)
def test_goldens_pinned_by_the_restatement(path):
    g = np.load(path)
    X, R, C = g["X"], g["R"], g["C"]
    dim = X.shape[1]
    # the rotation is exact under any summation order: orthonormal with power-of-two entries, the chain = float64 = a BLAS matmul
    assert np.array_equal(R.astype(np.float64) @ R.astype(np.float64).T, np.eye(dim))
    assert set(np.unique(np.abs(R[R != 0]))) == {np.abs(R[R != 0]).max()} and np.log2(np.abs(R[R != 0]).max()) % 1 == 0
    Y = oref.rotate(X, R)
    assert np.array_equal(Y.astype(np.float64), X.astype(np.float64) @ R.astype(np.float64).T)
    assert np.array_equal(Y, (torch.from_numpy(X) @ torch.from_numpy(R).t()).numpy())
    codes = oref.encode(X, R, C)
    assert pq_ref.codes_agree(codes, g["codes"], pq_ref.near_tie_sets(Y, C))
    assert (pq_ref.pq_encode(X, C) != g["codes"]).any(1).all()                 # a missing rotation cannot pass, on any row
    assert np.array_equal(oref.reconstruct(g["codes"][:32], R, C), g["reconstruct32"])
    from oracle import rq as orq

    cluster, _ = orq.cluster_dict(g["codes"])
    keys = [tuple(k) for k in g["cluster_keys"].tolist()]
    assert sorted(cluster) == keys and [d for k in keys for d in cluster[k]] == g["cluster_docs"].tolist()
    assert [len(cluster[k]) for k in keys] == g["cluster_sizes"].tolist()
    assert max(g["cluster_sizes"].tolist()) > 1                                 # clusters with several members
    for nbeam in (5, 10):
        lab, sc = oref.beam_search(X[:64], R, C, nbeam)
        assert pq_ref.beams_agree(lab, sc, g[f"beam{nbeam}_labels"], g[f"beam{nbeam}_scores"])


# ---- the entry points ----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_both_entry_points(L):
    from mevi_amd import hip, rq

    assert '#include "mevi_hip_opq_encode.h"' in open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    raw = open(os.path.join(ROOT, "include", "mevi_hip_opq_encode.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mevi_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["mevi_opq_encode_f32", "mevi_opq_encode_fused"]
    assert hip.exported_symbols("mevi_hip_opq_encode.h") == declared and declared == sorted(hip._OPQ_ENCODE_SIGNATURES)
    for other in ("mevi_hip.h", "mevi_hip_opq.h", "mevi_hip_aq.h", "mevi_hip_ivfpq.h"):
        assert not set(declared) & set(hip.exported_symbols(other)), other
    for name in declared:
        fn = getattr(L, name)
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text, flags=re.S).group(1).split(",")
        assert len(fn.argtypes) == len(args)
        for c_type, decl in zip(fn.argtypes, args):
            assert ("*" in decl) == (c_type.__name__ == "c_void_p") and ("int64_t " in decl or "*" in decl), decl
    assert callable(rq.opq_encode) and rq.OPQ_ENCODE_DEFAULT in ("fused", "steps")


def test_fused_envelope_is_host_arithmetic(L):
    f = L.mevi_opq_encode_fused
    for shape in ((768, 4, 32, 192), (768, 32, 256, 24), (64, 4, 32, 16), (44, 11, 16, 4), (1024, 8, 256, 128), (128, 8, 64, 16)):
        assert f(*shape) == 1, shape
    for shape in ((1024, 2, 32, 512), (4096, 32, 32, 128), (1028, 257, 32, 4), (768, 4, 32, 191), (768, 4, 257, 192),
                  (768, 4, 0, 192), (768, 33, 32, 24), (66, 3, 16, 22), (768, 4, 32, 96), (0, 0, 32, 0), (-64, 4, 32, -16)):
        assert f(*shape) == 0, shape


def test_refusals_come_before_any_launch(L):
    """Fake pointers: nothing may dereference them, and the library runs no kernel without a GPU."""
    A = 1 << 20

    def call(x=A, n=50, dim=64, R=A, cb=A, M=4, K=32, dsub=16, codes=A):
        st = L.mevi_opq_encode_f32(x, n, dim, R, cb, M, K, dsub, codes, None)
        return st, L.mevi_last_error().decode()

    def refused(code, word, **kw):
        for n in ((kw.pop("n"),) if "n" in kw else (50, 0)):                    # every refusal also for n == 0
            st, msg = call(n=n, **kw)
            assert st == code and word in msg and msg.startswith("opq_encode:"), (kw, n, st, msg)

    refused(INVALID, "n=-1", n=-1)
    refused(INVALID, "dim=0", dim=0, M=0, dsub=0)
    refused(INVALID, "K=0", K=0)
    refused(INVALID, "M=-1", M=-1)
    refused(INVALID, "dsub=12", dsub=12)                    # M * dsub != dim
    refused(UNSUPPORTED, "M=33", M=33, dim=132, dsub=4)
    refused(UNSUPPORTED, "K=257", K=257)
    refused(UNSUPPORTED, "dim=66", dim=66, M=3, dsub=22)
    refused(UNSUPPORTED, "dsub=6", dim=24, M=4, dsub=6)
    refused(UNSUPPORTED, "dim=4100", dim=4100, M=25, dsub=164)
    refused(UNSUPPORTED, "n=", n=1 << 31)
    refused(UNSUPPORTED, "dsub=512", dim=1024, M=2, dsub=512)      # inside the call's envelope, outside the fused kernel
    refused(UNSUPPORTED, "dim=4096", dim=4096, M=32, dsub=128)
    for name in ("R", "cb"):
        refused(INVALID, "null", **{name: None})
    for name in ("x", "codes"):
        refused(INVALID, "null", n=50, **{name: None})
    for name, step in (("x", 8), ("R", 4), ("cb", 8), ("codes", 2)):
        refused(INVALID, "align", **{name: A + step})
    assert call(n=0, x=None, codes=None)[0] == 0            # nothing to do: no launch, nothing dereferenced
    assert call(n=0)[0] == 0


# ---- the files -----------------------------------------------------------------------------------------------------------------
def test_pq_path_dict_round_trips_and_a_bare_tensor_is_refused(tmp_path):
    from mevi_amd import rq

    g = np.load(OPQ_GOLDENS[0])
    M, K, dsub = g["C"].shape
    dim = g["X"].shape[1]
    pq = rq.ProductQuantization("opq", M, int(np.log2(K)), "l2", dim, device="cpu")
    assert tuple(pq.rotate.shape) == (dim, dim) and tuple(pq.codebook.shape) == (M, K, dsub)
    path = str(tmp_path / "opqcodebook.pt")
    torch.save({"codebook": torch.from_numpy(g["C"]), "rotate": torch.from_numpy(g["R"])}, path)
    pq.initialize(path, rank=0)
    assert np.array_equal(pq.codebook.numpy(), g["C"]) and np.array_equal(pq.rotate.numpy(), g["R"])
    bare = str(tmp_path / "pqcodebook.pt")
    torch.save(torch.from_numpy(g["C"]), bare)
    with pytest.raises(ValueError, match="rotat"):
        rq.ProductQuantization("opq", M, int(np.log2(K)), "l2", dim, device="cpu").initialize(bare, rank=0)
    with pytest.raises(AssertionError):
        pq.load_rotation(np.zeros((dim, dim + 4), np.float32))
    with pytest.raises(FileNotFoundError):
        pq.initialize(str(tmp_path / "missing.pt"), rank=0)
    for M_bad, dim_bad in ((5, 64), (8, 48), (32, 64)):       # dim % M, or slices that are no multiple of 4 columns
        with pytest.raises(NotImplementedError, match=str(dim_bad)):
            rq.ProductQuantization("opq", M_bad, 4, "l2", dim_bad, device="cpu")
    plain = rq.ProductQuantization("pq", M, int(np.log2(K)), "l2", dim, device="cpu")
    assert plain.rotate is None
    plain.initialize(bare, rank=0)                             # 'pq' still reads the bare tensor


def test_checkpoint_helper_finds_the_rotation():
    from mevi_amd import evalrun

    sd = {"model.shared.weight": torch.zeros(4, 4), "pq.codebook": torch.zeros(2, 4, 8), "pq.rotate": torch.eye(16)}
    out = evalrun.split_whole_checkpoint(sd)
    assert len(out) == 3 and out[2] is sd["pq.codebook"]
    assert evalrun.checkpoint_rotation(sd) is sd["pq.rotate"]
    del sd["pq.rotate"]
    assert evalrun.checkpoint_rotation(sd) is None
