#!/usr/bin/env python3
"""Capture the rotated product-quantisation goldens (tests/golden/g4o_opq_*.npz) by importing the read-only reference.

Runs ONLY in the build container, like tools/capture_goldens_pq.py: everything written is data (seeded rows, rotations and
codebooks + the reference's own outputs of ProductQuantization('opq', M, bits, 'l2') with `codebook` and `rotate` copied in); no
reference source travels.

The reference rotates with a BLAS matmul whose summation order is not this project's sequential chain, so the fixtures make the
rotation exact in f32 under ANY order (tests/opq_clusters_ref.exact_case): R is a signed, permuted block-diagonal matrix of
normalised Hadamard blocks of size 4^p (entries +-2^-p), the rotated rows lie on multiples of 2^-6 and the centroids on
multiples of 2^-8.

  python tools/capture_goldens_opq.py
"""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_import  # noqa: E402

# (M, bits, dim, rows, Hadamard block): the scripts' 4 x 5, the parser's 8 bits, and one whose dim is no multiple of 32 with
# K = 16 < R at the first beam step (all candidates kept)
CASES = [(4, 5, 64, 300, 64), (8, 8, 64, 200, 16), (11, 4, 44, 257, 4)]


def g4o_opq():
    """get_pq_document_cluster / beam_search / get_reconstruct_vector of MEVI/pq.py with pq_type 'opq', dist_mode 'l2'."""
    import opq_clusters_ref as oref
    import pq_ref

    ref_import.setup()
    import torch
    from pq import ProductQuantization

    for (M, bits, dim, n, block) in CASES:
        X, Rm, C = oref.exact_case(M, bits, dim, n, block, seed=700 + M * 10 + bits)
        pq = ProductQuantization("opq", M, bits, "l2", dim, pq_init_method="none", pq_update_method="none")
        with torch.no_grad():
            pq.codebook.copy_(torch.from_numpy(C))
            pq.rotate.copy_(torch.from_numpy(Rm))
        pq.eval()
        with io.StringIO() as buf, redirect_stdout(buf):
            cluster, mapping = pq.get_document_cluster(X, 0, 1, batch_size=128, return_mapping=True)
        codes = np.array([mapping[i] for i in range(n)], dtype=np.int32)
        # the matmul is exact here: the chain, any BLAS order and float64 agree bit for bit
        Y = torch.matmul(torch.from_numpy(X), torch.from_numpy(Rm).t()).numpy()
        assert np.array_equal(Y, oref.rotate(X, Rm)) and np.array_equal(Y.astype(np.float64), X.astype(np.float64) @ Rm.astype(np.float64).T)
        unrotated = pq_ref.pq_encode(X, C)
        differ = float((unrotated != codes).any(1).mean())
        out = dict(X=X, R=Rm, C=C, codes=codes)
        for R in (5, 10):
            with torch.no_grad():
                lab, sc = pq.beam_search(torch.from_numpy(X[:64].copy()), R, return_proba=True)
            out[f"beam{R}_labels"] = lab.numpy().astype(np.int32)
            out[f"beam{R}_scores"] = sc.numpy().astype(np.float32)
        with torch.no_grad():
            rec = torch.stack([pq.get_reconstruct_vector(torch.from_numpy(codes[r].astype(np.int64))) for r in range(32)])
        out["reconstruct32"] = rec.numpy().astype(np.float32)
        keys = sorted(cluster)
        out["cluster_keys"] = np.array(keys, dtype=np.int32)
        out["cluster_sizes"] = np.array([len(cluster[k]) for k in keys], dtype=np.int32)
        out["cluster_docs"] = np.array([d for k in keys for d in cluster[k]], dtype=np.int64)
        path = os.path.join(GOLD, f"g4o_opq_{M}_{bits}_{dim}.npz")
        np.savez_compressed(path, **out)
        print("g4o", M, bits, dim, "clusters", len(keys), "rows whose unrotated pq codes differ", differ, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    os.makedirs(GOLD, exist_ok=True)
    g4o_opq()
