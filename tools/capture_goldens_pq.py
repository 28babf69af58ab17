#!/usr/bin/env python3
"""Capture the product-quantisation goldens (tests/golden/g4p_pq_*.npz) by importing the read-only reference.

Runs ONLY in the build container, like tools/capture_goldens.py: everything written is data (seeded rows and
codebooks + the reference's own outputs of ProductQuantization('pq', M, bits, 'l2')); no reference source travels.

  python tools/capture_goldens_pq.py
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

import ref_import  # noqa: E402

# (M, bits, dim, rows): the issue's two shapes, plus one whose dim leaves trailing columns (5 x 8 = 40 of 44) and whose
# K = 16 < R at the first beam step (all candidates kept)
CASES = [(4, 5, 64, 300), (8, 8, 64, 200), (5, 4, 44, 257)]


def g4p_pq():
    """get_pq_document_cluster / beam_search / get_reconstruct_vector of MEVI/pq.py with pq_type 'pq', dist_mode 'l2'."""
    ref_import.setup()
    import torch
    from pq import ProductQuantization

    for (M, bits, dim, n) in CASES:
        K = 2 ** bits
        dsub = dim // M
        rng = np.random.default_rng(400 + M * 10 + bits)
        # scale 0.25: distances of a few units, so one f32 ulp moves a beam probability by ~1e-7
        C = (0.25 * rng.standard_normal((M, K, dsub))).astype(np.float32)
        # rows near a random code path (clusters get several members) plus rows anywhere
        paths = rng.integers(0, K, size=(n, M))
        X = (0.25 * rng.standard_normal((n, dim))).astype(np.float32)
        near = rng.random(n) < 0.5
        X[near, :M * dsub] = (np.concatenate([C[j][paths[near, j]] for j in range(M)], axis=1)
                              + 0.05 * rng.standard_normal((int(near.sum()), M * dsub))).astype(np.float32)
        pq = ProductQuantization("pq", M, bits, "l2", dim, pq_init_method="none", pq_update_method="none")
        with torch.no_grad():
            pq.codebook.copy_(torch.from_numpy(C))
        pq.eval()
        with io.StringIO() as buf, redirect_stdout(buf):
            cluster, mapping = pq.get_document_cluster(X, 0, 1, batch_size=128, return_mapping=True)
        codes = np.array([mapping[i] for i in range(n)], dtype=np.int32)
        out = dict(X=X, C=C, codes=codes)
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
        path = os.path.join(GOLD, f"g4p_pq_{M}_{bits}_{dim}.npz")
        np.savez_compressed(path, **out)
        print("g4p", M, bits, dim, "clusters", len(keys), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    os.makedirs(GOLD, exist_ok=True)
    g4p_pq()
