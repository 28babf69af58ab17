#!/usr/bin/env python3
"""Randomised cross-check of the BERT-family tower (mevi_amd/bert.py, mtype 'bert': coCondenser / AR2 / ERNIE, MEVI/document_encoder.py:43-44,
104-123) against oracle/bert.py (pinned to the vendored BertModel by golden G8): the golden's architecture with RANDOM weights (its own
shapes and key names), 1..all layers, random batches of ragged lengths 1..max -- reps within 5e-5, packed == padded on real tokens:
  python tools/stress_bert.py [seconds] [seed]
--base: at bert-base width instead (d 768, ff 3072, 12 x 64 heads, eps 1e-12) with the realistic_weights() and the float64 bar of
tests/test_bert_f64_gpu.py (e_hip <= 4 e_32 + 2^-22 max |ref64| against tests/bert_ref64.py): random seeds, 1..3 layers, with and
without ERNIE's task_type table, S in 8..256, random ragged / full / empty / holed masks, packed and padded:
  python tools/stress_bert.py [seconds] [seed] --base"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mevi_amd import bert, nci  # noqa: E402
from oracle import bert as obert  # noqa: E402

BASE = "--base" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--base"]
budget = float(argv[0]) if len(argv) > 0 else 120.0
rng = np.random.default_rng(int(argv[1]) if len(argv) > 1 else 0)
dev = torch.device("cuda", 0)


def base_mode():
    """Random bert-base-width towers under the float64 bar of the suite."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bert_ref64 as r64
    import test_bert_f64_gpu as T

    t0, cases, worst = time.time(), 0, 0.0
    while time.time() - t0 < budget:
        L, seed, task = int(rng.integers(1, 4)), int(rng.integers(1 << 30)), bool(rng.integers(2))
        T._CACHE.clear()
        W = T.realistic_weights(L, seed=seed, task=task)
        S = int(rng.choice([8, 32, 64, 128, 256]))
        B = int(rng.integers(1, max(2, 2048 // S)))
        kind = str(rng.choice(["ragged", "full", "short", "holes"]))
        lengths = [S if kind == "full" else int(rng.integers(1, (4 if kind == "short" else S) + 1)) for _ in range(B)]
        if B > 2 and rng.random() < 0.3:
            lengths[int(rng.integers(1, B))] = 0                        # an empty row
        ids, mask = T.batch(lengths, S, seed=seed, holes=kind == "holes" and S >= 8)
        pack = bool(rng.random() < 0.8)
        tag = dict(L=L, seed=seed, task=task, S=S, B=B, kind=kind, pack=pack, path=T._path(mask, pack))
        enc = bert.BertEncoder(W, L, T.H, eps=T.EPS, device=dev)
        got = enc.forward(ids.to(dev), mask.to(dev), pack=pack).double().cpu()
        ref64 = r64.encoder(r64.cast(W, torch.float64, dev), T.cfg(L), ids.to(dev), mask.to(dev)).cpu()
        ref32 = r64.encoder(r64.cast(W, torch.float32), T.cfg(L), ids, mask).double()
        v = mask.bool()
        e_hip, e_32 = float((got - ref64)[v].abs().max()), float((ref32 - ref64)[v].abs().max())
        bar = 4.0 * e_32 + 2.0 ** -22 * float(ref64[v].abs().max())
        worst = max(worst, e_hip / bar)
        if not bool(torch.isfinite(got[v]).all()) or e_hip > bar:
            print("BAD", tag, dict(e_hip=e_hip, e_32=e_32, bar=bar))
            sys.exit(1)
        cases += 1
        if cases % 20 == 0:
            print(f"{cases} ok ... last {tag}", flush=True)
        del enc
    print(f"{cases} random bert-base-width encoders: worst e_hip / bar {worst:.3f} (bar: 4 e_32 + 2^-22 max |ref64|)")


if BASE:
    base_mode()
    sys.exit(0)
g = np.load(os.path.join(ROOT, "tests", "golden", "g8_bert_tower.npz"))
cfg0 = json.loads(str(g["cfg"]))
W0 = nci.load_npz_weights(g)
S, vocab = g["input_ids"].shape[1], int(W0[[k for k in W0 if k.endswith("word_embeddings.weight")][0]].shape[0])
t0, cases, worst = time.time(), 0, 0.0
while time.time() - t0 < budget:
    torch.manual_seed(int(rng.integers(1 << 30)))
    L = int(rng.integers(1, cfg0["num_hidden_layers"] + 1))
    W = {}
    for k, v in W0.items():
        if "LayerNorm.weight" in k:
            W[k] = 1 + 0.1 * torch.randn_like(v)
        elif "LayerNorm.bias" in k or k.endswith(".bias"):
            W[k] = 0.05 * torch.randn_like(v)
        else:
            W[k] = torch.randn_like(v) * (float(v.std()) if v.numel() > 1 else 1.0) * float(rng.choice([0.5, 1.0, 2.0]))
    cfg = dict(cfg0, num_hidden_layers=L)
    B = int(rng.integers(1, 20))
    ids = np.zeros((B, S), np.int64)
    mask = np.zeros((B, S), np.int64)
    for i in range(B):
        n = int(rng.choice([1, 2, S, int(rng.integers(1, S + 1))]))
        ids[i, :n] = rng.integers(1, vocab, size=n)
        mask[i, :n] = 1
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    tower = bert.BertTower(W, L, cfg["num_attention_heads"], eps=cfg["layer_norm_eps"], device=dev)
    reps = tower.encode_query({"input_ids": ids, "attention_mask": mask}).cpu()
    with torch.no_grad():
        want = obert.tower_encode({k: v for k, v in W.items()}, cfg, ids, mask)
    diff = float((reps - want).abs().max() / max(1.0, float(want.abs().max())))
    worst = max(worst, diff)
    hid = tower.lm_q.forward(ids.to(dev), mask.to(dev), pack=False).cpu().numpy()
    packed = tower.lm_q.forward(ids.to(dev), mask.to(dev), pack=True).cpu().numpy()
    valid = mask.numpy().astype(bool)
    if diff > 5e-5 or not np.array_equal(packed[valid], hid[valid]):
        print("BAD", dict(L=L, B=B, diff=diff))
        sys.exit(1)
    cases += 1
    del tower
print(f"{cases} random BERT towers: reps within {worst:.2e} (relative) of the oracle, packed == padded on the real tokens")
