#!/usr/bin/env python3
"""Golden G1V: the reference's generate() under VARIABLE-DEPTH decode trees (semantic ids, --codebook 0).

Imports the read-only reference through tools/ref_import.py (build container only) and runs its own
`generate(..., decode_tree=TreeBuilder().build())` with the tree built from ids of different lengths
(MEVI/main_models.py:50-69, 83-108, 1707-1728) on the miniature G1 / G1T models.  Writes data only to
tests/golden/g1v_*.npz: the id paths, the inputs, `decoded`, `scores`, every step's last-position logits, and the name
of the G1 / G1T golden that holds the same model's weights (checked equal here).

  python tools/capture_goldens_varlen.py [case name ...]

Trees: (a) depths 1 .. M + 1 mixed (M + 1 codes leave no room for eos: such hypotheses come from the final flush),
(b) ids that are prefixes of other ids (eos beside children), (c) a narrow tree whose nodes have fewer than R live
continuations, so the -1e9-seeded beams and -inf candidates are carried, (d) short ids that fill and close the pools
before the last step (the reference then stops early: the steps it never ran are not recorded), (e) the pure-NCI shapes
(`wide`): 40 beams over ids of 2 .. 8 codes (nine decoder positions, ids that are prefixes of ids) and 100 beams over K = 30.
The wide cases borrow the weights of a G1 model whose decode vocabulary is large enough and set the model's per-position
code count (`output_vocab_size`, read at every forward: modeling_t5.py:1585) to their own K.  Only hypotheses with a finite score are
specified by the reference (ties among -inf candidates are torch.topk's choice): every case must return finite scores.
"""
import json
import os
import sys
from argparse import Namespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_import  # noqa: E402
from capture_goldens import GOLD, _synthetic_queries  # noqa: E402
from capture_goldens_qemb import _model  # noqa: E402


def _ids_mixed(rng, M, K):
    """(a) 70 ids of 1 .. M + 1 codes over a few first codes, so that short and long ids share prefixes by chance."""
    out = set()
    while len(out) < 70:
        n = int(rng.integers(1, M + 2))
        out.add(tuple(int(c) for c in rng.integers(0, min(K, 6), size=n)))
    return sorted(out)


def _ids_prefixes(rng, M, K):
    """(b) every id's proper prefixes of 2+ codes are ids as well."""
    out = set()
    for _ in range(12):
        full = tuple(int(c) for c in rng.integers(0, min(K, 5), size=M))
        for n in range(2, M + 1):
            out.add(full[:n])
    return sorted(out)


def _ids_narrow(rng, M, K):
    """(c) chains: 14 ids under two first codes, most inner nodes with a single child."""
    out = {(0,), (0, 1, 2), (0, 1, 3), (1, 4)}
    while len(out) < 14:
        out.add((int(rng.integers(0, 2)),) + tuple(int(c) for c in rng.integers(0, K, size=int(rng.integers(1, M)))))
    return sorted(out)


def _ids_shallow(rng, M, K):
    """(d) many one-code ids and a few deep ones: pools fill at the second step and close before the last one."""
    return sorted({(c,) for c in range(K)} | {(5, 9, 9), (6, 1)})


def _ids_wide_deep(rng, M, K):
    """(e) 260 ids of 2 .. M codes over all K codes at the first two levels and a few below, every id's prefix of 2+ codes
    an id with probability 1/4."""
    out = set()
    while len(out) < 260:
        n = int(rng.integers(2, M + 1))
        full = tuple(int(c) for c in rng.integers(0, K, size=2)) + tuple(int(c) for c in rng.integers(0, min(K, 3), size=n - 2))
        out.add(full)
        for m in range(2, n):
            if rng.random() < 0.25:
                out.add(full[:m])
    return sorted(out)


def _ids_wide_flat(rng, M, K):
    """(e) 700 ids of 1 .. M + 1 codes, the first code over all K."""
    out = set()
    while len(out) < 700:
        n = int(rng.integers(1, M + 2))
        out.add((int(rng.integers(0, K)),) + tuple(int(c) for c in rng.integers(0, min(K, 5), size=n - 1)))
    return sorted(out)


CASES = [  # name, (M, K, beams, model seed, golden with the weights), id maker, queries
    ("mixed", (4, 32, 10, 0, "g1_nci_M4_K32_R10.npz"), _ids_mixed, 3),
    ("prefixes", (3, 16, 4, 1, "g1_nci_M3_K16_R4.npz"), _ids_prefixes, 4),
    ("narrow", (3, 8, 10, 22, "g1t_nci_tree_M3_K8_R10_P30.npz"), _ids_narrow, 4),
    ("shallow", (3, 16, 4, 1, "g1_nci_M3_K16_R4.npz"), _ids_shallow, 4),
    # wide: (..., (M, K) the borrowed model was built with) -- K (M + 2) + 2 decode tokens must fit its vocabulary
    ("wide", (8, 8, 40, 1, "g1_nci_M3_K16_R4.npz"), _ids_wide_deep, 3, (3, 16)),
    ("wide", (4, 30, 100, 0, "g1_nci_M4_K32_R10.npz"), _ids_wide_flat, 2, (4, 32)),
]


def main():
    ref_import.setup()
    import torch
    from transformers import T5Config, T5ForConditionalGeneration
    from main_models import TreeBuilder, encode_single_newid

    only = sys.argv[1:]
    for name, (M, K, beams, seed, weights_from), make_ids, nq, *borrowed in CASES:
        if only and name not in only:
            continue
        Mm, Km = borrowed[0] if borrowed else (M, K)
        cfg, model = _model(T5Config, T5ForConditionalGeneration, torch, Mm, Km, seed)
        assert K * (M + 2) + 2 <= cfg.decode_vocab_size
        model.output_vocab_size = K
        base = np.load(os.path.join(GOLD, weights_from))
        sd = {k_: v_.detach().numpy() for k_, v_ in model.state_dict().items()}
        assert all(np.array_equal(v_, base["w." + k_]) for k_, v_ in sd.items()), weights_from
        args = Namespace(kary=K, position=1, label_length_cutoff=0, max_output_length=M + 2)
        rng = np.random.default_rng(seed + 500)
        paths = make_ids(rng, M, K)
        builder = TreeBuilder()
        for pth in paths:
            builder.add(encode_single_newid(args, list(pth)))
        root = builder.build()
        ids, mask = _synthetic_queries(rng, nq, 32, cfg.vocab_size)
        step_logits = []
        orig_forward = model.forward

        def spy(*a, **k):
            out = orig_forward(*a, **k)
            step_logits.append(out[0][:, -1, :].detach().clone())
            return out

        model.forward = spy
        kwargs = dict(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), use_cache=False,
                      max_length=M + 2, length_penalty=0.8, num_return_sequences=beams, early_stopping=False,
                      decode_embedding=2, decode_vocab_size=cfg.decode_vocab_size, decode_tree=root,
                      output_hidden_states=True, output_scores=True, decoder_integration="series",
                      decoder_attention_mask=torch.tensor([[1] * (M + 1) + [0]] * nq), num_beams=beams)
        with torch.no_grad():
            outs, scores, enc_h, _ = model.generate(**kwargs)
            again = model.generate(**kwargs)
        model.forward = orig_forward
        scores = np.array(scores, dtype=np.float64)
        assert np.isfinite(scores).all(), (name, "a hypothesis with score -inf: its tokens are unspecified")
        assert torch.equal(outs, again[0]) and np.array_equal(scores, np.array(again[1])), (name, "not deterministic")
        decoded = np.zeros((nq * beams, M + 2), np.int64)          # the reference trims to the longest hypothesis + eos
        decoded[:, :outs.shape[1]] = outs.numpy()
        steps = len(step_logits) // 2
        np.savez_compressed(
            os.path.join(GOLD, f"g1v_{name}_M{M}_K{K}_R{beams}.npz"), input_ids=ids, attention_mask=mask, decoded=decoded,
            scores=scores, paths_flat=np.array([c for pth in paths for c in pth], np.int32),
            paths_len=np.array([len(pth) for pth in paths], np.int32),
            **{f"step{t}_logits": step_logits[t].numpy() for t in range(steps)}, weights_from=np.array(weights_from),
            cfg=np.array(json.dumps(dict(M=M, K=K, beams=beams, **(dict(decode_vocab_size=cfg.decode_vocab_size) if borrowed else {}),
                                         d_model=cfg.d_model, d_ff=cfg.d_ff, num_heads=cfg.num_heads,
                                         d_kv=cfg.d_kv, num_layers=cfg.num_layers, num_decoder_layers=cfg.num_decoder_layers,
                                         adaptor_layer_num=cfg.adaptor_layer_num, vocab_size=cfg.vocab_size,
                                         layer_norm_epsilon=cfg.layer_norm_epsilon,
                                         relative_attention_num_buckets=cfg.relative_attention_num_buckets))))
        lens = (decoded[:, 1:] > 1).sum(1)
        print("g1v", name, "ids", len(paths), "steps", steps, "decoded", tuple(outs.shape), "code counts", np.bincount(lens).tolist(),
              "score range", float(scores.min()), float(scores.max()))


if __name__ == "__main__":
    os.makedirs(GOLD, exist_ok=True)
    main()
