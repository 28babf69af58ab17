#!/usr/bin/env python3
"""Capture the G1Q goldens: `--query_encoder nci` query embeddings of the reference.

Runs ONLY in the build container (imports the read-only reference through tools/ref_import.py).  For three model
configurations -- shared-sons (4, 32, R=10), (3, 16, R=4) and a generic PrefixTree (3, 8, R=10, 30 paths) -- it stores
what G1 stores plus
  dec_hidden      f32 [B*R, M+1, d]  the decoder states generate() returns, in ITS row order (the beams as they entered
                                     the final step, before the hypotheses are sorted by score)
  presort_prefix  i64 [B*R, M+1]     the decoder input of that last forward (the same row order)
  attenpool_weight / attenpool_bias  the Linear(d, 1) of --query_embed_accum attenpool
  qemb_<qtower>_<accum>  f32 [B*R, d]  T5FineTuner.clus_repr(..., flatten=True) called unbound on a stub `self`
for qtower in {enc_dec, encmask_dec, encmask, dec, encmask_dec_emb, enc_dec_emb} x accum in {maxpool, avgpool, attenpool}.
The models and inputs are those of G1 / G1T (same seeds, same construction): a G1Q file names that golden in
`weights_from` instead of carrying the weights again, and the capture asserts that both hold the same tensors and inputs.

  python tools/capture_goldens_qemb.py
"""
import io
import json
import os
import sys
from argparse import Namespace
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_import  # noqa: E402
from capture_goldens import GOLD, _mevi_t5_config, _synthetic_queries  # noqa: E402

QTOWERS = ("enc_dec", "encmask_dec", "encmask", "dec", "encmask_dec_emb", "enc_dec_emb")
ACCUMS = ("maxpool", "avgpool", "attenpool")
CONFIGS = [  # (M, K, beams, generic-tree paths or None, seed, the G1 / G1T golden of the same model and inputs)
    (4, 32, 10, None, 0, "g1_nci_M4_K32_R10.npz"),
    (3, 16, 4, None, 1, "g1_nci_M3_K16_R4.npz"),
    (3, 8, 10, 30, 22, "g1t_nci_tree_M3_K8_R10_P30.npz"),
]


def _model(T5Config, T5ForConditionalGeneration, torch, M, K, seed):
    """The G1 / G1T miniature model of this seed (same construction and parameter perturbation)."""
    torch.manual_seed(seed)
    cfg = _mevi_t5_config(T5Config, M, K)
    with io.StringIO() as buf, redirect_stdout(buf):
        model = T5ForConditionalGeneration(cfg)
    model.eval()
    with torch.no_grad():
        for n_, p_ in model.named_parameters():
            if n_.endswith("layer_norm.weight") or "final_layer_norm" in n_:
                p_.copy_(1.0 + 0.2 * torch.randn_like(p_))
            if "relative_attention_bias" in n_:
                p_.copy_(torch.randn_like(p_))
            if n_.startswith("adaptor.") and n_.endswith("bias"):
                p_.copy_(0.05 * torch.randn_like(p_))
    return cfg, model


def g1q_nci_query_embedding():
    ref_import.setup()
    import torch
    from transformers import T5Config, T5ForConditionalGeneration
    from main_models import T5FineTuner, TreeBuilder, encode_single_newid

    for (M, K, beams, npaths, seed, weights_from) in CONFIGS:
        cfg, model = _model(T5Config, T5ForConditionalGeneration, torch, M, K, seed)
        args = Namespace(kary=K, position=1, label_length_cutoff=M, max_output_length=M + 2)
        rng = np.random.default_rng(seed + 50)
        paths = None
        if npaths is None:
            builder = TreeBuilder(share_sons=True)
            newids = [encode_single_newid(args, [i for _ in range(M)]) for i in range(K)]
            for i in range(M):
                builder.add_layer([ids[i] for ids in newids])
            builder.add_layer([1])
        else:
            paths = np.unique(rng.integers(0, K, size=(npaths, M)), axis=0)
            builder = TreeBuilder()
            for pth in paths:
                builder.add(encode_single_newid(args, [int(c) for c in pth]))
        root = builder.build()
        ids, mask = _synthetic_queries(rng, 4, 32, cfg.vocab_size)
        last_input = []
        orig_forward = model.forward

        def spy(*a, **k):
            last_input[:] = [k["decoder_input_ids"].detach().clone()]
            return orig_forward(*a, **k)

        model.forward = spy
        kwargs = dict(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), use_cache=False,
                      max_length=M + 2, length_penalty=0.8, num_return_sequences=beams, early_stopping=False,
                      decode_embedding=2, decode_vocab_size=cfg.decode_vocab_size, decode_tree=root,
                      output_hidden_states=True, output_scores=True, decoder_integration="series",
                      decoder_attention_mask=torch.tensor([[1] * (M + 1) + [0]] * 4), num_beams=beams)
        with torch.no_grad():
            outs, scores, enc_h, dec_h = model.generate(**kwargs)
        model.forward = orig_forward
        presort = last_input[0]
        assert tuple(dec_h.shape) == (4 * beams, M + 1, cfg.d_model), dec_h.shape
        assert tuple(presort.shape) == (4 * beams, M + 1), presort.shape
        # the golden pins the pairing quirk only if a query's final sort moves its beams, and plain `enc` only if pads exist
        moved = [(presort[b * beams:(b + 1) * beams] != outs[b * beams:(b + 1) * beams, :M + 1]).any().item() for b in range(4)]
        assert any(moved), "no query's final sort permutes its beams: pick another seed"
        assert (mask == 0).any(), "no padded position"
        # --query_embed_accum attenpool's projection (T5FineTuner.__init__: torch.nn.Linear(d_model, 1)), made peaky
        torch.manual_seed(seed + 100)
        atten = torch.nn.Linear(cfg.d_model, 1)
        with torch.no_grad():
            atten.weight.mul_(8.0)
            atten.bias.fill_(0.3)
        res = {}
        for qtower in QTOWERS:
            for accum in ACCUMS:
                stub = Namespace(args=Namespace(query_embed_accum=accum, qtower=qtower.split("_"), label_length_cutoff=M),
                                 attenpool_weight=atten if accum == "attenpool" else None, model=model)
                with torch.no_grad():
                    q = T5FineTuner.clus_repr(stub, enc_h.clone(), torch.from_numpy(mask), None, dec_h.clone(),
                                              outs[:, -2], flatten=True)
                assert tuple(q.shape) == (4 * beams, cfg.d_model) and torch.isfinite(q).all(), (qtower, accum)
                res[f"qemb_{qtower}_{accum}"] = q.numpy().astype(np.float32)
        sd = {k_: v_.detach().numpy() for k_, v_ in model.state_dict().items()}
        base = np.load(os.path.join(GOLD, weights_from))      # the same model and inputs: keep one copy of the weights
        assert sorted("w." + k_ for k_ in sd) == sorted(k_ for k_ in base.files if k_.startswith("w."))
        assert all(np.array_equal(v_, base["w." + k_]) for k_, v_ in sd.items()), weights_from
        assert np.array_equal(ids, base["input_ids"]) and np.array_equal(mask, base["attention_mask"])
        assert np.array_equal(outs.numpy(), base["decoded"]), weights_from
        name = f"g1q_nci_M{M}_K{K}_R{beams}" + ("" if paths is None else f"_P{len(paths)}")
        np.savez_compressed(
            os.path.join(GOLD, name + ".npz"),
            input_ids=ids, attention_mask=mask, decoded=outs.numpy(), scores=np.array(scores, dtype=np.float64),
            enc_hidden=enc_h[::beams].numpy(), dec_hidden=dec_h.numpy(), presort_prefix=presort.numpy(),
            attenpool_weight=atten.weight.detach().numpy().reshape(-1), attenpool_bias=atten.bias.detach().numpy(),
            **({} if paths is None else {"paths": paths.astype(np.int32)}),
            **res, weights_from=np.array(weights_from),
            cfg=np.array(json.dumps(dict(M=M, K=K, beams=beams, d_model=cfg.d_model, d_ff=cfg.d_ff,
                                         num_heads=cfg.num_heads, d_kv=cfg.d_kv, num_layers=cfg.num_layers,
                                         num_decoder_layers=cfg.num_decoder_layers,
                                         adaptor_layer_num=cfg.adaptor_layer_num, vocab_size=cfg.vocab_size,
                                         layer_norm_epsilon=cfg.layer_norm_epsilon,
                                         relative_attention_num_buckets=cfg.relative_attention_num_buckets))))
        print("g1q", name, "moved queries", sum(moved), "pads", int((mask == 0).sum()))


if __name__ == "__main__":
    os.makedirs(GOLD, exist_ok=True)
    g1q_nci_query_embedding()
