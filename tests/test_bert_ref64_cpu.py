"""tests/bert_ref64.py (the dtype-generic BERT restatement the float64 GPU tests are held to) pinned to the f32 oracle and
the reference's own golden G8: in float32 it reproduces oracle.bert.encoder / tower_encode and the golden within the
golden's 5e-5; in float64 it agrees with its own float32 run to f32 rounding; the ERNIE task_type table is the same model
with the table's row 0 added to the token-type row."""
import json
import os

import numpy as np
import torch

import bert_ref64 as r64
from oracle import bert as obert

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 5e-5


def _load():
    g = np.load(os.path.join(GOLD, "g8_bert_tower.npz"))
    cfg = json.loads(str(g["cfg"]))
    return g, cfg, obert.load_weights(g), torch.from_numpy(g["input_ids"]), torch.from_numpy(g["attention_mask"])


def test_float32_restatement_reproduces_the_oracle_and_the_golden():
    g, cfg, W, ids, mask = _load()
    valid = mask.bool()
    W32 = r64.cast(W, torch.float32)
    hid, hs = r64.encoder(W32, cfg, ids, mask, return_all=True)
    assert hid.dtype == torch.float32 and len(hs) == cfg["num_hidden_layers"] + 1 and hs[-1] is hid
    ohid = obert.encoder(W, cfg, ids, mask)
    assert (hid - ohid)[valid].abs().max() <= TOL
    assert np.abs(hid.numpy() - g["hidden"])[valid.numpy()].max() <= TOL          # padded positions are not defined outputs
    for n in range(1, cfg["num_hidden_layers"] + 1):                              # n_layers: the oracle cut to n layers
        cut = r64.encoder(W32, cfg, ids, mask, n_layers=n)
        assert torch.equal(cut, hs[n])
        assert (cut - obert.encoder(W, dict(cfg, num_hidden_layers=n), ids, mask))[valid].abs().max() <= TOL
    reps = r64.tower_encode(W32, cfg, ids, mask)
    assert (reps - obert.tower_encode(W, cfg, ids, mask)).abs().max() <= TOL
    assert np.abs(reps.numpy() - g["reps"]).max() <= TOL


def test_float64_restatement_agrees_with_float32_to_its_rounding():
    """f32 against f64 of the same arithmetic: O(1) activations through 2 layers differ by a few hundred f32 ulps at most
    (2^-24 ~ 6e-8 per operation, sums of <= 96 terms); 2e-5 * max is 300x that and still 2.5x under the golden's bar (the
    statement and the number of test_t5_ref64_cpu.py)."""
    _, cfg, W, ids, mask = _load()
    valid = mask.bool()
    W32, W64 = r64.cast(W, torch.float32), r64.cast(W, torch.float64)
    for dt, Wd in ((torch.float32, W32), (torch.float64, W64)):
        assert all(v.dtype == dt for v in Wd.values())
    e32, h32 = r64.encoder(W32, cfg, ids, mask, return_all=True)
    e64, h64 = r64.encoder(W64, cfg, ids, mask, return_all=True)
    assert e64.dtype == torch.float64 and all(h.dtype == torch.float64 for h in h64)
    for a, b in zip(h32, h64):
        assert (a.double() - b)[valid].abs().max() <= 2e-5 * b[valid].abs().max()
    t32, t64 = r64.tower_encode(W32, cfg, ids, mask), r64.tower_encode(W64, cfg, ids, mask)
    assert t64.dtype == torch.float64
    assert (t32.double() - t64).abs().max() <= 2e-5 * t64.abs().max()
    # and the f64 run is not the f32 run: the difference is rounding, not zero
    assert (e32.double() - e64)[valid].abs().max() > 0


def test_task_type_table_adds_its_row_zero_to_the_type_row():
    """ERNIE with use_task_id (task_type_ids = 0): the model with a task_type_embeddings table equals the model whose type
    row is token_type_embeddings[0] + task_type_embeddings[0], and differs from the model without the table."""
    _, cfg, W, ids, mask = _load()
    W64 = r64.cast(W, torch.float64)
    d = W64["embeddings.word_embeddings.weight"].shape[1]
    task = torch.randn(3, d, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 0.3
    with_table = dict(W64)
    with_table[r64.TASK] = task
    folded = dict(W64)
    tt = W64["embeddings.token_type_embeddings.weight"].clone()
    tt[0] += task[0]
    folded["embeddings.token_type_embeddings.weight"] = tt
    a, ha = r64.encoder(with_table, cfg, ids, mask, return_all=True)
    b, hb = r64.encoder(folded, cfg, ids, mask, return_all=True)
    for x, y in zip(ha, hb):
        assert (x - y).abs().max() <= 1e-12 * y.abs().max()
    ra, rb = r64.tower_encode(with_table, cfg, ids, mask), r64.tower_encode(folded, cfg, ids, mask)
    assert (ra - rb).abs().max() <= 1e-12 * rb.abs().max()
    plain = r64.encoder(W64, cfg, ids, mask)
    assert (a - plain)[mask.bool()].abs().max() > 1e-3 * plain.abs().max()        # the table is not ignored


def test_the_float64_bar_catches_the_mutations_it_is_meant_for(monkeypatch):
    """The float32 restatement stands in for the HIP tower at bert-base width (weights, batch and bar of
    tests/test_bert_f64_gpu.py), with one fault at a time: no type row (cvec dropped), scale 1 instead of 1/8, no value
    bias, tanh-GELU, eps 1e-5.  Each must miss the bar of the embedding block or of the one-layer encoder by more than the
    bar itself, so that a kernel that is within the bar of float64 apart from the fault still fails its GPU test."""
    import math

    import test_bert_f64_gpu as T

    W = T.realistic_weights(1)
    ids, mask, _ = T._regime("packed_le32")
    valid, c = mask.bool(), T.cfg(1)
    ref64 = r64.encoder(r64.cast(W, torch.float64), c, ids, mask, return_all=True)[1]
    ref32 = r64.encoder(W, c, ids, mask, return_all=True)[1]

    def err(hs, i):
        return (hs[i].double() - ref64[i])[valid].abs().max().item()

    bars = [4.0 * err(ref32, i) + 2.0 ** -22 * ref64[i][valid].abs().max().item() for i in (0, 1)]
    assert all(err(ref32, i) <= bars[i] for i in (0, 1))

    def caught(Wm, cm=c):
        hs = r64.encoder(Wm, cm, ids, mask, return_all=True)[1]
        return [err(hs, i) > 2 * bars[i] for i in (0, 1)]

    p = "encoder.layer.0.attention.self."
    no_type = dict(W)
    no_type["embeddings.token_type_embeddings.weight"] = torch.zeros_like(W["embeddings.token_type_embeddings.weight"])
    assert caught(no_type) == [True, True]
    scale1 = dict(W)                                    # q k^T without the 1/8: the query projection times 8, exactly
    scale1[p + "query.weight"], scale1[p + "query.bias"] = W[p + "query.weight"] * 8, W[p + "query.bias"] * 8
    assert caught(scale1) == [False, True]
    no_vbias = dict(W)
    no_vbias[p + "value.bias"] = torch.zeros(T.D)
    assert caught(no_vbias) == [False, True]
    assert caught(W, dict(c, layer_norm_eps=1e-5))[0]   # the embedding block: the row of the all-zero word row
    monkeypatch.setattr(r64, "gelu", lambda h: 0.5 * h * (1 + torch.tanh(math.sqrt(2 / math.pi) * (h + 0.044715 * h ** 3))))
    assert caught(W) == [False, True]
