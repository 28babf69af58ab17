"""Passages past 256 tokens through the public stacks: the T5 encoder and tower at t5-base width, the dh-8 golden tower, a
BERT encoder at bert-base width with 512 positions, NCI beam search on a 300-token query and generate.gen_doc_embedding --
each against the float64 restatements (tests/t5_ref64.py, tests/bert_ref64.py) under the project's bar (tests/f64_bar.py:
e_hip <= 4 e_32 + 2^-22 max |ref64| over the real positions), or against the torch-fp32 oracle where the G1 tests do.
Every model here hands more than 256 keys to attention, which only ops.attention_long* accept: the tests count those calls."""
import json
import os

import numpy as np
import pytest
import torch

import bert_ref64 as b64
import t5_ref64 as r64
import test_bert_f64_gpu as BT
from f64_bar import check, refs
from mevi_amd import bert, nci, ops, t5
from oracle import t5 as ot5
from test_t5_f64_gpu import batch, cfg, dims, realistic_weights

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LENS, S = (300, 384, 257, 129, 40, 1), 384


@pytest.fixture
def calls(monkeypatch):
    """Counts the calls of the four attention entry points of mevi_amd.ops while a test runs."""
    n = {}
    for name in ("attention", "attention_varlen", "attention_long", "attention_long_varlen"):
        def counted(*a, _fn=getattr(ops, name), _name=name, **kw):
            n[_name] = n.get(_name, 0) + 1
            return _fn(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    return n


def test_t5_base_width_encoder_and_tower(cuda, calls, record_property):
    W = realistic_weights(2, 2)
    ids, mask = batch(LENS, S, seed=S)
    enc = t5.EncoderStack(W, dims(2, 0), cuda)
    emb = W["shared.weight"].to(cuda)

    def run(dt, dev):
        Wd = r64.cast(W, dt, dev)
        return r64.encoder(Wd, cfg(2, 0), Wd["shared.weight"][ids.to(dev)], mask.to(dev), n_layers=2)

    ref64, ref32 = refs(("long_t5_enc",), run)
    packed = enc.forward(emb, ids.to(cuda), mask.to(cuda), pack=True)
    assert calls == {"attention_long_varlen": 2}            # right-padded: the packed rows, no scatter
    check("long/t5_encoder/packed", packed, ref64, ref32, mask.bool(), record_property)
    calls.clear()
    padded = enc.forward(emb, ids.to(cuda), mask.to(cuda), pack=False)
    assert calls == {"attention_long": 2}
    check("long/t5_encoder/padded", padded, ref64, ref32, mask.bool(), record_property)
    valid = mask.bool()
    assert torch.equal(packed.cpu()[valid], padded.cpu()[valid])
    assert float(packed.cpu()[~valid].abs().max()) == 0.0

    hids, hmask = batch(LENS, S, seed=S, holes=True)
    assert t5.packed_offsets(hmask)[0] is None

    def run_holes(dt, dev):
        Wd = r64.cast(W, dt, dev)
        return r64.encoder(Wd, cfg(2, 0), Wd["shared.weight"][hids.to(dev)], hmask.to(dev), n_layers=2)

    h64, h32 = refs(("long_t5_enc_holes",), run_holes)
    calls.clear()
    holes = enc.forward(emb, hids.to(cuda), hmask.to(cuda), pack=True)
    assert calls == {"attention_long": 2}                   # scattered into the padded layout, the key mask with its holes
    check("long/t5_encoder/holes", holes, h64, h32, hmask.bool(), record_property)

    tower = t5.TwinTower(W, dims=dims(2, 2), device=cuda)
    calls.clear()
    reps = tower.encode_passage({"input_ids": ids, "attention_mask": mask})
    assert calls == {"attention_long_varlen": 2, "attention_long": 2}      # encoder; cross-attention over 384 packed keys

    def run_tower(dt, dev):
        return r64.tower_encode(r64.cast(W, dt, dev), cfg(2, 2), ids.to(dev), mask.to(dev))

    t64, t32 = refs(("long_t5_tower",), run_tower)
    check("long/t5_tower", reps, t64, t32, None, record_property)
    tower.encoder.pack = False                               # padded K|V with the key mask: same bits
    x = tower.encoder.forward(tower.shared, ids.to(cuda), mask.to(cuda))
    x0 = ops.gather_rows(tower.shared, torch.zeros(len(LENS), dtype=torch.int64, device=cuda))
    step = tower.decoder.step(x0, 0, tower.decoder.new_cache(len(LENS)), tower.decoder.cross_kv(x, mask.to(cuda), pack=False),
                              mask.to(cuda), 1)
    check("long/t5_tower/padded_kv", step, t64, t32, None, record_property)


def test_golden_passage_tower_with_8_wide_heads(cuda, calls, record_property):
    """The g2p golden weights (d 32, 4 heads of 8: the rows kernel) on 300-token passages."""
    g = np.load(os.path.join(GOLD, "g2p_t5_passage.npz"))
    c = json.loads(str(g["cfg"]))
    W = ot5.load_weights(g)
    lens, S_ = (300, 257, 129, 40, 1), 300
    rng = np.random.default_rng(300)
    ids = torch.from_numpy(rng.integers(0, c["vocab_size"], (len(lens), S_)))
    mask = (torch.arange(S_)[None, :] < torch.tensor(lens)[:, None]).to(torch.int64)
    tower = t5.TwinTower(nci.load_npz_weights(g), device=cuda, **c)

    def run(dt, dev):
        Wd = r64.cast(W, dt, dev)
        return r64.encoder(Wd, c, Wd["shared.weight"][ids.to(dev)], mask.to(dev)), r64.tower_encode(Wd, c, ids.to(dev), mask.to(dev))

    (e64, t64), (e32, t32) = refs(("long_g2p",), run)
    packed = tower.encoder.forward(tower.shared, ids.to(cuda), mask.to(cuda), pack=True)
    padded = tower.encoder.forward(tower.shared, ids.to(cuda), mask.to(cuda), pack=False)
    assert calls == {"attention_long_varlen": 2, "attention_long": 2}
    valid = mask.bool()
    check("long/g2p_encoder/packed", packed, e64, e32, valid, record_property)
    check("long/g2p_encoder/padded", padded, e64, e32, valid, record_property)
    assert torch.equal(packed.cpu()[valid], padded.cpu()[valid])
    holes = mask.clone()
    holes[:, 2] = 0
    holes[0, 130:140] = 0

    def run_holes(dt, dev):
        Wd = r64.cast(W, dt, dev)
        return r64.encoder(Wd, c, Wd["shared.weight"][ids.to(dev)], holes.to(dev))

    h64, h32 = refs(("long_g2p_holes",), run_holes)
    check("long/g2p_encoder/holes", tower.encoder.forward(tower.shared, ids.to(cuda), holes.to(cuda), pack=True), h64, h32,
          holes.bool(), record_property)
    reps = tower.encode_passage({"input_ids": ids, "attention_mask": mask})
    check("long/g2p_tower", reps, t64, t32, None, record_property)


def test_bert_base_width_512_positions(cuda, calls, record_property):
    lens, S_ = (512, 300, 257, 12), 512
    assert BT.POSITIONS >= 512
    W = BT.realistic_weights(2)
    ids, mask = BT.batch(lens, S_, seed=S_)
    enc = bert.BertEncoder(W, 2, BT.H, eps=BT.EPS, device=cuda)

    def run(dt, dev):
        return b64.encoder(b64.cast(W, dt, dev), BT.cfg(2), ids.to(dev), mask.to(dev), n_layers=2)

    ref64, ref32 = refs(("long_bert",), run)
    packed = enc.forward(ids.to(cuda), mask.to(cuda), pack=True)
    assert calls == {"attention_long_varlen": 2}
    check("long/bert_encoder/packed", packed, ref64, ref32, mask.bool(), record_property)
    calls.clear()
    padded = enc.forward(ids.to(cuda), mask.to(cuda), pack=False)
    assert calls == {"attention_long": 2}
    check("long/bert_encoder/padded", padded, ref64, ref32, mask.bool(), record_property)
    hids, hmask = BT.batch(lens, S_, seed=S_, holes=True)

    def run_holes(dt, dev):
        return b64.encoder(b64.cast(W, dt, dev), BT.cfg(2), hids.to(dev), hmask.to(dev), n_layers=2)

    h64, h32 = refs(("long_bert_holes",), run_holes)
    check("long/bert_encoder/holes", enc.forward(hids.to(cuda), hmask.to(cuda), pack=True), h64, h32, hmask.bool(), record_property)
    # past the position table: said so, with the table's row count
    too_long = torch.zeros((1, BT.POSITIONS + 1), dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError, match=f"position table has {BT.POSITIONS} rows"):
        enc.forward(too_long, torch.ones_like(too_long))


def test_nci_beam_search_on_a_300_token_query(cuda, calls):
    """M 3, K 8 (the G1 golden's weights), 4 beams, queries of 300 and 20 tokens: the beams of oracle.t5.nci_generate, scores
    within 1e-5 as the G1 tests hold; cross-attention of every step reads 300 packed keys with kv_div = the beams."""
    g = np.load(os.path.join(GOLD, "g1_nci_M3_K8_R10.npz"))
    c = json.loads(str(g["cfg"]))
    c.pop("beams")
    assert (c["M"], c["K"]) == (3, 8)
    R, S_ = 4, 300
    rng = np.random.default_rng(8)
    ids = np.zeros((2, S_), np.int64)
    mask = np.zeros((2, S_), np.int64)
    for i, L in enumerate((300, 20)):
        ids[i, :L - 1] = rng.integers(3, c["vocab_size"], L - 1)
        ids[i, L - 1] = 1
        mask[i, :L] = 1
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    odec, osc, oenc = ot5.nci_generate(ot5.load_weights(g), c, ids, mask, R)
    model = nci.NCIModel(nci.load_npz_weights(g), device=cuda, **c)
    dec, sc, enc, _ = model.generate(ids, mask, num_beams=R, num_return_sequences=R, max_length=c["M"] + 2)
    assert calls.get("attention_long_varlen") == c["num_layers"] and calls.get("attention_long", 0) >= c["num_decoder_layers"] * c["M"]
    valid = mask.bool()
    assert (enc.cpu() - oenc)[valid].abs().max() <= 5e-5
    assert np.array_equal(dec.cpu().numpy(), odec.numpy())
    assert np.abs(np.array(sc) - osc.numpy()).max() <= 1e-5


def test_gen_doc_embedding_at_doc_length_320(cuda, tmp_path):
    """generate.gen_doc_embedding(..., doc_length=320): exactly what one encode_passage call returns."""
    import generate

    g = np.load(os.path.join(GOLD, "g2p_t5_passage.npz"))
    c = json.loads(str(g["cfg"]))
    tower = t5.TwinTower(nci.load_npz_weights(g), device=cuda, **c)
    L, lens = 320, (320, 257, 300, 5, 128, 129, 1)
    rng = np.random.default_rng(320)
    ids = rng.integers(0, c["vocab_size"], (len(lens), L)).astype(np.int64)
    mask = (np.arange(L)[None, :] < np.array(lens)[:, None]).astype(np.int64)
    ids.tofile(tmp_path / "all_document_tokens.bin")
    mask.tofile(tmp_path / "all_document_masks.bin")
    out = str(tmp_path / "docemb.bin")
    generate.gen_doc_embedding(0, str(tmp_path), None, None, out, 4, c["d_model"], [0], L, encoder=tower)
    got = np.fromfile(out, dtype=np.float32).reshape(-1, c["d_model"])
    want = tower.encode_passage({"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask)}).cpu().numpy()
    assert got.shape == (len(lens), c["d_model"]) and np.isfinite(got).all() and np.array_equal(got, want)
