"""tests/t5_ref64.py (the dtype-parametrised T5 restatement the float64 GPU tests are held to) pinned to the f32 oracle
and the reference's own goldens (G2 tower, G2P passages): in float32 it reproduces oracle.t5.encoder / decoder /
tower_encode within the goldens' 5e-5; in float64 it agrees with its own float32 run to f32 rounding."""
import json
import os

import numpy as np
import pytest
import torch

import t5_ref64 as r64
from oracle import t5 as ot5

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 5e-5


def _load(name):
    g = np.load(os.path.join(GOLD, name))
    cfg = json.loads(str(g["cfg"]))
    return g, cfg, ot5.load_weights(g), torch.from_numpy(g["input_ids"]), torch.from_numpy(g["attention_mask"])


@pytest.mark.parametrize("name", ["g2_t5_tower.npz", "g2p_t5_passage.npz"])
def test_float32_restatement_reproduces_the_oracle_and_the_goldens(name):
    g, cfg, W, ids, mask = _load(name)
    W32 = r64.cast(W, torch.float32)
    enc, hs = r64.encoder(W32, cfg, W32["shared.weight"][ids], mask, return_all=True)
    oenc, ohs = ot5.encoder(W, cfg, ids, mask, return_all=True)
    assert (enc - oenc).abs().max() <= TOL
    for h, oh in zip(hs[:-1], ohs[:-1]):                        # the oracle's last entry is the normed state
        assert (h - oh).abs().max() <= TOL
    assert np.abs(enc.numpy() - g["enc_last"]).max() <= TOL
    if "enc_h1" in g.files:
        assert np.abs(hs[1].numpy() - g["enc_h1"]).max() <= TOL
    reps = r64.tower_encode(W32, cfg, ids, mask)
    assert (reps - ot5.tower_encode(W, cfg, ids, mask)).abs().max() <= TOL
    assert np.abs(reps.numpy() - g["reps"]).max() <= TOL
    # the full-prefix decoder against the oracle's on a 5-token prefix (causal self-attention, relative bias, cross-attention)
    dec_ids = torch.from_numpy(np.random.default_rng(0).integers(0, W["shared.weight"].shape[0], (ids.shape[0], 5)))
    dec = r64.decoder(W32, cfg, W32["shared.weight"][dec_ids], oenc, mask)
    odec = ot5.decoder(W, cfg, dec_ids, oenc, mask, emb="shared.weight")
    assert (dec - odec).abs().max() <= TOL


@pytest.mark.parametrize("name", ["g2_t5_tower.npz", "g2p_t5_passage.npz"])
def test_float64_restatement_agrees_with_float32_to_its_rounding(name):
    """f32 against f64 of the same arithmetic: O(1) activations through 2 layers differ by a few hundred f32 ulps at most
    (2^-24 ~ 6e-8 per operation, sums of <= 128 terms); 2e-5 * max is 300x that and still 2.5x under the goldens' bar."""
    _, cfg, W, ids, mask = _load(name)
    W32, W64 = r64.cast(W, torch.float32), r64.cast(W, torch.float64)
    for dt, Wd in ((torch.float32, W32), (torch.float64, W64)):
        assert Wd["shared.weight"].dtype == dt
    e32, h32 = r64.encoder(W32, cfg, W32["shared.weight"][ids], mask, return_all=True)
    e64, h64 = r64.encoder(W64, cfg, W64["shared.weight"][ids], mask, return_all=True)
    assert e64.dtype == torch.float64
    assert (e32.double() - e64).abs().max() <= 2e-5 * e64.abs().max()
    for a, b in zip(h32, h64):
        assert (a.double() - b).abs().max() <= 2e-5 * b.abs().max()
    t32, t64 = r64.tower_encode(W32, cfg, ids, mask), r64.tower_encode(W64, cfg, ids, mask)
    assert (t32.double() - t64).abs().max() <= 2e-5 * t64.abs().max()
    # and the f64 run is not the f32 run: the difference is rounding, not zero
    assert (e32.double() - e64).abs().max() > 0


def test_tower_step_is_the_one_position_decoder():
    """tower_step (position 0 alone: one key, the context is v) against the full-prefix decoder's first position."""
    _, cfg, W, ids, mask = _load("g2_t5_tower.npz")
    W64 = r64.cast(W, torch.float64)
    enc = r64.encoder(W64, cfg, W64["shared.weight"][ids], mask)
    x = W64["shared.weight"][torch.tensor([[0, 7, 9]] * ids.shape[0])]
    full = r64.decoder(W64, cfg, x, enc, mask)
    step = r64.tower_step(W64, cfg, x[:, 0], enc, mask)
    assert (full[:, 0] - step).abs().max() <= 1e-12 * step.abs().max()
