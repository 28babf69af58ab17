"""The BERT tower of mevi_amd/bert.py at bert-base width (d 768, ff 3072, 12 x 64 heads, eps 1e-12, 512 positions) against
the float64 restatement (tests/bert_ref64.py) applied to the same f32 inputs -- every attention route BertEncoder.forward
dispatches to (the padded masked image kernel, the three packed dh = 64 kernels, the scatter route with f32 contexts up to
256 keys), 6 to ~18 000 real tokens (latency GEMMs and the tile stream with bias / GELU epilogues), the embedding block
alone (the dim == 768 LayerNorm branch with cvec and eps 1e-12, with and without ERNIE's task_type table), the 12-layer
stack and tower, the f32-context A/B switch, and batch invariance of the tower's bits.

Bar.  That of tests/test_t5_f64_gpu.py, unchanged (tests/f64_bar.py): with e_hip = max |hip - ref64| and
e_32 = max |ref32 - ref64| over the real positions (ref32 = the same restatement in float32 on the host),

    e_hip <= 4 e_32 + 2^-22 max |ref64|.

The derivation in that module's docstring carries over: split GEMMs within the f32 chain's own error, operand images that
keep 22 bits under a bound above the row's max (here ctx_bound with the LayerNorm bias and the value bias), softmax as an
f32 operation.  The BERT-specific terms are of the same kind: erf in f32 (the GELU epilogue) and LayerNorm's two reductions
(mean, then the biased variance of the centred row) are each a few f32 ulps, as the host's f32 run makes them -- covered by
the factor 4 on e_32; the GELU epilogue writes the next GEMM's image, the 2^-22 term.  e_32 is measured at the depth of
the case, so the 12-layer cases carry the depth.  Both numbers and the bar are recorded with record_property.

Weights.  Nobody here has a real checkpoint; realistic_weights() ASSUMES the following statistics of trained BERT-family
checkpoints, which a seeded N(0, sigma) initialiser lacks:
  * LayerNorm weights log-normal around 1 (sigma 0.3), four entries of 3..10 and four near 0.05 per LayerNorm;
  * LayerNorm biases N(0, 0.1), with +-2..5 on the channels of the large weights;
  * four residual channels (OUTLIERS) whose pre-norm values are 20..50x the rest: in the word / position / type rows and in
    the rows of attention.output.dense / output.dense that write them;
  * linear biases N(0, 0.05), four value-bias entries of +-1 per layer (v_bias matters in ctx_bound);
  * query / key weights with a per-head gain: heads whose scores reach +-30 before the softmax (peaked rows) next to heads
    whose rows are nearly flat (gain 0.02);
  * word row 0 all zero (padding_idx); token 0 is a real token in every batch (its row is position + type only)."""
import numpy as np
import pytest
import torch

import bert_ref64 as r64
from f64_bar import check, refs
from mevi_amd import bert, ops, t5

pytestmark = pytest.mark.gpu
D, FF, H, DH = 768, 3072, 12, 64
VOCAB, POSITIONS, EPS = 600, 512, 1e-12
OUTLIERS = (5, 111, 400, 700)
# per head, on query AND key rows: unit gain gives scores of +-5..7 on LayerNorm outputs with these statistics, so 2.2 reaches
# +-30 (peaked rows) and 0.02 stays within +-0.01 (flat rows)
HEAD_GAIN = (2.2, 0.02, 1.0, 2.2, 0.02, 2.2, 0.3, 1.0, 0.02, 2.2, 2.2, 0.3)
_CACHE = {}


def cfg(n):
    return dict(num_attention_heads=H, layer_norm_eps=EPS, num_hidden_layers=n)


def realistic_weights(n_layers=12, seed=0, task=False):
    """state_dict-named weights (CPU f32) with the statistics assumed in the module docstring.  Layers are drawn one after
    the other, so the first layers of a deeper model are the shallower model's; task: ERNIE's task_type_embeddings table."""
    key = ("w", n_layers, seed, task)
    if key in _CACHE:
        return _CACHE[key]
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=g)           # noqa: E731
    sign = lambda n: torch.where(ru(n) < 0.5, -1.0, 1.0)  # noqa: E731
    big = torch.ones(D)
    big[list(OUTLIERS)] = 20 + 30 * ru(len(OUTLIERS))

    def ln(name, W):
        w = torch.exp(0.3 * rn(D))
        b = 0.1 * rn(D)
        ch = torch.randperm(D, generator=g)[:8]
        w[ch[:4]] = 3 + 7 * ru(4)
        b[ch[:4]] = sign(4) * (2 + 3 * ru(4))
        w[ch[4:]] = 0.05 * (1 + 0.2 * rn(4))
        W[name + ".weight"], W[name + ".bias"] = w, b

    W = {}
    word = rn(VOCAB, D) * (0.5 + ru(VOCAB, 1)) * big
    word[0] = 0
    W["embeddings.word_embeddings.weight"] = word
    W["embeddings.position_embeddings.weight"] = 0.5 * rn(POSITIONS, D) * big
    W["embeddings.token_type_embeddings.weight"] = 0.3 * rn(2, D) * big
    ln("embeddings.LayerNorm", W)
    gain = torch.tensor(HEAD_GAIN).repeat_interleave(DH)[:, None]
    for l in range(n_layers):
        p = f"encoder.layer.{l}."
        for n in ("query", "key", "value"):
            W[p + f"attention.self.{n}.weight"] = rn(D, D) * D ** -0.5 * (gain if n != "value" else 1.0)
            W[p + f"attention.self.{n}.bias"] = 0.05 * rn(D)
        vb = W[p + "attention.self.value.bias"]
        vb[torch.randperm(D, generator=g)[:4]] = sign(4)
        W[p + "attention.output.dense.weight"] = rn(D, D) * D ** -0.5 * big[:, None]
        W[p + "attention.output.dense.bias"] = 0.05 * rn(D)
        ln(p + "attention.output.LayerNorm", W)
        W[p + "intermediate.dense.weight"] = rn(FF, D) * D ** -0.5
        W[p + "intermediate.dense.bias"] = 0.05 * rn(FF)
        W[p + "output.dense.weight"] = rn(D, FF) * FF ** -0.5 * big[:, None]
        W[p + "output.dense.bias"] = 0.05 * rn(D)
        ln(p + "output.LayerNorm", W)
    if task:
        W[r64.TASK] = 0.3 * torch.randn(3, D, generator=torch.Generator().manual_seed(seed + 1000))
    _CACHE[key] = W
    return W


def batch(lengths, S, seed, holes=False):
    """ids i64 [B, S] (token 0, the all-zero word row, is real in every batch), right-padded mask (or one with holes)."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, VOCAB, (len(lengths), S))
    mask = np.zeros((len(lengths), S), np.int64)
    for i, L in enumerate(lengths):
        mask[i, :L] = 1
    first = next(i for i, L in enumerate(lengths) if L > 0)
    ids[first, min(1, lengths[first] - 1)] = 0
    if holes:
        mask[:, 1] = 0
        mask[0, 2] = 0
        ids[first, 3] = 0
    return torch.from_numpy(ids), torch.from_numpy(mask)


_LE32 = [3 + (7 * i) % 30 for i in range(22)]
REGIMES = {
    # name: (lengths, S, pack, expected route)
    "padded": ([32, 5, 17, 32, 9, 30], 32, False, "padded"),
    "dense_fill": ([32, 30, 31, 32, 30, 32], 32, True, "padded"),
    "latency": ([6], 8, True, "mfma16"),
    "packed_le32": (_LE32, 32, True, "mfma16"),
    "packed_33_64": ([33 + (11 * i) % 27 for i in range(7)] + [64], 64, True, "varlen_short"),
    "passages_65_128": ([65 + (13 * i) % 50 for i in range(5)] + [128], 128, True, "h16"),
    "long_129_256": ([129, 256, 200, 180], 256, True, "scatter"),
    "holes": ([32, 20, 31, 12, 28, 30], 32, True, "scatter"),
    "empty_row": (_LE32[:9] + [0] + _LE32[10:], 32, True, "mfma16"),
    "tokens_20k": ([90 + (7 * i) % 36 for i in range(168)], 128, True, "h16"),
}


def _path(mask, pack):
    """The route BertEncoder.forward takes for this mask: its 0.9 fill rule, packed_offsets and varlen_ok."""
    n = int((mask != 0).sum())
    if not pack or n == 0 or n > 0.9 * mask.numel():
        return "padded"
    seq_off, longest = t5.packed_offsets(mask)
    if seq_off is None or not t5.varlen_ok(longest, DH):
        return "scatter"
    return "mfma16" if longest <= 32 else ("varlen_short" if longest <= 64 else "h16")


def _regime(name):
    lengths, S, pack, path = REGIMES[name]
    ids, mask = batch(lengths, S, seed=len(lengths) + S, holes=name == "holes")
    assert _path(mask, pack) == path, (name, _path(mask, pack))
    return ids, mask, pack


def _refs(key, W, n, ids, mask, fn=r64.encoder):
    def run(dt, dev):
        return fn(r64.cast(W, dt, dev), cfg(n), ids.to(dev), mask.to(dev), n_layers=n)

    return refs(("bert",) + key, run)


def test_regimes_cover_the_dispatch():
    routes = {}
    for name, (lengths, S, pack, path) in REGIMES.items():
        _, mask, _ = _regime(name)
        routes[name] = (path, int(mask.sum(1).max()), int(mask.sum()))
    assert routes["long_129_256"][1] == 256 and routes["tokens_20k"][2] > 17000
    assert 32 < routes["packed_33_64"][1] <= 64 < routes["passages_65_128"][1] <= 128
    assert {r[0] for r in routes.values()} == {"padded", "mfma16", "varlen_short", "h16", "scatter"}


@pytest.mark.parametrize("regime", list(REGIMES))
def test_encoder_layer_against_float64(cuda, regime, record_property):
    """One BertLayer behind the embedding block (BertEncoder with one layer) in each regime of the dispatch."""
    ids, mask, pack = _regime(regime)
    W = realistic_weights(1)
    enc = bert.BertEncoder(W, 1, H, eps=EPS, device=cuda)
    assert enc.layers[0]["vb"] is not None and enc.dh == DH
    got = enc.forward(ids.to(cuda), mask.to(cuda), pack=pack)
    ref64, ref32 = _refs(("enc1", regime), W, 1, ids, mask)
    valid = mask.bool()
    if regime == "empty_row":
        empty = int((mask.sum(1) == 0).nonzero()[0])
        assert bool(torch.isfinite(got[empty]).all()) and float(got[empty].abs().max()) == 0.0
    if pack and _path(mask, pack) != "padded":
        assert float(got.cpu()[~valid].abs().max()) == 0.0            # packed: padded positions of the result are 0
    check(f"bert_layer/{regime}", got, ref64, ref32, valid, record_property)


@pytest.mark.parametrize("regime", ["packed_le32", "padded"])
def test_encoder_layer_with_f32_contexts_against_float64(cuda, monkeypatch, regime, record_property):
    """The A/B switch: attention contexts as f32 rows + split_rows instead of the o-projection's image, same bar -- a miss
    above that this case does not share is the context image's."""
    monkeypatch.setattr(ops, "CTX_IMAGE", False)
    ids, mask, pack = _regime(regime)
    W = realistic_weights(1)
    enc = bert.BertEncoder(W, 1, H, eps=EPS, device=cuda)
    assert enc.layers[0]["vb"] is None
    got = enc.forward(ids.to(cuda), mask.to(cuda), pack=pack)
    ref64, ref32 = _refs(("enc1", regime), W, 1, ids, mask)
    check(f"bert_layer_f32_ctx/{regime}", got, ref64, ref32, mask.bool(), record_property)


@pytest.mark.parametrize("task", [False, True], ids=["bert", "ernie_task_type"])
def test_embedding_block_against_float64(cuda, task, record_property):
    """gather_rows + add_layernorm(..., cvec=type0) alone on the packed_le32 batch: the dim == 768 branch with cvec and eps
    1e-12; with a task_type_embeddings table its row 0 is folded into type0."""
    ids, mask, _ = _regime("packed_le32")
    W = realistic_weights(0, task=task)
    enc = bert.BertEncoder(W, 0, H, eps=EPS, device=cuda)
    t0 = W["embeddings.token_type_embeddings.weight"][0] + (W[r64.TASK][0] if task else 0)
    assert torch.equal(enc.type0.cpu(), t0)
    S = ids.shape[1]
    idx = torch.nonzero(mask.reshape(-1) != 0).view(-1).to(cuda)
    x = ops.gather_rows(enc.word, ids.to(cuda).reshape(-1)[idx])
    got = ops.add_layernorm(x, ops.gather_rows(enc.pos, idx % S), enc.emb_ln[0], enc.emb_ln[1], eps=EPS, cvec=enc.type0)

    def run(dt, dev, W=W):
        return r64.embed(r64.cast(W, dt, dev), cfg(0), ids.to(dev))

    ref64, ref32 = refs(("bert", "embed", task), run)
    valid = mask.bool()
    check(f"bert_embeddings/{'ernie_task_type' if task else 'bert'}", got, ref64[valid.to(ref64.device)], ref32[valid], None,
          record_property)
    assert torch.equal(got, enc.forward(ids.to(cuda), mask.to(cuda))[valid.to(cuda)])      # what a 0-layer forward returns
    if task:                                                                               # and the table is not ignored
        plain = refs(("bert", "embed", False), lambda dt, dev: run(dt, dev, realistic_weights(0)))[0]
        assert float((ref64 - plain)[valid.to(ref64.device)].abs().max()) > 1e-2


def _tower12(cuda):
    if "tower12" not in _CACHE:
        _CACHE["tower12"] = bert.BertTower(realistic_weights(12), 12, H, eps=EPS, device=cuda)
    return _CACHE["tower12"]


@pytest.mark.parametrize("regime", ["packed_le32", "passages_65_128"])
def test_twelve_layer_stack_and_tower_against_float64(cuda, regime, record_property):
    """Depth: last_hidden_state of the 12-layer stack on the real positions and BertTower.encode_query's reps, same formula;
    e_32 is the f32 run through the 12 layers."""
    ids, mask, _ = _regime(regime)
    W = realistic_weights(12)
    tower = _tower12(cuda)
    ref64, ref32 = _refs(("enc12", regime), W, 12, ids, mask)
    got = tower.lm_q.forward(ids.to(cuda), mask.to(cuda))
    check(f"bert_stack_12/{regime}", got, ref64, ref32, mask.bool(), record_property)
    tower.batch_size = None
    reps = tower.encode_query({"input_ids": ids, "attention_mask": mask})
    assert reps.shape == (ids.shape[0], D)
    check(f"bert_tower_12/{regime}", reps, ref64[:, 0], ref32[:, 0], None, record_property)


def test_tower_bits_do_not_depend_on_batch_grouping_or_stale_memory(cuda):
    """1500 queries of 3..28 tokens through the 12-layer tower: bit-identical reps in one pass and in groups of 96 / 700
    (GEMM tile shapes, packed token counts and attention grids all change; every group stays on the packed <= 32-key
    kernel), and again with the allocator's free blocks filled with NaN (no kernel reads memory it did not write)."""
    nq, S = 1500, 32
    rng = np.random.default_rng(7)
    ids, mask = batch([int(n) for n in rng.integers(3, 29, nq)], S, seed=8)
    for b in (2048, 96, 700):
        for a in range(0, nq, b):
            assert _path(mask[a:a + b], True) == "mfma16"
    tower = _tower12(cuda)
    qry = {"input_ids": ids, "attention_mask": mask}

    def emb(b):
        tower.batch_size = b
        return tower.encode_query(qry)

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(cuda)
    base = torch.cuda.memory_allocated(cuda)
    e0 = emb(2048)
    assert e0.shape == (nq, D) and bool(torch.isfinite(e0).all())
    for b in (96, 700):
        assert torch.equal(emb(b), e0)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated(cuda) - base              # what the passes allocated at their peak
    torch.cuda.empty_cache()
    piece = max(1 << 20, used // 2)
    junk = [torch.full((piece // 4,), float("nan"), device=cuda) for _ in range(6)]      # 3x that, as free blocks
    del junk
    assert torch.equal(emb(700), e0) and torch.equal(emb(96), e0)
    tower.batch_size = None


def test_tower_host_side(cuda):
    """encode_query on an empty batch returns (0, 768); with weights_p the passage side runs the second weight set."""
    Wq, Wp = realistic_weights(1), realistic_weights(1, seed=1)
    tower = bert.BertTower(Wq, 1, H, weights_p=Wp, eps=EPS, device=cuda)
    assert tower.lm_p is not tower.lm_q and tower.dim == D
    none = {"input_ids": torch.zeros((0, 32), dtype=torch.int64), "attention_mask": torch.zeros((0, 32), dtype=torch.int64)}
    for out in (tower.encode_query(none), tower.encode_passage(none)):
        assert out.shape == (0, D) and out.is_cuda
    ids, mask, _ = _regime("packed_le32")
    qry = {"input_ids": ids, "attention_mask": mask}
    q, p = tower.encode_query(qry), tower.encode_passage(qry)
    assert torch.equal(p, bert.BertTower(Wp, 1, H, eps=EPS, device=cuda).encode_query(qry))
    assert torch.equal(q, bert.BertTower(Wq, 1, H, eps=EPS, device=cuda).encode_passage(qry))        # tied: one model
    assert float((p - q).abs().max()) > 1e-2
