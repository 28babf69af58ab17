"""The variable-depth beam search at 33 .. 128 beams (the 1024-thread form and the opted-in LDS included) and the
ancestor-indexed attention over 9 .. 16 cached keys: the kernels against the restatement tests/varbeam_ref.py bit for bit (the
`run_both` of test_varbeam_gpu.py), the C entry points driven directly, refusals before launch, and NCIModel.generate against
the reference's goldens g1v_wide_* (40 beams over ids of 2 .. 8 codes: nine decoder positions; 100 beams over K = 30)."""
import os

import numpy as np
import pytest
import torch

import varbeam_ref as vr
from test_varbeam_cpu import GOLD, golden_paths
from test_varbeam_gpu import _golden_model, random_ids, run_both

pytestmark = pytest.mark.gpu

WIDE = [os.path.join(GOLD, "g1v_wide_M8_K8_R40.npz"), os.path.join(GOLD, "g1v_wide_M4_K30_R100.npz")]


@pytest.mark.parametrize("T", [7, 11])
@pytest.mark.parametrize("R", [33, 64, 100, 128])
@pytest.mark.parametrize("K", [8, 30, 256])
def test_wide_kernel_matches_restatement_on_random_trees(cuda, R, K, T):
    """Every output, the pool and its state after every step, the hypotheses after finalize.  R = 128, K = 256: 129 KiB
    of candidates in LDS, the 1024-thread form; K = 8, 30: the 256-thread form."""
    rng = np.random.default_rng(1000 * R + K + T)
    B = 4 if K == 256 else 8
    for depth, n_ids, spread in ((5, 120, min(K, 5)), (3, 14, 3), (6, 400, K)):
        paths = random_ids(rng, K, depth, n_ids, spread)
        run_both(cuda, rng, R, K, T, B, paths)


@pytest.mark.parametrize("R,K", [(40, 8), (100, 30), (128, 8)])
def test_wide_exact_ties_resolve_by_flat_index(cuda, R, K):
    rng = np.random.default_rng(7 * R + K)
    paths = random_ids(rng, K, 4, 60, min(K, 6))
    qs, _, _ = run_both(cuda, rng, R, K, 6, 8, paths, quantum=1.0)
    assert qs


def test_wide_pools_fill_close_and_flush(cuda):
    """Only one-code ids (64 of them, 40 beams): after the first step every live beam can only end, the pools fill and close
    while the rows keep flowing as -inf placeholders.  A tree of T - 1 codes per id: nothing ends, everything comes from the
    flush.  A mix: done queries mid-batch.  A narrow tree at R = 100: fewer finite candidates than 2R at every step, the
    -inf placeholders in flat-index order (run_both compares their parents, codes and nodes as well)."""
    rng = np.random.default_rng(5)
    K, R, T = 64, 40, 6
    qs, done_seen, lengths = run_both(cuda, rng, R, K, T, 8, [(c,) for c in range(K)])
    assert all(q.done for q in qs) and not done_seen[0].any() and done_seen[-2].all() and (lengths == 2).all()
    deep = sorted({tuple(int(c) for c in rng.integers(0, 4, size=T - 1)) for _ in range(300)})
    qs, done_seen, lengths = run_both(cuda, rng, R, K, T, 8, deep)
    assert not any(q.done for q in qs) and (lengths == T).all()
    mix = ([(c,) for c in range(40)] + [(c, d) for c in range(40) for d in range(2)] +
           [(60 + (i % 2), i % 5, i % 7, i % 2) for i in range(40)])
    qs, done_seen, lengths = run_both(cuda, rng, R, K, T, 24, mix)
    flags = [q.done for q in qs]
    assert any(flags) and not all(flags) and lengths.min() == 2
    narrow = random_ids(rng, 8, 3, 14, 3)
    qs, _, lengths = run_both(cuda, rng, 100, 8, T, 8, narrow)
    assert all(np.isinf(q.scores).any() for q in qs)               # open beams taken from -inf candidates


@pytest.mark.parametrize("R", [1, 10, 32])
def test_entry_points_match_restatement_up_to_32_beams(cuda, R):
    """The C entry points themselves (raw pointers, anc null at p = 0) on half-integer logits (ties included): every output
    of every step, the pool (scores, insertion numbers, lengths, tokens, state) and the hypotheses against the restatement."""
    rng = np.random.default_rng(R)
    for K, T, paths in ((8, 7, random_ids(rng, 8, 5, 80, 4)), (256, 5, random_ids(rng, 256, 3, 300, 256)),
                        (30, 6, [(c,) for c in range(30)] + random_ids(rng, 30, 4, 40, 3))):
        run_both(cuda, np.random.default_rng(17 + K), R, K, T, 6, paths, quantum=0.5, direct=True)


def test_wide_refuses_unsupported_shapes_before_launch(cuda):
    from mevi_amd import hip, nci

    L = hip.lib()

    def attempt(R, K, p, T, match):
        tree = nci.RaggedPrefixTree([(0,), (1, 2)], K, cuda, levels=3)
        full = lambda shape, dt=torch.int32: torch.full(shape, 77, dtype=dt, device=cuda)         # noqa: E731
        logits = torch.zeros((R, K + 1), dtype=torch.float32, device=cuda)
        scores = torch.zeros((1, R), dtype=torch.float32, device=cuda)
        node, prefix, anc = (torch.zeros(s, dtype=torch.int32, device=cuda) for s in ((1, R), (1, R, T), (R, max(p, 1))))
        len_pow = torch.ones(T + 1, dtype=torch.float64, device=cuda)
        pool = (full((1, R), torch.float64), full((1, R)), full((1, R)), full((1, R, T)), full((1, 4)))
        out = (full((1, R), torch.float32), full((1, R)), full((1, R)), full((1, R)), full((1, R, T)), full((R, p + 1)))
        st = L.mevi_beam_step_var_f32(
            hip.ptr(logits), hip.ptr(scores), hip.ptr(node), hip.ptr(prefix), hip.ptr(anc), 1, R, K, p, T, hip.ptr(tree.mask[0]),
            hip.ptr(tree.base[0]), hip.ptr(tree.ends[0]), tree.base[0].numel(), hip.ptr(len_pow), *(hip.ptr(t) for t in pool),
            *(hip.ptr(t) for t in out), hip.stream_ptr())
        assert st != 0
        with pytest.raises(hip.MeviHipError, match=match):
            hip.check(st, "mevi_beam_step_var_f32")
        torch.cuda.synchronize()
        assert all(bool((t == 77).all()) for t in pool + out)
        return pool, out, scores, prefix, len_pow

    attempt(129, 8, 0, 4, "R <= 128")
    attempt(4, 257, 0, 4, "K <= 256")
    attempt(4, 8, 3, 4, "p \\+ 1 < T")
    attempt(4, 8, 0, 65, "T <= 64")
    pool, out, scores, prefix, len_pow = attempt(129, 8, 0, 4, "R <= 128")
    fin = (torch.full((129, 4), 77, dtype=torch.int64, device=cuda), torch.full((129,), 77.0, dtype=torch.float64, device=cuda),
           torch.full((129,), 77, dtype=torch.int32, device=cuda))
    st = L.mevi_beam_finalize_var_f32(hip.ptr(scores), hip.ptr(prefix), 1, 129, 4, hip.ptr(len_pow), *(hip.ptr(t) for t in pool),
                                      *(hip.ptr(t) for t in fin), hip.stream_ptr())
    with pytest.raises(hip.MeviHipError, match="R <= 128"):
        hip.check(st, "mevi_beam_finalize_var_f32")
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in fin + pool)


@pytest.mark.parametrize("tk", [9, 12, 16])
@pytest.mark.parametrize("H,dh", [(12, 64), (8, 96)])
def test_attention_over_9_to_16_indexed_keys_equals_the_reordered_copy(cuda, tk, H, dh):
    """mevi_attention_cached_f32 / _split_f16 with 9 .. 16 keys: identical bits to `attention` over the gathered copy of the
    caches, f32 and split-f16 image, with bias and causal mask; 7 and 70 rows (pair counts that do not fill a wave)."""
    from mevi_amd import hip, ops

    g = torch.Generator(device=cuda).manual_seed(tk * 7 + H)
    rows, T = 37, 16
    for n in (7, 70):
        cache = torch.randn((rows, T, 2 * H * dh), device=cuda, generator=g)
        q = torch.randn((n, H * dh), device=cuda, generator=g)
        bias = torch.randn((H, T, T), device=cuda, generator=g)
        key_rows = torch.randint(0, rows, (n, tk), device=cuda, generator=g).to(torch.int32)
        gathered = cache[key_rows.long(), torch.arange(tk, device=cuda)[None, :], :]          # the re-ordered copy
        kw = dict(bias=bias, q_pos0=tk - 1, causal=True, scale=1.0 if dh == 64 else dh ** -0.5)
        want = ops.attention(q.view(n, 1, -1), gathered[:, :, :H * dh], gathered[:, :, H * dh:], H, **kw).view(n, -1)
        got = ops.attention_cached(q, cache[:, :, :H * dh], cache[:, :, H * dh:], key_rows, H, **kw)
        assert torch.isfinite(got).all() and torch.equal(got, want), (n, tk, H, dh)
        bound = float(cache.abs().max())
        wimg = ops.attention(q.view(n, 1, -1), gathered[:, :, :H * dh], gathered[:, :, H * dh:], H, split_bound=bound, **kw)
        gimg = ops.attention_cached(q, cache[:, :, :H * dh], cache[:, :, H * dh:], key_rows, H, split_bound=bound, **kw)
        assert torch.equal(gimg.img, wimg.img) and torch.equal(gimg.exp.cpu(), wimg.exp.cpu()), (n, tk, H, dh, "image")
    key_rows = torch.zeros((n, 17), dtype=torch.int32, device=cuda)
    with pytest.raises(hip.MeviHipError, match="1..16 cached positions"):
        ops.attention_cached(q, cache[:, :, :H * dh], cache[:, :, H * dh:], key_rows, H, bias=None, q_pos0=16)


@pytest.mark.parametrize("path", WIDE)
def test_generate_matches_wide_reference_golden(cuda, path):
    """decoded identical, scores within the G1V bound (1e-5 * max(1, |ref|)), lengths = the eos positions; prefix tables off
    and graph replay (eager, capture, replay) give the same bits."""
    g = np.load(path)
    cfg, beams, model, tree = _golden_model(g, cuda)
    assert beams > 32
    ids, mask = torch.from_numpy(g["input_ids"]), torch.from_numpy(g["attention_mask"])
    dec, scores, enc, none, lengths = model.generate(ids, mask, num_beams=beams, num_return_sequences=beams,
                                                     max_length=cfg["M"] + 2, decode_tree=tree)
    assert none is None and dec.shape == (ids.shape[0] * beams, cfg["M"] + 2)
    assert np.array_equal(dec.cpu().numpy(), g["decoded"])
    ref = g["scores"]
    assert (np.abs(np.array(scores) - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref))).all()
    eos_at = np.array([list(row).index(1) if 1 in row else len(row) for row in g["decoded"]])
    assert np.array_equal(lengths.cpu().numpy(), eos_at)
    ids_set = set(golden_paths(g))
    for row, n in zip(dec.cpu().numpy(), eos_at):
        assert tuple(int(t) - 2 - i * cfg["K"] for i, t in enumerate(row[1:n])) in ids_set
    model.prefix_table_bytes, model._tables = 0, None
    d2, s2, _, _, l2 = model.generate(ids, mask, num_beams=beams, decode_tree=tree)
    assert torch.equal(d2, dec) and s2 == scores and torch.equal(l2, lengths)
    for _ in range(3):                                                # eager, capture, replay
        d3, s3, _, _, l3 = model.generate(ids[:2], mask[:2], num_beams=beams, decode_tree=tree, graph=True)
        assert torch.equal(d3, dec[:2 * beams]) and s3 == scores[:2 * beams] and torch.equal(l3, lengths[:2 * beams])
    with pytest.raises(NotImplementedError, match="output_dec_hidden"):
        model.generate(ids, mask, num_beams=beams, decode_tree=tree, output_dec_hidden=True)

