"""Variable-depth beam search (semantic ids, --codebook 0) without a GPU: the restatement tests/varbeam_ref.py against the
reference's goldens G1V (tools/capture_goldens_varlen.py), and the level arrays of nci.RaggedPrefixTree against a
brute-force trie."""
import glob
import json
import os

import numpy as np
import pytest

import varbeam_ref as vr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G1V = sorted(glob.glob(os.path.join(GOLD, "g1v_*.npz")))


def golden_paths(g):
    flat, lens = g["paths_flat"], g["paths_len"]
    offs = np.concatenate([[0], np.cumsum(lens)])
    return [tuple(int(c) for c in flat[a:b]) for a, b in zip(offs[:-1], offs[1:])]


def golden_search(g, dtype=np.float32):
    """The restatement fed the reference's own step logits (its beams are the reference's as long as it agrees with it)."""
    cfg = json.loads(str(g["cfg"]))
    M, K, R = cfg["M"], cfg["K"], cfg["beams"]
    B = g["input_ids"].shape[0]
    root = vr.build_trie(golden_paths(g))

    def step_lsm(p, qs):
        if f"step{p}_logits" not in g.files:           # the reference stopped: every query was done
            assert all(q.done for q in qs)
            return np.zeros((B, R, K + 1), np.float32)
        cols = [1] + list(range(2 + p * K, 2 + (p + 1) * K))
        logits = g[f"step{p}_logits"][:, cols]
        return np.stack([vr.log_softmax_wave(row) for row in logits]).reshape(B, R, K + 1)

    return vr.search(root, step_lsm, B, R, K, M + 2, 0.8, dtype)


def test_goldens_exist():
    assert len(G1V) >= 3


@pytest.mark.parametrize("path", G1V)
def test_restatement_matches_reference_golden(path):
    """Tokens identical, scores within the G1 / G1T tolerance (1e-5, relative above 1)."""
    g = np.load(path)
    decoded, scores, lengths, _ = golden_search(g)
    assert np.array_equal(decoded, g["decoded"])
    ref = g["scores"]
    assert (np.abs(scores - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref))).all()
    eos_at = np.array([list(row).index(1) if 1 in row else len(row) for row in g["decoded"]])
    assert np.array_equal(lengths, eos_at)


def test_goldens_cover_early_done_and_final_flush():
    """One query whose pool is full and closed before the last step, one that is still open after it (the flush adds its
    beams, hypotheses of max_length tokens without eos), and ids ending at inner nodes."""
    early = flush = inner_end = False
    for path in G1V:
        g = np.load(path)
        cfg = json.loads(str(g["cfg"]))
        M, K, R = cfg["M"], cfg["K"], cfg["beams"]
        B = g["input_ids"].shape[0]
        root = vr.build_trie(golden_paths(g))
        done_at = [None] * B

        def step_lsm(p, qs, g=g, K=K, R=R, B=B, done_at=done_at):
            for b, q in enumerate(qs):
                if q.done and done_at[b] is None:
                    done_at[b] = p
            if f"step{p}_logits" not in g.files:
                return np.zeros((B, R, K + 1), np.float32)
            cols = [1] + list(range(2 + p * K, 2 + (p + 1) * K))
            return np.stack([vr.log_softmax_wave(row) for row in g[f"step{p}_logits"][:, cols]]).reshape(B, R, K + 1)

        decoded, _, lengths, qs = vr.search(root, step_lsm, B, R, K, M + 2, 0.8)
        early |= any(d is not None for d in done_at)
        flush |= any(not q.done for q in qs) and bool((lengths == M + 2).any())
        paths = set(golden_paths(g))
        inner_end |= any(p[:n] in paths for p in paths for n in range(1, len(p)))
    assert early and flush and inner_end


@pytest.mark.parametrize("seed", range(6))
def test_ragged_tree_arrays_match_a_brute_force_trie(seed):
    import torch

    from mevi_amd import nci

    rng = np.random.default_rng(seed)
    K = [4, 30, 33, 64, 200, 256][seed]
    D = int(rng.integers(1, 7))
    n = int(rng.integers(1, 400))
    spread = int(rng.integers(1, min(K, 6) + 1))
    paths = [tuple(int(c) for c in rng.integers(0, spread if rng.random() < 0.8 else K, size=int(rng.integers(1, D + 1))))
             for _ in range(n)]
    paths += paths[:3]                                             # duplicates
    for cutoff, levels in ((None, D + 1), (max(1, D - 1), D), (None, None)):
        tree = nci.RaggedPrefixTree(paths, K, "cpu", cutoff=cutoff, levels=levels)
        n_levels = len(tree.mask)
        want, counts = vr.trie_levels(vr.build_trie(paths, cutoff), K, n_levels)
        assert tree.n_nodes == counts
        assert tree.depth == max(len(p[:cutoff]) for p in paths)
        for p in range(n_levels):
            mask, base, ends = want[p]
            assert np.array_equal(tree.mask[p].numpy().view(np.uint32), mask), (p, "mask")
            assert np.array_equal(tree.ends[p].numpy(), ends), (p, "ends")
            has_child = mask.any(1)
            assert np.array_equal(tree.base[p].numpy()[has_child], base[has_child]), (p, "base")
            assert tree.mask[p].dtype == torch.int32 and tree.base[p].dtype == torch.int32 and tree.ends[p].dtype == torch.uint8
    # the padded-array form gives the same tree
    arr = np.full((len(paths), D), 7, np.int64)
    lens = np.array([len(p) for p in paths])
    for i, p in enumerate(paths):
        arr[i, :len(p)] = p
    a = nci.RaggedPrefixTree(paths, K, "cpu", levels=D + 1)
    b = nci.RaggedPrefixTree(arr, K, "cpu", lengths=lens, levels=D + 1)
    for p in range(D + 1):
        assert torch.equal(a.mask[p], b.mask[p]) and torch.equal(a.base[p], b.base[p]) and torch.equal(a.ends[p], b.ends[p])


def test_pool_keeps_the_reference_order():
    """BeamHypotheses: a full pool takes a strictly better score only, drops its lowest (score, position) entry, and the
    output pops a stable ascending sort from the end (equal scores: the later insertion first)."""
    h = vr.Hypotheses(3, 1.0)
    for i, s in enumerate([-4.0, -2.0, -2.0]):
        h.add([0, 10 + i], s)
    assert h.worst == -2.0 and not h.is_done(-1.0, 2) and h.is_done(-4.0, 2)
    h.add([0, 20], -4.0)                                           # equal to the worst: refused
    assert [b[2][1] for b in h.beams] == [10, 11, 12]
    h.add([0, 21], -1.0)                                           # replaces the worst (-4 / 2)
    assert [b[2][1] for b in h.beams] == [11, 12, 21] and h.worst == -1.0
    q = vr.Query(vr.build_trie([(0,)]), 3, 2, 4, 1.0)
    q.pool, q.done = h, True
    decoded, scores, lengths = q.finalize()
    assert decoded[:, 1].tolist() == [21, 12, 11] and scores.tolist() == [-0.5, -1.0, -1.0] and lengths.tolist() == [2, 2, 2]


SEMANTIC_ARGV = """--n_gpu 1 --mode eval --query_type gtq --model_info base --id_class bert_k30_c30_1 --dataset marco
--eval_batch_size 2 --encode_batch_size 1024 --document_encoder ance --recall_level both --codebook 0 --kary 30
--label_length_cutoff 4 --max_output_length 10 --mapping_path D/ids/mapping.pkl --position 1 --tree 1 --query_encoder twin
--num_return_sequences 10 --nci_ckpt D/ckpts/nci.ckpt --data_dir D/origin --ckpt_dir D/ckpts
--embedding_path D/ance/docemb.bin --custom_save_path D/ance/nci_result_k30_top10.tsv""".split()


def _without(argv, flag):
    i = argv.index(flag)
    return argv[:i] + argv[i + 2:]


def test_check_supported_accepts_codebook_0_with_cutoff_and_mapping():
    import main

    a = main.parsers_parser(SEMANTIC_ARGV)
    main.check_supported(a)                                        # no --pq_path / --pq_cluster_path needed
    assert (a.codebook, a.label_length_cutoff, a.kary, a.mapping_path) == (0, 4, 30, "D/ids/mapping.pkl")
    assert not any(f in ("--label_length_cutoff", "--mapping_path", "--kary") for f, _ in a.ignored_flags)
    for enc in ("cocondenser", "ar2"):
        main.check_supported(main.parsers_parser(SEMANTIC_ARGV + ["--document_encoder", enc]))
    for flag in ("--label_length_cutoff", "--mapping_path", "--kary"):
        with pytest.raises(SystemExit, match=flag):
            main.check_supported(main.parsers_parser(_without(SEMANTIC_ARGV, flag)))
    for extra, named in ((["--query_encoder", "nci"], "query_encoder"), (["--doc_multiclus", "2"], "doc_multiclus"),
                         (["--use_topic_model", "1"], "use_topic_model"), (["--max_output_length", "5"], "max_output_length"),
                         (["--num_return_sequences", "100"], "num_return_sequences"), (["--dataset", "nq_dpr"], "dataset")):
        with pytest.raises(SystemExit, match=named):
            main.check_supported(main.parsers_parser(SEMANTIC_ARGV + extra))
    # the codebook path reads none of this: its flags stay pass-through
    b = main.parsers_parser(SEMANTIC_ARGV + ["--codebook", "1"])
    assert ("--label_length_cutoff", "4") in b.ignored_flags
