"""The NCI baseline -- `main.py --mode eval` without --document_encoder -- without a GPU: what the argv resolves to, what is
refused, that the tower path's refusals stand, and the restatement tests/varbeam_ref.py at 40 / 100 beams against the
reference's goldens g1v_wide_* (tools/capture_goldens_varlen.py)."""
import json
import os

import numpy as np
import pytest

from test_varbeam_cpu import GOLD, SEMANTIC_ARGV, _without, golden_paths, golden_search

PURE_ARGV = """--n_gpu 1 --mode eval --query_type gtq --model_info base --id_class bert_k30_c30_1 --dataset marco
--eval_batch_size 2 --kary 30 --mapping_path D/ids/mapping.pkl --position 1 --tree 1
--nci_ckpt D/ckpts/nci.ckpt --data_dir D/origin --ckpt_dir D/ckpts --custom_save_path D/nci/nci_result_k30.tsv""".split()
WIDE = [os.path.join(GOLD, "g1v_wide_M8_K8_R40.npz"), os.path.join(GOLD, "g1v_wide_M4_K30_R100.npz")]


def test_pure_nci_argv_is_accepted_with_the_reference_defaults():
    import main

    a = main.parsers_parser(PURE_ARGV)
    main.check_supported(a)
    assert a.pure_nci and a.document_encoder is None and a.codebook == 0
    assert a.label_length_cutoff == a.max_output_length - 2 == 8 and a.num_return_sequences == 100
    assert a.recall_num == [1, 5, 10, 20, 50, 100] and a.recall_level == "coarse"
    flags = [f for f, _ in a.ignored_flags]
    assert not any(f in ("--mapping_path", "--kary", "--label_length_cutoff", "--max_output_length") for f in flags)
    # --codebook 1 is overridden (MEVI/main.py:628), --query_encoder is not read, a cutoff shortens the output
    b = main.parsers_parser(PURE_ARGV + ["--codebook", "1", "--query_encoder", "nci", "--label_length_cutoff", "4",
                                         "--max_output_length", "10", "--num_return_sequences", "40"])
    main.check_supported(b)
    assert (b.codebook, b.label_length_cutoff, b.max_output_length, b.recall_num) == (0, 4, 6, [1, 5, 10, 20])
    assert not any(f in ("--label_length_cutoff", "--max_output_length") for f, _ in b.ignored_flags)
    c = main.parsers_parser(PURE_ARGV + ["--max_output_length", "17", "--num_return_sequences", "128", "--kary", "256"])
    main.check_supported(c)
    assert c.label_length_cutoff == 15
    main.check_supported(main.parsers_parser(_without(PURE_ARGV, "--nci_ckpt") + ["--infer_ckpt", "D/ckpts/whole.ckpt"]))


@pytest.mark.parametrize("argv,named", [
    (_without(PURE_ARGV, "--mapping_path"), "--mapping_path"),
    (_without(PURE_ARGV, "--kary"), "--kary"),
    (_without(PURE_ARGV, "--nci_ckpt"), "--nci_ckpt or --infer_ckpt"),
    (_without(PURE_ARGV, "--custom_save_path"), "--custom_save_path"),
    (PURE_ARGV + ["--num_return_sequences", "129"], "--num_return_sequences"),
    (PURE_ARGV + ["--kary", "257"], "--kary"),
    (PURE_ARGV + ["--max_output_length", "18"], "--label_length_cutoff"),
    (_without(PURE_ARGV, "--dataset") + ["--dataset", "nq_dpr"], "--dataset"),
    (PURE_ARGV + ["--use_topic_model", "1"], "--use_topic_model"),
    (PURE_ARGV + ["--eval_all_documents", "1"], "--eval_all_documents"),
    (PURE_ARGV + ["--recall_level", "both"], "--recall_level"),
])
def test_pure_nci_refusals_name_the_flag(argv, named):
    import main

    with pytest.raises(SystemExit, match=named):
        main.check_supported(main.parsers_parser(argv))


def test_tower_path_refusals_stand():
    import main

    a = main.parsers_parser(SEMANTIC_ARGV)
    main.check_supported(a)
    assert not a.pure_nci and a.label_length_cutoff == 4 and a.max_output_length == 10
    for extra, named in ((["--num_return_sequences", "100"], "num_return_sequences"), (["--num_return_sequences", "33"], "num_return_sequences"),
                         (["--label_length_cutoff", "8"], "label_length_cutoff"), (["--query_encoder", "nci"], "query_encoder")):
        with pytest.raises(SystemExit, match=named):
            main.check_supported(main.parsers_parser(SEMANTIC_ARGV + extra))
    with pytest.raises(SystemExit, match="document_encoder"):
        main.check_supported(main.parsers_parser(SEMANTIC_ARGV + ["--document_encoder", "dpr"]))
    # other modes without a tower are what they were
    with pytest.raises(SystemExit, match="inference hot path only"):
        main.check_supported(main.parsers_parser(_without(_without(PURE_ARGV, "--mode"), "--kary")))


@pytest.mark.parametrize("path", WIDE)
def test_restatement_matches_the_wide_goldens(path):
    """40 beams over ids of 2 .. 8 codes (nine decoder positions, ids that are prefixes of ids) and 100 beams over K = 30:
    tokens identical, scores within the G1V bound, lengths = the eos positions."""
    g = np.load(path)
    cfg = json.loads(str(g["cfg"]))
    assert cfg["beams"] > 32 and str(g["weights_from"]) in os.listdir(GOLD)
    decoded, scores, lengths, _ = golden_search(g)
    assert np.array_equal(decoded, g["decoded"])
    ref = g["scores"]
    assert (np.abs(scores - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref))).all()
    eos_at = np.array([list(row).index(1) if 1 in row else len(row) for row in g["decoded"]])
    assert np.array_equal(lengths, eos_at)


def test_wide_goldens_have_the_shapes_the_search_is_for():
    g = np.load(WIDE[0])
    paths = set(golden_paths(g))
    lens = {len(p) for p in paths}
    assert (min(lens), max(lens)) == (2, 8) and any(p[:n] in paths for p in paths for n in range(2, len(p)))
    assert "step8_logits" in g.files and g["decoded"].shape == (3 * 40, 10)        # nine decoder positions
    g = np.load(WIDE[1])
    assert json.loads(str(g["cfg"]))["beams"] == 100 and g["decoded"].shape == (2 * 100, 6)


def test_metrics_without_clusters_have_no_ndoc_line(tmp_path):
    """handle_infer_results with `length is None` (MEVI/main_models.py:4100-4201, 4381-4393): recall / mrr / hitrate over the
    id ranks, no cluster figures, no ndocs line."""
    from mevi_amd.evalrun import summarize, write_metrics

    results = [("q0", None, (0, None)), ("q1", None, (7,)), ("q2", None, (None,))]
    out = summarize(results, [1, 5, 10], 40, both=False, at_all=False)
    assert out["ndoc"] is None and out["nqueries"] == 3
    assert out["recall"] == {1: 0.5 / 3, 5: 0.5 / 3, 10: 1.5 / 3} and out["mrr"] == {1: 1 / 3, 5: 1 / 3, 10: (1 + 1 / 8) / 3}
    assert out["hitrate"] == {1: 1 / 3, 5: 1 / 3, 10: 2 / 3}
    write_metrics(out, str(tmp_path / "m.txt"), 40, 5)
    text = (tmp_path / "m.txt").read_text()
    assert "ndocs" not in text and "cluster" not in text and text.splitlines()[0] == f"recall1 {0.5 / 3}"
