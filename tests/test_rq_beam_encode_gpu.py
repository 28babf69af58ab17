"""The fused beam encode (mevi_rq_beam_encode_f32, csrc/rq_beam.hip) against the per-level composition it replaces -- labels
equal, probabilities equal as bits -- and against the float64-softmax chain reference under the relative comparison of
tests/index_build_ref.py (its constants, no new tolerance); row counts around the tile and over a whole persistent grid,
ties, R = 1 against the encoders, a null `proba`, the Python routing, stream order and graph capture, guard bands."""
import numpy as np
import pytest
import torch

import index_build_ref as ib
import rq_beam_cases as rc
from mevi_amd import hip, rq

pytestmark = pytest.mark.gpu

ROWS_SHAPE, ROWS_R = (32, 3, 16), 4           # (dim, M, K) of the row-count runs


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _both(x, cb, R, pq):
    lab, pr = rc.fused(x, cb, R, pq)
    wl, wp = rc.composition(x, cb, R, pq)
    return lab, pr, wl, wp


def _assert_identical(lab, pr, wl, wp, what):
    assert lab.shape == wl.shape and torch.equal(lab, wl), (what, int((lab != wl).any(-1).sum()))
    assert rc.same_bits(pr, wp), (what, int((pr.view(torch.int32) != wp.view(torch.int32)).sum()))


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_identical_to_the_composition_and_close_to_the_chain_reference(cuda, case):
    shape, R, pq = case
    n, dim, M, K = shape
    x, cb = rc.inputs(shape, pq)
    lab, pr, wl, wp = _both(_t(x, cuda), _t(cb, cuda), R, pq)
    assert lab.shape == (n, R, M) and lab.dtype == torch.int32 and pr.shape == (n, R)
    _assert_identical(lab, pr, wl, wp, case)
    # the independent reference: oracle fmaf chain, float64 softmax, the project's constants
    rl, rs, cut = rc.reference(shape, R, pq)
    lab, pr = lab.cpu().numpy(), pr.cpu().numpy()
    ok, share = ib.beams_agree_rel(lab, pr, rl, rs, ib.SCORE_RTOL, ib.GAP_RTOL, cut)
    rel = np.abs(pr.astype(np.float64) - rs) / rs
    print(f"{rc.case_id(case)}: max relative score difference {rel[cut > ib.GAP_RTOL].max():.3g}, firm share {share:.3f}, "
          f"label rows differing from the reference {int((lab != rl).any((1, 2)).sum())}")
    assert ok and share >= ib.FIRM_SHARE_MIN, (case, share)


def test_row_counts_around_the_tile(cuda):
    dim, M, K = ROWS_SHAPE
    T = int(hip.lib().mevi_rq_beam_encode_tile_docs(dim, M, K, ROWS_R, 0))
    assert T > 1
    x, cb = ib.clustered_inputs(3 * T + 1, dim, M, K, 77)
    xt, ct = _t(x, cuda), _t(cb, cuda)
    wl, wp = rc.composition(xt, ct, ROWS_R, False)
    for n in (0, 1, T - 1, T, T + 1, 3 * T + 1):
        lab, pr = rc.fused(xt[:n].contiguous(), ct, ROWS_R, False)
        assert lab.shape == (n, ROWS_R, M)
        _assert_identical(lab, pr, wl[:n], wp[:n], n)


@pytest.mark.parametrize("pq", [False, True], ids=["rq", "pq"])
def test_every_workgroup_walks_several_tiles(cuda, pq):
    """Three tiles and a bit per workgroup of the persistent grid (at most two workgroups per CU), the last tile partly
    filled: the ticket walk, the reuse of a workgroup's LDS state from tile to tile, the tail."""
    dim, M, K = ROWS_SHAPE
    M = 4 if pq else M
    T = int(hip.lib().mevi_rq_beam_encode_tile_docs(dim, M, K, ROWS_R, int(pq)))
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    n = T * (3 * 2 * cus) + T // 2 + 1
    x, cb = ib.clustered_inputs(n, dim, M, K, 78, pq=pq)
    lab, pr, wl, wp = _both(_t(x, cuda), _t(cb, cuda), ROWS_R, pq)
    _assert_identical(lab, pr, wl, wp, n)


def test_ties_go_to_the_lower_beam_and_code(cuda):
    x, cb = rc.tie_inputs()
    K = cb.shape[1]
    xt, ct = _t(x, cuda), _t(cb, cuda)
    for R in (6, 16, 3):                       # 16 == K: kept unsorted at level 0, top-R over ties after it
        lab, pr, wl, wp = _both(xt, ct, R, False)
        _assert_identical(lab, pr, wl, wp, R)
        if R % 2 == 0:                         # pairs of equal scores, the lower code of the twin centroids first
            assert torch.equal(pr[:, 0::2], pr[:, 1::2]) and torch.equal(lab[:, 0::2, -1] + K // 2, lab[:, 1::2, -1])
        assert torch.equal(lab[:len(x) // 2], lab[len(x) // 2:])            # the twin rows


@pytest.mark.parametrize("case", [c for c in rc.CASES if c[1] == 1], ids=rc.case_id)
def test_one_beam_is_the_encoder(cuda, case):
    shape, R, pq = case
    x, cb = rc.inputs(shape, pq)
    xt, ct = _t(x, cuda), _t(cb, cuda)
    lab, _ = rc.fused(xt, ct, 1, pq)
    want = rq.pq_encode(xt, ct) if pq else rq.rq_encode(xt, ct, mode="exact")
    assert torch.equal(lab[:, 0], want)


def test_null_proba_gives_the_same_labels(cuda):
    for shape, R, pq in (((301, 64, 3, 16), 10, False), ((301, 64, 4, 16), 16, True)):
        x, cb = rc.inputs(shape, pq)
        xt, ct = _t(x, cuda), _t(cb, cuda)
        lab, _ = rc.fused(xt, ct, R, pq)
        lab2, none = rc.fused(xt, ct, R, pq, want_proba=False)
        assert none is None and torch.equal(lab, lab2)


def test_guard_bands_stay_intact(cuda):
    for pq, M in ((False, 3), (True, 4)):
        dim, _, K = ROWS_SHAPE
        T = int(hip.lib().mevi_rq_beam_encode_tile_docs(dim, M, K, ROWS_R, int(pq)))
        x, cb = ib.clustered_inputs(T + 1, dim, M, K, 79, pq=pq)
        xt, ct = _t(x, cuda), _t(cb, cuda)
        wl, wp = rc.composition(xt, ct, ROWS_R, pq)
        for want_proba in (True, False):
            lab, pr, intact = rc.fused(xt, ct, ROWS_R, pq, want_proba=want_proba, guard=4096)
            assert intact and torch.equal(lab, wl) and (pr is None or rc.same_bits(pr, wp))


def _object(shape, pq, cb, cuda):
    n, dim, M, K = shape
    obj = rq.ProductQuantization("pq" if pq else "rq", M, int(np.log2(K)), "l2", dim, device=cuda)
    obj.load_codebook(cb)
    return obj


@pytest.mark.parametrize("shape,R,pq", [((301, 64, 3, 16), 3, False), ((130, 768, 4, 32), 10, False), ((301, 64, 4, 16), 16, True)], ids=str)
def test_beam_search_is_the_same_with_and_without_the_fused_call(cuda, monkeypatch, shape, R, pq):
    x, cb = rc.inputs(shape, pq)
    obj = _object(shape, pq, cb, cuda)
    calls = []
    real = obj._beam_search_steps
    monkeypatch.setattr(obj, "_beam_search_steps", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    monkeypatch.delenv("MEVI_RQ_BEAM", raising=False)
    lab, pr = obj.beam_search(torch.from_numpy(x), R, return_proba=True)
    only = obj.beam_search(torch.from_numpy(x), R)
    assert not calls and obj.beam_search_is_fused(R)
    monkeypatch.setenv("MEVI_RQ_BEAM", "steps")
    wl, wp = obj.beam_search(torch.from_numpy(x), R, return_proba=True)
    assert len(calls) == 1 and not obj.beam_search_is_fused(R)
    _assert_identical(lab, pr, wl, wp, (shape, R, pq))
    assert torch.equal(only, lab)
    monkeypatch.delenv("MEVI_RQ_BEAM")
    empty = obj.beam_search(torch.zeros((0, shape[1])), R, return_proba=True)
    assert empty[0].shape == (0, R, shape[2]) and empty[0].dtype == torch.int32 and empty[1].shape == (0, R)


def test_wide_beams_still_take_the_composition(cuda, monkeypatch):
    shape = (301, 64, 3, 16)
    x, cb = rc.inputs(shape)
    obj = _object(shape, False, cb, cuda)
    monkeypatch.delenv("MEVI_RQ_BEAM", raising=False)
    calls = []
    real = obj._beam_search_steps
    monkeypatch.setattr(obj, "_beam_search_steps", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    lab = obj.beam_search(torch.from_numpy(x), 40)
    assert len(calls) == 1 and lab.shape == (301, 40, 3)
    wl, _ = rc.composition(_t(x, cuda), _t(cb, cuda), 40, False)
    assert torch.equal(lab, wl)


def test_topk_document_mapping_over_ranks_and_input_kinds(cuda, monkeypatch):
    shape = (301, 64, 3, 16)
    x, cb = rc.inputs(shape)
    obj = _object(shape, False, cb, cuda)
    monkeypatch.delenv("MEVI_RQ_BEAM", raising=False)
    whole = obj.beam_search(torch.from_numpy(x), 3).cpu()
    for source in (x, torch.from_numpy(x), _t(x, cuda)):                    # numpy, host tensor, CUDA tensor
        parts = [obj.get_topk_document_mapping(source, r, 3, 3, batch_size=100) for r in range(3)]
        assert [len(p) for p in parts] == [100, 100, 101] and all(p.dtype == torch.int32 and not p.is_cuda for p in parts)
        assert torch.equal(torch.cat(parts), whole)
    # a CUDA tensor is one fused call over the rank's slice, whatever the batch size
    calls = []
    real = obj._beam_search_fused
    monkeypatch.setattr(obj, "_beam_search_fused", lambda *a, **kw: calls.append(a[0].shape[0]) or real(*a, **kw))
    assert torch.equal(obj.get_topk_document_mapping(_t(x, cuda), 2, 3, 3, batch_size=7), whole[200:])
    assert calls == [101]
    calls.clear()
    assert torch.equal(obj.get_topk_document_mapping(x, 2, 3, 3, batch_size=50), whole[200:])
    assert calls == [50, 50, 1]


def test_stream_ordered_and_capturable(cuda):
    shape, R = (301, 64, 3, 16), 10
    x, cb = rc.inputs(shape)
    obj = _object(shape, False, cb, cuda)
    xt = _t(x, cuda)
    want_l, want_p = rc.composition(xt, _t(cb, cuda), R, False)
    torch.cuda.synchronize(cuda)
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        y = xt * 1.0                                                        # produced on the side stream, consumed by the call
        lab, pr = obj.beam_search(y, R, return_proba=True)
        graph = torch.cuda.CUDAGraph()
        static_x = y.clone()
        with torch.cuda.graph(graph, stream=side):                          # one chain: a memset node and a kernel node
            g_lab, g_pr = obj.beam_search(static_x, R, return_proba=True)
        static_x.copy_(xt.flip(0))
        graph.replay()
    side.synchronize()
    _assert_identical(lab, pr, want_l, want_p, "side stream")
    _assert_identical(g_lab, g_pr, want_l.flip(0), want_p.flip(0), "graph replay")
