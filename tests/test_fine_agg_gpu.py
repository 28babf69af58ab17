"""The device fine stage's merge and weight modes (mevi_fine_topk_agg_f32, FineStage.topk / topk_graph with aggregate=,
beam_weights=, doc_proba=) on the GPU: every case of tests/fine_agg_cases.py against the numpy restatement of the rules and --
where FineStage.rerank models the case -- against the first k of rerank's lists with its counts; the refusal above 16384 places,
the captured graph, and the entry point without a mode against the plain call.  Everything is compared exactly: ids equal,
scores equal as uint32 bits, counts equal."""
import numpy as np
import pytest
import torch

import fine_agg_cases as ac
import fine_cases as fc
from mevi_amd import hip, ops
from mevi_amd.fine import FineStage
from mevi_amd.rq import ClusterIndex
from oracle import dense as odense

pytestmark = pytest.mark.gpu


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(np.array(a)).to(cuda)      # a copy: the cases' arrays are read-only


def _check(got, want, what=""):
    s, i, n = (t.cpu().numpy() for t in got[:3])
    want_s, want_i, want_n, want_u = want
    assert n.dtype == np.int32 and np.array_equal(n, want_n), (what, n, want_n)
    if want_u is None:
        assert got[3] is None, what
    else:
        u = got[3].cpu().numpy()
        assert u.dtype == np.int32 and np.array_equal(u, want_u), (what, u, want_u)
    bad = np.flatnonzero((i != want_i).any(1) | (s.view(np.uint32) != want_s.view(np.uint32)).any(1))
    if bad.size:
        b = int(bad[0])
        at = int(np.flatnonzero((i[b] != want_i[b]) | (s[b].view(np.uint32) != want_s[b].view(np.uint32)))[0])
        raise AssertionError(f"{what}: {bad.size} queries differ; query {b} place {at}: got ({s[b, at]!r}, {i[b, at]}), "
                             f"want ({want_s[b, at]!r}, {want_i[b, at]})")


def _stage(case, cuda):
    """The case's index behind a FineStage: one-level codes, so a key is its code."""
    base = case.base
    return FineStage(_dev(base.emb, cuda), ClusterIndex(1, 1 << 20, np.array(base.keys), np.array(base.offsets), np.array(base.docs)))


def _cut(lists, ndoc, k, counted):
    s = np.full((len(lists), k), -odense.FLT_MAX, np.float32)
    i = np.full((len(lists), k), -1, np.int64)
    for b, (ids, sc) in enumerate(lists):
        m = min(k, len(ids))
        s[b, :m], i[b, :m] = sc[:m], ids[:m]
    return s, i, np.asarray(ndoc).astype(np.int32), np.array([len(ids) for ids, _ in lists], np.int32) if counted else None


@pytest.mark.parametrize("entry", ac.ALL, ids=ac.case_id)
def test_case_equals_the_restatement_and_rerank(cuda, entry):
    builder, args = entry
    case = builder(*args)
    base = case.base
    stage = _stage(case, cuda)
    q, keys, dp = _dev(base.q, cuda), _dev(base.beam, cuda), _dev(case.doc_proba, cuda)
    got = stage.topk(q, keys, base.k, max_cand=base.max_cand, aggregate=case.aggregate, beam_weights=_dev(case.weights, cuda),
                     doc_proba=dp, ratio=case.ratio)
    torch.cuda.synchronize()
    assert len(got) == 4
    _check(got, ac.expected_of(builder, *args), ac.case_id(entry))
    if case.rerank:
        lists, ndoc = stage.rerank(q, np.array(base.beam)[:, :, None], aggregate=case.aggregate, beam_weights=_dev(case.weights, cuda),
                                   doc_proba=dp, ratio=case.ratio)
        _check(got, _cut(lists, ndoc, base.k, case.aggregate is not None), ac.case_id(entry) + " vs rerank")


def test_a_merge_above_16384_places_is_refused(cuda):
    """16385 places: the call returns MEVI_ERR_UNSUPPORTED naming max_cand, FineStage.topk points at rerank; weights alone pass."""
    case = ac.full_sort("add")
    base = case.base
    stage = _stage(case, cuda)
    q, keys, w = _dev(base.q, cuda), _dev(base.beam, cuda), _dev(case.weights, cuda)
    for mode in ac.MODES:
        with pytest.raises(ValueError, match="rerank"):
            stage.topk(q, keys, base.k, max_cand=ac.SORT_MAX + 1, aggregate=mode)
        with pytest.raises(hip.MeviHipError, match="max_cand=16385"):
            ops.fine_topk(q, stage.emb, *stage._device_index(), keys, ac.SORT_MAX + 1, base.k, aggregate=mode)
    got = stage.topk(q, keys, base.k, max_cand=ac.SORT_MAX + 1, beam_weights=w)
    _check(got, ac.expected(case._replace(aggregate=None)), "weights alone, max_cand 16385")


def test_the_entry_point_without_a_mode_is_the_plain_call(cuda):
    """mevi_fine_topk_agg_f32 with aggregate 0 and null weights on every plain case: mevi_fine_topk_f32's outputs bit for bit,
    with out_nuniq null."""
    L = hip.lib()
    for builder, args in fc.ALL:
        case = builder(*args)
        B, R = case.beam.shape
        dim, k = case.q.shape[1], case.k
        q, emb, beam = _dev(case.q, cuda), _dev(case.emb, cuda), _dev(case.beam, cuda)
        csr = [None] * 3 if len(case.keys) == 0 else [_dev(a, cuda) for a in (case.keys, case.offsets, case.docs)]
        want = ops.fine_topk(q, emb, *csr, beam, case.max_cand, k)
        out_s = torch.full((B, k), 7.0, dtype=torch.float32, device=cuda)
        out_i = torch.full((B, k), 7, dtype=torch.int64, device=cuda)
        out_n = torch.full((B,), 7, dtype=torch.int32, device=cuda)
        need = L.mevi_fine_topk_agg_workspace_bytes(B, R, k, dim, case.max_cand, 0)
        assert need == ops.fine_topk_workspace_bytes(B, R, k, dim, case.max_cand)
        ws = torch.empty(need, dtype=torch.uint8, device=cuda)
        st = L.mevi_fine_topk_agg_f32(q.data_ptr(), dim, int(case.per_beam), B, R, emb.data_ptr(), len(case.emb), dim,
                                      *(None if a is None else a.data_ptr() for a in csr), len(case.keys), beam.data_ptr(),
                                      case.max_cand, k, 0, None, None, 0.0, 1.0, out_s.data_ptr(), out_i.data_ptr(), out_n.data_ptr(),
                                      None, ws.data_ptr(), need, hip.stream_ptr())
        hip.check(st, "mevi_fine_topk_agg_f32")
        torch.cuda.synchronize()
        for a, b in zip((out_s, out_i, out_n), want):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b), builder.__name__
        assert len(want) == 3


# ---- the captured graph --------------------------------------------------------------------------------------------------
N_DOCS, DIM, K_CODES, C = 20000, 64, 64, 3


@pytest.fixture(scope="module")
def multi_stage(cuda):
    """20 000 x 64 embeddings, every document in C = 3 of 4096 two-level clusters (a multi-cluster index)."""
    rng = np.random.default_rng(501)
    member = np.stack([rng.choice(K_CODES ** 2, size=C, replace=False) for _ in range(N_DOCS)])
    flat = member.reshape(-1)
    order = np.argsort(flat, kind="stable")
    keys, first = np.unique(flat[order], return_index=True)
    offsets = np.append(first, len(flat)).astype(np.int64)
    index = ClusterIndex(2, K_CODES, keys.astype(np.int64), offsets, (order // C).astype(np.int64))
    gen = torch.Generator(device=cuda).manual_seed(502)
    emb = torch.randn((N_DOCS, DIM), generator=gen, device=cuda, dtype=torch.float32)
    return FineStage(emb, index), torch.rand((N_DOCS,), generator=gen, device=cuda, dtype=torch.float32), member


def _beam_row(rng, member, keys, R):
    """R distinct cluster keys: all the clusters of three documents, then others."""
    row = list(dict.fromkeys(member[rng.choice(len(member), size=3, replace=False)].reshape(-1).tolist()))
    for key in rng.permutation(keys).tolist():
        if len(row) == R:
            break
        if key not in row:
            row.append(key)
    return rng.permutation(row)


@pytest.mark.parametrize("B", [1, 32])
def test_graph_replays_with_other_weights_and_keys(cuda, multi_stage, B):
    """topk_graph with merge, weights and blend, replayed twice with different weights and keys: the eager call and rerank.
    Capture itself is the check that the call neither synchronises nor allocates."""
    stage, proba, member = multi_stage
    R, k = 10, 100
    graph = stage.topk_graph(B, R, k, aggregate="add", weighted=True, doc_proba=proba, ratio=0.3)
    for round_ in range(2):
        rng = np.random.default_rng(510 + round_)
        picked = np.stack([_beam_row(rng, member, stage.index.keys, R) for _ in range(B)])
        codes = np.stack([picked // K_CODES, picked % K_CODES], axis=-1).astype(np.int64)
        keys = torch.from_numpy(picked).to(cuda)
        w = np.log(rng.random((B, R)) * 0.9 + 0.05).astype(np.float32)
        gen = torch.Generator(device=cuda).manual_seed(520 + round_)
        q = torch.randn((B, DIM), generator=gen, device=cuda, dtype=torch.float32)
        got = graph.run(q, keys, torch.from_numpy(w).to(cuda))
        eager = stage.topk(q, keys, k, aggregate="add", beam_weights=w, doc_proba=proba, ratio=0.3)
        _check(got, tuple(t.cpu().numpy() for t in eager), f"graph vs eager, round {round_}")
        lists, ndoc = stage.rerank(q, codes, aggregate="add", beam_weights=w, doc_proba=proba, ratio=0.3)
        assert (np.array([len(ids) for ids, _ in lists]) < ndoc).any()          # documents really met twice
        _check(got, _cut(lists, ndoc, k, True), f"graph vs rerank, round {round_}")
    with pytest.raises(ValueError, match="weighted"):
        stage.topk_graph(B, R, k, doc_proba=proba, ratio=0.3)
