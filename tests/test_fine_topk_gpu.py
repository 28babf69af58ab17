"""The device fine stage (mevi_fine_topk_f32, FineStage.topk / topk_graph) on the GPU: every case of tests/fine_cases.py against
the oracle's lists (tests/test_fine_topk_cpu.py proves which path each case reaches), `topk` against `rerank` cut to k, and the
captured graph against both.  Everything is compared exactly: ids equal, scores equal as uint32 bits, ndoc equal."""
import numpy as np
import pytest
import torch

import fine_cases as fc
from mevi_amd import ops
from mevi_amd.fine import FineStage
from mevi_amd.rq import ClusterIndex
from oracle import dense as odense

pytestmark = pytest.mark.gpu


def _dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)                # a copy: the cases' arrays are read-only


def _csr(case, cuda):
    return (None, None, None) if len(case.keys) == 0 else tuple(_dev(a, cuda) for a in (case.keys, case.offsets, case.docs))


def _check(got, want, what=""):
    s, i, n = (t.cpu().numpy() for t in got)
    want_s, want_i, want_n = want
    assert n.dtype == np.int32 and np.array_equal(n, want_n), (what, n, want_n)
    bad = np.flatnonzero((i != want_i).any(1) | (s.view(np.uint32) != want_s.view(np.uint32)).any(1))
    if bad.size:
        b = int(bad[0])
        at = int(np.flatnonzero((i[b] != want_i[b]) | (s[b].view(np.uint32) != want_s[b].view(np.uint32)))[0])
        raise AssertionError(f"{what}: {bad.size} queries differ; query {b} place {at}: got ({s[b, at]!r}, {i[b, at]}), "
                             f"want ({want_s[b, at]!r}, {want_i[b, at]})")


@pytest.mark.parametrize("entry", fc.ALL, ids=fc.case_id)
def test_case_equals_the_oracle(cuda, entry):
    builder, args = entry
    case = builder(*args)
    got = ops.fine_topk(_dev(case.q, cuda), _dev(case.emb, cuda), *_csr(case, cuda), _dev(case.beam, cuda), case.max_cand, case.k)
    torch.cuda.synchronize()
    _check(got, fc.expected_of(builder, *args), fc.case_id(entry))


@pytest.mark.parametrize("per_beam", [False, True])
def test_query_rows_with_a_stride_above_dim(cuda, per_beam):
    """ldq = 48 > dim = 36: the query rows are a column slice of a wider matrix whose other columns are NaN."""
    case = fc.dims(36, per_beam)
    wide = torch.full((case.q.shape[0], 48), float("nan"), dtype=torch.float32, device=cuda)
    wide[:, :36] = _dev(case.q, cuda)
    q = wide[:, :36]
    assert q.stride(0) == 48 and not q.is_contiguous()
    got = ops.fine_topk(q, _dev(case.emb, cuda), *_csr(case, cuda), _dev(case.beam, cuda), case.max_cand, case.k)
    _check(got, fc.expected_of(fc.dims, 36, per_beam), "ldq 48")


@pytest.mark.parametrize("per_beam", [False, True])
def test_a_walk_longer_than_max_cand_is_cut_and_nothing_else_is_written(cuda, per_beam):
    """max_cand = 100 below two queries' walks: ndoc is the true count, the lists are the top-k of the first 100 candidates in
    walk order, and the guard words before and after the three outputs and the workspace keep their pattern."""
    case = fc.short_bound(per_beam)
    B, R = case.beam.shape
    k, G = case.k, 256                                            # guard: 256 bytes on either side
    need = ops.fine_topk_workspace_bytes(B, R, k, case.q.shape[1], case.max_cand)

    def guarded(nbytes):
        buf = torch.full((G + nbytes + G,), 0xA5, dtype=torch.uint8, device=cuda)
        assert buf.data_ptr() % 256 == 0
        return buf, buf[G:G + nbytes]

    bs, vs = guarded(B * k * 4)
    bi, vi = guarded(B * k * 8)
    bn, vn = guarded(B * 4)
    bw, vw = guarded(need)
    out = (vs.view(torch.float32).view(B, k), vi.view(torch.int64).view(B, k), vn.view(torch.int32))
    got = ops.fine_topk(_dev(case.q, cuda), _dev(case.emb, cuda), *_csr(case, cuda), _dev(case.beam, cuda), case.max_cand, k, out=out,
                        workspace=vw)
    torch.cuda.synchronize()
    want = fc.expected_of(fc.short_bound, per_beam)
    _check(got, want, "short bound")
    walks = np.array([len(fc.walk(case, b)[0]) for b in range(B)])
    assert np.array_equal(want[2], walks) and (walks > case.max_cand).sum() == 2
    for name, buf, n in (("scores", bs, B * k * 4), ("ids", bi, B * k * 8), ("ndoc", bn, B * 4), ("workspace", bw, need)):
        assert (buf[:G] == 0xA5).all() and (buf[G + n:] == 0xA5).all(), name


# ---- FineStage.topk against rerank -------------------------------------------------------------------------------------------
N_DOCS, DIM, M, K = 50000, 768, 2, 256


@pytest.fixture(scope="module")
def stage(cuda):
    """50 000 x 768 embeddings, clusters of ~Poisson(8) documents under random distinct two-level codes."""
    rng = np.random.default_rng(301)
    sizes = []
    while sum(sizes) < N_DOCS:
        sizes.append(int(rng.poisson(8)))
    sizes[-1] -= sum(sizes) - N_DOCS
    sizes = np.array([s for s in sizes if s > 0], np.int64)
    keys = np.sort(rng.choice(K ** M, size=len(sizes), replace=False)).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    index = ClusterIndex(M, K, keys, offsets, rng.permutation(N_DOCS).astype(np.int64))
    gen = torch.Generator(device=cuda).manual_seed(302)
    emb = torch.randn((N_DOCS, DIM), generator=gen, device=cuda, dtype=torch.float32)
    return FineStage(emb, index)


def _beams(stage, rng, B, R):
    """Codes i64 [B, R, M]: distinct clusters of the index per row, one row in eight with an absent code in it."""
    keys = stage.index.keys
    picked = np.stack([rng.choice(keys, size=R, replace=False) for _ in range(B)])
    absent = np.setdiff1d(np.arange(K ** M), keys)
    picked[::8, R // 2] = rng.choice(absent, size=len(picked[::8]))
    return np.stack([picked // K, picked % K], axis=-1).astype(np.int64)


def _cut(lists, ndoc, k):
    s = np.full((len(lists), k), -odense.FLT_MAX, np.float32)
    i = np.full((len(lists), k), -1, np.int64)
    for b, (ids, sc) in enumerate(lists):
        m = min(k, len(ids))
        s[b, :m], i[b, :m] = sc[:m], ids[:m]
    return s, i, np.asarray(ndoc).astype(np.int32)


@pytest.mark.parametrize("per_beam", [False, True])
def test_topk_equals_rerank_cut_to_k(cuda, stage, per_beam):
    B, R, k = 200, 10, 100
    rng = np.random.default_rng(303 + per_beam)
    codes = _beams(stage, rng, B, R)
    gen = torch.Generator(device=cuda).manual_seed(304)
    q = torch.randn((B * R if per_beam else B, DIM), generator=gen, device=cuda, dtype=torch.float32)
    lists, ndoc = stage.rerank(q, codes)
    assert 40 < np.mean(ndoc) < 120 and max(ndoc) <= stage.max_candidates(R)
    want = _cut(lists, ndoc, k)
    for beam in (torch.from_numpy(codes).to(cuda), torch.from_numpy(codes.astype(np.int32)).to(cuda),
                 torch.from_numpy(ClusterIndex.code_keys(codes, K)).to(cuda)):
        got = stage.topk(q, beam, k)
        assert all(t.is_cuda for t in got) and got[0].shape == (B, k) and got[1].shape == (B, k) and got[2].shape == (B,)
        _check(got, want, f"topk vs rerank, beam {beam.dtype} {tuple(beam.shape)}")


@pytest.mark.parametrize("per_beam", [False, True])
def test_graph_replays_equal_the_eager_call_and_the_oracle(cuda, stage, per_beam):
    """Capture itself is the check that the call neither synchronises nor allocates."""
    B, R, k = 8, 10, 100
    graph = stage.topk_graph(B, R, k, per_beam=per_beam)
    emb = None
    for round_ in range(3):
        rng = np.random.default_rng(310 + round_)
        codes = _beams(stage, rng, B, R)
        keys = torch.from_numpy(ClusterIndex.code_keys(codes, K)).to(cuda)
        gen = torch.Generator(device=cuda).manual_seed(320 + round_)
        q = torch.randn((B * R if per_beam else B, DIM), generator=gen, device=cuda, dtype=torch.float32)
        got = graph.run(q, keys)
        eager = stage.topk(q, keys, k)
        _check(got, tuple(t.cpu().numpy() for t in eager), f"graph vs eager, round {round_}")
        if round_ == 2:                                           # the oracle once: the rows it needs, not the whole matrix
            idx, qh = stage.index, q.cpu().numpy()
            cl = {(int(c) // K, int(c) % K): idx.doc_ids[a:b] for c, a, b in zip(idx.keys, idx.offsets[:-1], idx.offsets[1:])}
            rows = np.unique(np.concatenate([cl.get(tuple(c), np.zeros(0, np.int64)) for c in codes.reshape(-1, M)]))
            emb = np.zeros((N_DOCS, DIM), np.float32)
            emb[rows] = stage.emb[torch.from_numpy(rows).to(cuda)].cpu().numpy()
            lists, ndoc = [], []
            for b in range(B):
                if per_beam:
                    parts = [odense.fine_stage(qh[b * R + j], emb, cl, [codes[b, j]]) for j in range(R)]
                    docs, sc = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
                    order = np.lexsort((docs, -sc))
                    docs, sc = docs[order], sc[order]
                else:
                    docs, sc, _ = odense.fine_stage(qh[b], emb, cl, codes[b])
                lists.append((docs, sc))
                ndoc.append(len(docs))
            _check(got, _cut(lists, ndoc, k), "graph vs oracle")


def test_graph_refuses_more_than_32_queries(cuda, stage):
    with pytest.raises(ValueError, match="B=33"):
        stage.topk_graph(33, 10, 100)
    with pytest.raises(ValueError, match="B=0"):
        stage.topk_graph(0, 10, 100)
