"""The refine call (dense.refine_topk = mevi_refine_topk_f32) against tests/refine_cases.py: ids equal and score bits equal at every
slab shape (dim), every selection width and launch (n_cand around the wave, the chunk and the 2048 split, the 16384 limit), k
below, at and above the candidates, padded / out-of-range / repeated / all-invalid candidate rows with their counts, ties, strides
with guard values, zero vectors, a second query tile, and graph replay."""
import functools

import numpy as np
import pytest
import torch

import refine_cases as rc
from mevi_amd import dense, hip

pytestmark = pytest.mark.gpu
ND = 3000


def _bits(a):
    return a.view(np.uint32)


@functools.lru_cache(maxsize=None)
def _corpus(dim):
    """(docs, queries) of one width, shared by the tests: nobody writes to them.  Rows 10..19 are copies of row 10."""
    rng = np.random.default_rng(100 + dim)
    d = rng.standard_normal((ND, dim)).astype(np.float32)
    d[10:20] = d[10]
    q = rng.standard_normal((5, dim)).astype(np.float32)
    d.setflags(write=False)
    q.setflags(write=False)
    return d, q


@functools.lru_cache(maxsize=None)
def _docs_on(dim):
    return torch.from_numpy(np.array(_corpus(dim)[0])).cuda()


def _candidates(seed, nq, n_cand):
    """Random ids without repeats inside a row while the corpus has enough rows (above ND: with repeats)."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(ND)[:n_cand] if n_cand <= ND else rng.integers(0, ND, size=n_cand) for _ in range(nq)]).astype(np.int64)


def _run(q, docs_t, cand, k, **kw):
    s, i, n = dense.refine_topk(torch.from_numpy(np.array(q)).cuda(), docs_t, torch.from_numpy(np.array(cand)).cuda(),
                                k, **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy()


def _check(got, want, k, what):
    np.testing.assert_array_equal(got[1], want[1][:, :k], err_msg=f"ids {what}")
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0][:, :k]), err_msg=f"score bits {what}")
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"nvalid {what}")


@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 129, 2048, 2049, 4096])
@pytest.mark.parametrize("dim", [4, 32, 36, 100, 768])
def test_call_equals_the_reference(cuda, dim, n_cand):
    d, q = _corpus(dim)
    cand = _candidates(7 * dim + n_cand, 5, n_cand)
    full = max(4096, n_cand + 5)
    want = rc.refine_expected(q, d, cand, full)                     # once per shape: every k is a prefix of it
    for nq in (1, 5):
        for k in sorted({1, n_cand, min(n_cand + 5, 4096), 4096}):
            got = _run(q[:nq], _docs_on(dim), cand[:nq], k)
            _check(got, tuple(w[:nq] for w in want), k, f"dim={dim} n_cand={n_cand} nq={nq} k={k}")


def test_the_longest_candidate_row(cuda):
    d, q = _corpus(32)
    cand = _candidates(3, 2, 16384)
    cand[1, 5000:5100] = -1
    want = rc.refine_expected(q[:2], d, cand, 4096)
    for k in (1, 4096):
        _check(_run(q[:2], _docs_on(32), cand, k), want, k, f"n_cand=16384 k={k}")
    assert want[2].tolist() == [16384, 16284]


@pytest.mark.parametrize("dim,n_cand", [(36, 70), (32, 2100)])
def test_candidate_rows_with_padding_foreign_ids_repeats_and_nothing(cuda, dim, n_cand):
    d, q = _corpus(dim)
    cand = _candidates(11, 5, n_cand)
    cand[0, 30:40] = -1                                             # -1 in the middle
    cand[0, -7:] = -1                                               # ... and at the tail
    cand[1, 0] = ND                                                 # ids >= n_docs, the first one past the end and far ones
    cand[1, 17] = ND + 1
    cand[1, 64] = (1 << 31) + 5
    cand[1, 65] = (1 << 40) + 3
    cand[1, 66] = -(1 << 33)
    cand[2, 5] = cand[2, 6] = cand[2, 50] = cand[2, 3]              # one id four times
    cand[2, 69] = cand[2, 0]
    cand[3] = -1                                                    # nothing valid: all padding, count 0
    cand[4, :] = np.arange(n_cand) % 25                             # few distinct ids, rows 10..19 (equal rows) among them
    k = n_cand + 5
    want = rc.refine_expected(q, d, cand, k)
    assert want[2].tolist() == [n_cand - 17, n_cand - 5, n_cand, 0, n_cand]
    got = _run(q, _docs_on(dim), cand, k)
    _check(got, want, k, "special rows")
    assert (got[1][3] == -1).all() and (got[0][3] == -rc.FLT_MAX).all()
    assert (got[1][2] == cand[2, 3]).sum() == 4
    _check(_run(q, _docs_on(dim), cand, 10), want, 10, "special rows, k=10")


def test_equal_scores_come_out_in_ascending_id(cuda):
    d, q = _corpus(100)
    cand = np.stack([np.random.default_rng(b).permutation(40) for b in range(5)]).astype(np.int64)      # rows 10..19 in any order
    want = rc.refine_expected(q, d, cand, 40)
    got = _run(q, _docs_on(100), cand, 40)
    _check(got, want, 40, "ties")
    for b in range(5):
        at = np.flatnonzero((got[1][b] >= 10) & (got[1][b] < 20))
        assert len(at) == 10 and (np.diff(at) == 1).all() and got[1][b][at].tolist() == list(range(10, 20))
        assert len(set(_bits(got[0][b][at]).tolist())) == 1


def test_strided_queries_and_candidates_leave_their_padding_alone(cuda):
    dim, n_cand, k = 36, 130, 20
    d, q = _corpus(dim)
    cand = _candidates(5, 5, n_cand)
    cand[2, 100:] = -1
    qbuf = torch.full((5, dim + 12), float("nan"), dtype=torch.float32, device=cuda)       # ldq = 48: NaN guards behind every row
    qbuf[:, :dim] = torch.from_numpy(np.array(q))
    cbuf = torch.full((5, n_cand + 3), 7, dtype=torch.int64, device=cuda)                  # ld_cand = 133: valid ids as guards
    cbuf[:, :n_cand] = torch.from_numpy(cand)
    out = (torch.full((5, k), 123.0, dtype=torch.float32, device=cuda), torch.full((5, k), 123, dtype=torch.int64, device=cuda),
           torch.full((5,), 123, dtype=torch.int32, device=cuda))
    ws = torch.full((dense.refine_topk_workspace_bytes(5, n_cand, k, dim) + 256,), 0xAB, dtype=torch.uint8, device=cuda)
    s, i, n = dense.refine_topk(qbuf[:, :dim], _docs_on(dim), cbuf[:, :n_cand], k, out=out, workspace=ws[:-256])
    torch.cuda.synchronize()
    assert s is out[0] and i is out[1] and n is out[2]
    _check((s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy()), rc.refine_expected(q, d, cand, k), k, "strided")
    assert torch.isnan(qbuf[:, dim:]).all() and (cbuf[:, n_cand:] == 7).all() and (ws[-256:] == 0xAB).all()
    assert torch.equal(cbuf[:, :n_cand].cpu(), torch.from_numpy(cand))


def test_zero_vectors_score_plus_zero(cuda):
    dim, n_cand = 36, 70
    d, _ = _corpus(dim)
    d = np.array(d)
    d[5] = -0.0
    cand = _candidates(9, 2, n_cand)
    cand[1, 0] = 5
    cand[1, 1] = -1
    q = np.zeros((2, dim), np.float32)
    q[1] = -0.0
    s, i, n = _run(q, torch.from_numpy(d).cuda(), cand, n_cand)
    want = rc.refine_expected(q, d, cand, n_cand)
    _check((s, i, n), want, n_cand, "zero queries")
    assert (_bits(s[0]) == 0).all() and (np.diff(i[0]) > 0).all()            # +0 for every candidate, so ascending id
    assert (_bits(s[1][:n_cand - 1]) == 0).all() and 5 in i[1] and i[1][-1] == -1 and n.tolist() == [n_cand, n_cand - 1]


def test_a_second_query_tile(cuda):
    """The smallest shape whose tile is below a few thousand queries is the one with the most candidates: 16384 a query -> 512."""
    n_cand, dim, k = 16384, 4, 4
    tile = dense.refine_topk_query_tile(1 << 20, n_cand, k, dim)
    assert tile == 512
    nq = tile + 3
    assert dense.refine_topk_query_tile(nq, n_cand, k, dim) == tile < nq
    d, _ = _corpus(dim)
    rng = np.random.default_rng(21)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    cand = rng.integers(0, ND, size=(nq, n_cand)).astype(np.int64)
    cand[tile - 1, ::2] = -1
    cand[tile, ::3] = -1                                                       # the first query of the second tile
    cand[nq - 1, 100:] = -1
    want = rc.refine_expected(q, d, cand, k)
    _check(_run(q, _docs_on(dim), cand, k), want, k, "two tiles")
    assert want[2][tile - 1] == n_cand // 2 and want[2][nq - 1] == 100


@pytest.mark.parametrize("n_cand", [100, 2100])
def test_graph_replay_equals_eager(cuda, n_cand):
    dim, k, nq = 100, 50, 5
    d, q = _corpus(dim)
    docs_t = _docs_on(dim)
    qt = torch.zeros((nq, dim), dtype=torch.float32, device=cuda)
    ct = torch.zeros((nq, n_cand), dtype=torch.int64, device=cuda)
    out = (torch.empty((nq, k), dtype=torch.float32, device=cuda), torch.empty((nq, k), dtype=torch.int64, device=cuda),
           torch.empty((nq,), dtype=torch.int32, device=cuda))
    ws = torch.empty(dense.refine_topk_workspace_bytes(nq, n_cand, k, dim), dtype=torch.uint8, device=cuda)
    dense.refine_topk(qt, docs_t, ct, k, out=out, workspace=ws)               # loads the kernels
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        dense.refine_topk(qt, docs_t, ct, k, out=out, workspace=ws)
    for r in range(2):
        cand = _candidates(40 + r, nq, n_cand)
        cand[r, 3] = -1
        qr = np.roll(np.array(q), r, axis=0)
        qt.copy_(torch.from_numpy(qr))
        ct.copy_(torch.from_numpy(cand))
        graph.replay()
        torch.cuda.synchronize()
        replay = tuple(o.cpu().numpy().copy() for o in out)
        eager = _run(qr, docs_t, cand, k)
        np.testing.assert_array_equal(replay[1], eager[1])
        np.testing.assert_array_equal(_bits(replay[0]), _bits(eager[0]))
        np.testing.assert_array_equal(replay[2], eager[2])
        _check(replay, rc.refine_expected(qr, d, cand, k), k, f"replay {r}")


def test_every_score_body_gives_the_same_bits(cuda):
    """mevi_refine_topk_set_score_body: the measurement's other body (the fine stage's slab loop) returns what the shipped one does."""
    dim, n_cand, k = 100, 300, 300
    d, q = _corpus(dim)
    cand = _candidates(13, 5, n_cand)
    cand[0, 200:] = -1
    want = rc.refine_expected(q, d, cand, k)
    L = hip.lib()
    try:
        for body in (1, 0):
            L.mevi_refine_topk_set_score_body(body)
            _check(_run(q, _docs_on(dim), cand, k), want, k, f"body {body}")
    finally:
        L.mevi_refine_topk_set_score_body(0)
