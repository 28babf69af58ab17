"""One level of the residual quantiser's beam-search encoder (mevi_rq_errbeam_step_f32 through dense.rq_errbeam_step) and the backtrack
(mevi_rq_errbeam_codes_u8) against tests/rq_errbeam_cases.py.  Bar: parents and codes equal, errors and residual rows identical as
uint32 bits; no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

import rq_errbeam_cases as ec
from mevi_amd import dense, hip, rqindex

pytestmark = pytest.mark.gpu

# (dim, K, B, L, n); n in documents per ticket T: "1", "T-1", "T+1", "3T+7".  dim 4 / 36 / 100 / 768: one short slab, a slab tail, three slabs
# and a tail, 24 slabs; K 1 / 2 / 33 / 64 / 65 / 256 and 128 / 129: the chunk edges of both tiles and the threshold between them;
# Lo == B * K (K = 2, B = 2, L = 5) and L > B * K.
CASES = [
    (4, 1, 1, 1, "1"), (4, 2, 2, 5, "T+1"), (4, 2, 1, 5, "3T+7"), (4, 256, 16, 1, "3T+7"), (4, 64, 5, 16, "T+1"), (4, 65, 1, 1, "T-1"),
    (36, 16, 5, 5, "T-1"), (36, 16, 5, 5, "3T+7"), (36, 33, 2, 16, "T+1"), (36, 64, 16, 16, "1"), (36, 65, 16, 5, "T+1"),
    (36, 1, 1, 16, "3T+7"), (36, 2, 5, 16, "T+1"), (36, 256, 2, 5, "3T+7"),
    (100, 33, 5, 5, "3T+7"), (100, 64, 1, 5, "T+1"), (100, 65, 2, 1, "T-1"), (100, 256, 5, 5, "T+1"), (100, 256, 16, 16, "3T+7"),
    (100, 2, 2, 5, "1"), (100, 128, 5, 5, "T+1"), (100, 129, 5, 5, "T+1"),
    (768, 256, 5, 5, "T+1"), (768, 256, 16, 16, "T-1"), (768, 256, 1, 16, "T+1"), (768, 64, 5, 5, "3T+7"), (768, 1, 5, 5, "T+1"),
    (768, 2, 16, 16, "T-1"), (768, 33, 16, 5, "T+1"), (768, 65, 2, 16, "3T+7"),
]


def _n(case):
    dim, K, B, L, n = case
    T = dense.rq_errbeam_step_tile_docs(dim, K, B, L)
    assert T >= 4
    return {"1": 1, "T-1": T - 1, "T+1": T + 1, "3T+7": 3 * T + 7}[n]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    dim, K, B, L, _ = case
    return ec.random_step(hash(case[:4]) % 1000 + len(case[4]), _n(case), B, dim, K)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want, res=True):
    torch.cuda.synchronize()
    parent, code, err, out = got
    assert parent.dtype == torch.uint8 and code.dtype == torch.uint8 and parent.shape == want[0].shape
    np.testing.assert_array_equal(parent.cpu().numpy(), want[0])
    np.testing.assert_array_equal(code.cpu().numpy(), want[1])
    if err is not None:
        np.testing.assert_array_equal(_bits(err.cpu().numpy()), _bits(want[2]))
    if res:
        assert out.shape == want[3].shape
        np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(want[3]))
    else:
        assert out is None


def _raw_step(x, cent, L, err=True, res=True, guard=64):
    """The C call with every output between `guard` sentinel elements, which it must leave alone."""
    n, B, dim = x.shape
    K = cent.shape[0]
    Lo = min(L, B * K)
    dev = x.device
    bufs = {"parent": torch.full((n * Lo + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev),
            "code": torch.full((n * Lo + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev),
            "err": torch.full((n * Lo + 2 * guard,), -7.0, dtype=torch.float32, device=dev),
            "out": torch.full((n * Lo * dim + 2 * guard,), -7.0, dtype=torch.float32, device=dev)}
    ws = torch.empty(dense.rq_errbeam_step_workspace_bytes(n, dim, K, B, L), dtype=torch.uint8, device=dev)

    def at(name, wanted=True):
        return bufs[name].data_ptr() + guard * bufs[name].element_size() if wanted else None

    st = hip.lib().mevi_rq_errbeam_step_f32(hip.ptr(x), n, B, dim, hip.ptr(cent), K, L, at("parent"), at("code"), at("err", err), at("out", res),
                                            hip.ptr(ws), ws.numel(), hip.stream_ptr())
    hip.check(st, "mevi_rq_errbeam_step_f32")
    torch.cuda.synchronize()
    for name, t in bufs.items():
        fill = t[0].item()
        assert (t[:guard] == fill).all() and (t[-guard:] == fill).all(), name
        if (name == "err" and not err) or (name == "out" and not res):
            assert (t == fill).all(), name
    inner = {k: t[guard:-guard] for k, t in bufs.items()}
    return (inner["parent"].view(n, Lo), inner["code"].view(n, Lo), inner["err"].view(n, Lo) if err else None,
            inner["out"].view(n, Lo, dim) if res else None)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "dim%d-K%d-B%d-L%d-n%s" % c)
def test_step_equals_the_reference_bit_for_bit(cuda, case):
    x, cent = _inputs(case)
    want = ec.step_expected(x, cent, case[3])
    dx, dc = torch.from_numpy(x).to(cuda), torch.from_numpy(cent).to(cuda)
    _same(dense.rq_errbeam_step(dx, dc, case[3]), want)
    np.testing.assert_array_equal(_bits(dx.cpu().numpy()), _bits(x))          # the rows read are left alone


def test_the_case_table_reaches_what_it_names():
    assert 25 <= len(CASES) <= 35 and len(set(CASES)) == len(CASES)
    assert {c[0] for c in CASES} == {4, 36, 100, 768} and {c[1] for c in CASES} >= {1, 2, 33, 64, 65, 128, 129, 256}
    assert {c[2] for c in CASES} == {1, 2, 5, 16} and {c[3] for c in CASES} == {1, 5, 16} and {c[4] for c in CASES} == {"1", "T-1", "T+1", "3T+7"}
    assert (4, 2, 2, 5, "T+1") in CASES                                     # Lo == B * K
    assert any(L > B * K for _, K, B, L, _ in CASES)


def test_ties_are_ordered_by_beam_and_code(cuda):
    """Duplicated centroid rows, duplicated beam rows and all-zero rows: equal errors, kept in b * K + c order."""
    x, cent = ec.random_step(21, 30, 5, 36, 16)
    cent[9], cent[15] = cent[2], cent[2]
    x[:, 4] = x[:, 1]
    x[::3] = 0.0
    x[1::6, :] = x[1::6, :1]                                                # every beam row the same
    for L in (5, 16):
        want = ec.step_expected(x, cent, L)
        assert (np.diff(want[2], axis=1) == 0).mean() > 0.2
        _same(_raw_step(torch.from_numpy(x).to(cuda), torch.from_numpy(cent).to(cuda), L), want)
    zero = np.zeros((7, 16, 100), np.float32)                               # nothing but ties: 4096 equal keys, the first 16 in order
    c0 = np.zeros((256, 100), np.float32)
    got = dense.rq_errbeam_step(torch.from_numpy(zero).to(cuda), torch.from_numpy(c0).to(cuda), 16)
    _same(got, ec.step_expected(zero, c0, 16))
    assert (got[0] == 0).all() and (got[1].cpu() == torch.arange(16, dtype=torch.uint8)).all()


def test_optional_outputs_and_guard_bands(cuda):
    """res_out = null and err = null leave the other outputs identical; nothing is written outside an output."""
    for case in ((36, 16, 5, 5, "3T+7"), (100, 256, 16, 16, "T+1"), (768, 33, 1, 5, "T-1")):
        x, cent = _inputs(case)
        want = ec.step_expected(x, cent, case[3])
        dx, dc = torch.from_numpy(x).to(cuda), torch.from_numpy(cent).to(cuda)
        _same(_raw_step(dx, dc, case[3]), want)
        _same(_raw_step(dx, dc, case[3], res=False), want, res=False)
        _same(_raw_step(dx, dc, case[3], err=False), want)
        _same(dense.rq_errbeam_step(dx, dc, case[3], want_res=False), want, res=False)


def test_two_steps_back_to_back_without_a_sync(cuda):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((150, 1, 100)).astype(np.float32)
    book = rng.standard_normal((2, 64, 100)).astype(np.float32)
    first = ec.step_expected(x, book[0], 5)
    second = ec.step_expected(first[3], book[1], 5)
    dx, db = torch.from_numpy(x).to(cuda), torch.from_numpy(book).to(cuda)
    ws = torch.empty(dense.rq_errbeam_step_workspace_bytes(150, 100, 64, 5, 5), dtype=torch.uint8, device=cuda)
    a = dense.rq_errbeam_step(dx, db[0], 5, workspace=ws)                   # one workspace: the calls are ordered by the stream
    b = dense.rq_errbeam_step(a[3], db[1], 5, workspace=ws)
    _same(b, second)
    _same(a, first)


def test_no_documents_is_no_launch(cuda):
    dc = torch.zeros((16, 36), device=cuda)
    parent, code, err, out = dense.rq_errbeam_step(torch.zeros((0, 5, 36), device=cuda), dc, 5)
    assert parent.shape == code.shape == err.shape == (0, 5) and out.shape == (0, 5, 36)
    assert dense.rq_errbeam_codes(torch.zeros((3, 0, 5), dtype=torch.uint8, device=cuda), torch.zeros((3, 0, 5), dtype=torch.uint8, device=cuda),
                                  0).shape == (0, 3)


def test_a_three_level_walk_is_captured_and_replayed(cuda):
    """Three steps over ping-pong buffers and the backtrack, captured on one stream, replayed twice on new rows."""
    rng = np.random.default_rng(4)
    n, dim, K, L = 77, 36, 16, 5
    book = rng.standard_normal((3, K, dim)).astype(np.float32) * (0.7 ** np.arange(3))[:, None, None].astype(np.float32)
    db = torch.from_numpy(book).to(cuda)
    x = torch.zeros((n, 1, dim), device=cuda)
    bufs = [torch.empty((n, L, dim), device=cuda) for _ in range(2)]
    ws = torch.empty(dense.rq_errbeam_step_workspace_bytes(n, dim, K, L, L), dtype=torch.uint8, device=cuda)
    trace = torch.zeros((2, 3, n, L), dtype=torch.uint8, device=cuda)
    codes = torch.empty((n, 3), dtype=torch.uint8, device=cuda)

    def walk():
        cur = x
        for j in range(3):
            parent, code, _, cur = dense.rq_errbeam_step(cur, db[j], L, res_out=bufs[j & 1] if j < 2 else None, want_res=j < 2, workspace=ws)
            trace[0, j].copy_(parent)
            trace[1, j].copy_(code)
        dense.rq_errbeam_codes(trace[0], trace[1], n, out=codes)

    walk()                                                                   # eagerly first: it loads the kernels
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        walk()
    for seed in (5, 6):
        rows = np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)
        x.copy_(torch.from_numpy(rows).to(cuda).view(n, 1, dim))
        codes.zero_()
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(codes.cpu().numpy(), ec.walk_expected(rows, book, L))


def test_the_composition_returns_the_same_bits(cuda, monkeypatch):
    """MEVI_RQINDEX_BEAM_STEP=steps: mevi_rq_neg_dist_f32 -> torch.sort of the packed keys -> mevi_gather_sub_f32."""
    monkeypatch.setenv("MEVI_RQINDEX_BEAM_STEP", "steps")
    for case in ((36, 16, 5, 5, "3T+7"), (4, 2, 2, 5, "T+1"), (100, 256, 16, 16, "T+1"), (768, 65, 2, 16, "3T+7"), (36, 1, 1, 16, "3T+7")):
        x, cent = _inputs(case)
        want = ec.step_expected(x, cent, case[3])
        dx, dc = torch.from_numpy(x).to(cuda), torch.from_numpy(cent).to(cuda)
        assert not rqindex.beam_step_is_fused(len(x), case[0], case[1], case[2], case[3])
        _same(rqindex.beam_step(dx, dc, case[3]), want)
        _same(rqindex.beam_step(dx, dc, case[3], want_res=False), want, res=False)
    x, cent = ec.random_step(8, 20, 5, 36, 16)
    x[::2] = 0.0
    cent[5] = cent[1]
    _same(rqindex.beam_step(torch.from_numpy(x).to(cuda), torch.from_numpy(cent).to(cuda), 16), ec.step_expected(x, cent, 16))
    monkeypatch.delenv("MEVI_RQINDEX_BEAM_STEP")
    assert rqindex.beam_step_is_fused(20, 36, 16, 5, 16)


@pytest.mark.parametrize("L", [1, 5, 16])
@pytest.mark.parametrize("M", [1, 2, 9, 64])
def test_backtrack_equals_the_reference(cuda, M, L):
    """row_stride > Lo (the slots behind hold parents never to be followed) and code_stride > M (the columns behind are left alone)."""
    n, S = 1000, L + 3
    parent, code = ec.random_trace(M * 100 + L, M, n, L, S)
    want = ec.codes_expected(parent, code)
    dp, dcode = torch.from_numpy(parent).to(cuda), torch.from_numpy(code).to(cuda)
    got = dense.rq_errbeam_codes(dp, dcode, n)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    wide = torch.full((n, M + 5), 0xEE, dtype=torch.uint8, device=cuda)
    back = dense.rq_errbeam_codes(dp, dcode, n, out=wide)
    torch.cuda.synchronize()
    assert back is wide
    np.testing.assert_array_equal(wide[:, :M].cpu().numpy(), want)
    assert (wide[:, M:] == 0xEE).all()
