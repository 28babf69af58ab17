"""mevi_opq_rotate_rows_f32 (csrc/opq_rotate.hip, dense.opq_rotate_rows) bit for bit -- outputs compared as uint32 -- against
tests/opq_cases.py: rotate_expected (the oracle's chain and one np.float32 subtraction) and against the `steps` composition of
existing calls, at the edges of the 128-row group and the 256-row workgroup, of the 64- and 128-column tiles and of the 32-k
slab; the gather, the centroid subtraction, out-of-range rows and lists, the rows of `out` past n, the refusals and a replayed
graph."""
import numpy as np
import pytest
import torch

import opq_cases as oc
from mevi_amd import dense, hip

pytestmark = pytest.mark.gpu
GUARD = 12345.0


def _case(seed, n, dim, nlist):
    """(x [n + 5, dim], R, crot [nlist, dim], list_of): R is any matrix here, the kernel does not need it orthonormal."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n + 5, dim)).astype(np.float32)
    R = rng.standard_normal((dim, dim)).astype(np.float32)
    crot = rng.standard_normal((max(nlist, 1), dim)).astype(np.float32)
    list_of = rng.integers(0, max(nlist, 1), size=n + 5).astype(np.int32)
    return rng, x, R, crot, list_of


def _run(cuda, x, R, rows, list_of, crot, n_rows=None):
    """The fused call into a guarded buffer and the `steps` composition; both as numpy, the guard rows checked."""
    xt, Rt, rt, lt, ct = (None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (x, R, rows, list_of, crot))
    n = len(x) if rows is None else len(rows)
    buf = torch.full((n + 3, x.shape[1]), GUARD, dtype=torch.float32, device=cuda)
    out = dense.opq_rotate_rows(xt, rt, lt, ct, Rt, out=buf[:n], mode="fused")
    steps = dense.opq_rotate_rows(xt, rt, lt, ct, Rt, mode="steps")
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() and (buf[n:] == GUARD).all()            # rows past n are not written
    return out.cpu().numpy(), steps.cpu().numpy()


def _same(got, want):
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("dim", [32, 48, 96, 160])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 257])
def test_rotate_equals_the_reference_and_the_steps(cuda, n, dim):
    rng, x, R, crot, list_of = _case(1000 * dim + n, n, dim, 7)
    n_src = len(x)
    chains = oc.rotate_expected(x, R)                                               # every source row's chain, once
    # rows NULL, no centroids: row i of the first n
    got, steps = _run(cuda, x[:n], R, None, None, None)
    _same(got, chains[:n])
    _same(steps, chains[:n])
    # a gather with repeats, 7 lists
    rows = rng.integers(0, n_src, size=n).astype(np.int64)
    if n > 1:
        rows[1] = rows[0]
    want = oc.rotate_expected(x, R, rows, list_of, crot)
    _same(want, chains[rows] - crot[list_of[rows]])                                 # the chain, then one f32 subtraction
    got, steps = _run(cuda, x, R, rows, list_of, crot)
    _same(got, want)
    _same(steps, want)
    # rows NULL with one list
    one = np.zeros(n, np.int32)
    got, steps = _run(cuda, x[:n], R, None, one, crot[:1])
    _same(got, chains[:n] - crot[0])
    _same(steps, got)
    # a gather without centroids
    got, _ = _run(cuda, x, R, rows, None, None)
    _same(got, chains[rows])


@pytest.mark.parametrize("n,dim", [(129, 48), (257, 96)])
def test_out_of_range_rows_and_lists_give_zero_rows(cuda, n, dim):
    rng, x, R, crot, list_of = _case(77 + n, n, dim, 7)
    n_src = len(x)
    rows = rng.permutation(n_src)[:n].astype(np.int64)
    rows[0], rows[n // 2], rows[n - 1] = -1, n_src, -(1 << 40)
    bad = list_of.copy()
    bad[rows[1]], bad[rows[2]] = -1, 7
    want = oc.rotate_expected(x, R, rows, bad, crot)
    zero = [0, 1, 2, n // 2, n - 1]
    assert (want[zero] == 0).all() and (np.abs(want).max(1) > 0).sum() == n - len(zero)
    got, steps = _run(cuda, x, R, rows, bad, crot)
    _same(got, want)                                                                # zero rows, and nothing else is disturbed
    _same(steps, want)
    got, _ = _run(cuda, x, R, rows, None, None)                                     # without centroids only the row id counts
    assert (got[[0, n // 2, n - 1]] == 0).all() and (np.abs(got).max(1) > 0).sum() == n - 3
    # rows NULL with a bad list
    got, _ = _run(cuda, x, R, None, bad, crot)
    _same(got, oc.rotate_expected(x, R, None, bad, crot))
    # an empty source: every row id is out of range, nothing of x is read
    empty = torch.empty((0, dim), dtype=torch.float32, device=cuda)
    out = dense.opq_rotate_rows(empty, torch.zeros(5, dtype=torch.int64, device=cuda), None, None, torch.from_numpy(R).to(cuda))
    assert out.shape == (5, dim) and (out == 0).all()


def test_full_width_case(cuda):
    """n = 300, dim = 768: 24 slabs, two row pairs, the production width."""
    n, dim = 300, 768
    rng, x, R, crot, list_of = _case(5, n, dim, 7)
    rows = rng.integers(0, len(x), size=n).astype(np.int64)
    want = oc.rotate_expected(x, R, rows, list_of, crot)
    got, steps = _run(cuda, x, R, rows, list_of, crot)
    _same(got, want)
    _same(steps, want)


def test_refusals_and_empty_call(cuda):
    oc.check_refusals(hip.lib())
    x = torch.zeros((4, 32), dtype=torch.float32, device=cuda)
    R = torch.eye(32, dtype=torch.float32, device=cuda)
    out = dense.opq_rotate_rows(x, torch.zeros(0, dtype=torch.int64, device=cuda), None, None, R)
    assert out.shape == (0, 32)
    with pytest.raises(hip.MeviHipError, match="opq_rotate: dim=34"):
        dense.opq_rotate_rows(torch.zeros((4, 34), dtype=torch.float32, device=cuda), None, None, None,
                              torch.zeros((34, 34), dtype=torch.float32, device=cuda))
    with pytest.raises(ValueError):
        dense.opq_rotate_rows(x, None, None, None, R, mode="other")


def test_one_call_inside_a_replayed_graph(cuda):
    n, dim = 129, 96
    rng, x, R, crot, list_of = _case(9, n, dim, 7)
    xt = torch.from_numpy(x).to(cuda)
    rt = torch.zeros(n, dtype=torch.int64, device=cuda)
    lt, ct, Rt = torch.from_numpy(list_of).to(cuda), torch.from_numpy(crot).to(cuda), torch.from_numpy(R).to(cuda)
    out = torch.zeros((n, dim), dtype=torch.float32, device=cuda)
    dense.opq_rotate_rows(xt, rt, lt, ct, Rt, out=out, mode="fused")                # loads the kernel outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dense.opq_rotate_rows(xt, rt, lt, ct, Rt, out=out, mode="fused")
    for r in range(2):
        rows = rng.integers(0, len(x), size=n).astype(np.int64)
        x2 = (x * np.float32(r + 2)).astype(np.float32)
        rt.copy_(torch.from_numpy(rows))
        xt.copy_(torch.from_numpy(x2))
        graph.replay()
        torch.cuda.synchronize()
        _same(out.cpu().numpy(), oc.rotate_expected(x2, R, rows, list_of, crot))
