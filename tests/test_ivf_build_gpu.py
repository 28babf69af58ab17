"""The IVF-Flat build on the device (mevi_ivf_assign_f32, mevi_ivf_build_lists; mevi_amd/ivf.py: assign, IVFFlatIndex) against
oracle.dense.ip_topk_exact and numpy's stable argsort (tests/ivf_build_cases.py).  Bar: labels identical, best scores
identical as uint32 bits, offsets / ids / longest list exact, nothing written outside the outputs."""
import numpy as np
import pytest
import torch

import ivf_build_cases as bc
from mevi_amd import dense, hip, ivf
from oracle import dense as odense

pytestmark = pytest.mark.gpu


def _assign_equals(cuda, x, cent, want=None, with_score=True):
    want = bc.nearest(x, cent) if want is None else want
    xt, ct = torch.from_numpy(x).to(cuda), torch.from_numpy(cent).to(cuda)
    out = (torch.full((len(x),), -7, dtype=torch.int32, device=cuda),
           torch.full((len(x),), np.nan, dtype=torch.float32, device=cuda) if with_score else None)
    lab, score = dense.ivf_assign(xt, ct, out=out)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(lab.cpu().numpy(), want[0])
    if with_score:
        np.testing.assert_array_equal(score.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    return want


@pytest.mark.parametrize("dim", bc.ASSIGN_DIM)
def test_assign_equals_the_oracle_at_the_tile_edges(cuda, dim):
    x, cent = bc.normal(dim, max(bc.ASSIGN_N), dim), bc.normal(dim + 1, max(bc.ASSIGN_NLIST), dim)
    for nlist in bc.ASSIGN_NLIST:
        full = bc.nearest(x, cent[:nlist])                                  # one oracle run per centroid set: rows are independent
        for n in bc.ASSIGN_N:
            _assign_equals(cuda, x[:n], cent[:nlist], (full[0][:n], full[1][:n]))


@pytest.mark.parametrize("n,nlist,dim", [
    (dense.IVF_ASSIGN_ROWS * (dense.IVF_ASSIGN_SPLIT_WGS // 2) - 3, 129, 28),      # 128 row blocks x 2 tiles of 128: the walk is split in two
    (dense.IVF_ASSIGN_ROWS * (dense.IVF_ASSIGN_SPLIT_WGS // 2) - 3, 257, 36),      # ... in two parts of 1 and 2 tiles
    (dense.IVF_ASSIGN_ROWS * (dense.IVF_ASSIGN_SPLIT_WGS - 1) + 1, 127, 36),       # 256 row blocks: one workgroup walks every tile
    (dense.IVF_ASSIGN_ROWS * (dense.IVF_ASSIGN_SPLIT_WGS - 1) + 1, 128, 4),
    (dense.IVF_ASSIGN_ROWS * (dense.IVF_ASSIGN_SPLIT_WGS - 1) + 1, 129, 64),
])
def test_assign_in_tiles_of_128_columns(cuda, n, nlist, dim):
    """The tile edges above have so few row blocks that they run in 64-column tiles; these have enough for the wide ones."""
    _assign_equals(cuda, bc.normal(n % 97, n, dim), bc.normal(nlist, nlist, dim))


def test_assign_at_model_width(cuda):
    _assign_equals(cuda, bc.normal(1, 600, 768), bc.normal(2, 130, 768))


@pytest.mark.parametrize("n", [120, dense.IVF_ASSIGN_ROWS * (dense.IVF_ASSIGN_SPLIT_WGS - 1) + 1])
def test_assign_gives_ties_to_the_lowest_index(cuda, n):
    """120 rows: the centroid walk is split among workgroups (64-column tiles), the parts meet in the combine kernel; 65281 rows:
    one workgroup walks all three 128-column tiles with its running best in registers."""
    x, cent, winner = bc.tie_case(n)
    want = _assign_equals(cuda, x, cent)
    np.testing.assert_array_equal(want[0], winner)
    assert ivf.assign(torch.from_numpy(x[:500]).to(cuda), torch.from_numpy(cent).to(cuda)).cpu().numpy().tolist() == winner[:500].tolist()


@pytest.mark.parametrize("name", sorted(bc.range_cases()))
def test_assign_sign_range_and_padded_columns(cuda, name):
    x, cent = bc.range_cases()[name]
    lab, _ = _assign_equals(cuda, x, cent)
    assert lab.min() >= 0 and lab.max() < len(cent)


def test_assign_more_row_blocks_than_resident_workgroups(cuda):
    """Two rounds of workgroups on every CU and a ragged tail of one row; with and without best_score, and on a side stream."""
    n_cu = torch.cuda.get_device_properties(cuda).multi_processor_count
    n, dim, nlist = 2 * n_cu * dense.IVF_ASSIGN_ROWS + 1, 32, 70
    x, cent = bc.normal(5, n, dim), bc.normal(6, nlist, dim)
    want = _assign_equals(cuda, x, cent)
    _assign_equals(cuda, x, cent, want, with_score=False)
    xt, ct = torch.from_numpy(x).to(cuda), torch.from_numpy(cent).to(cuda)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        lab, score = dense.ivf_assign(xt, ct)
    side.synchronize()
    np.testing.assert_array_equal(lab.cpu().numpy(), want[0])
    np.testing.assert_array_equal(score.cpu().numpy().view(np.uint32), want[1].view(np.uint32))


GUARD = 64          # int64 guard words around every output


def _build_lists_guarded(cuda, lab_t, nlist, ws):
    """The raw call with sentinel-filled outputs inside guard words -> (offsets, row_ids incl. unwritten slots, longest)."""
    n = lab_t.numel()
    L = hip.lib()
    sizes = (nlist + 1, n, 1)
    buf = torch.full((sum(sizes) + GUARD * (len(sizes) + 1),), -99, dtype=torch.int64, device=cuda)
    views, at = [], GUARD
    for s in sizes:
        views.append(buf[at:at + s])
        at += s + GUARD
    st = L.mevi_ivf_build_lists(hip.ptr(lab_t), n, nlist, hip.ptr(views[0]), hip.ptr(views[1]), hip.ptr(views[2]), hip.ptr(ws), ws.numel(),
                                hip.stream_ptr())
    hip.check(st, "mevi_ivf_build_lists")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    mask = np.ones(len(host), bool)
    at = GUARD
    outs = []
    for s in sizes:
        outs.append(host[at:at + s].copy())
        mask[at:at + s] = False
        at += s + GUARD
    assert (host[mask] == -99).all()                                        # the words around every output are untouched
    return outs


@pytest.mark.parametrize("nlist", bc.LISTS_NLIST)
def test_build_lists_equals_the_stable_argsort(cuda, nlist):
    ws = torch.empty(dense.ivf_build_lists_workspace_bytes(max(bc.LISTS_N), nlist), dtype=torch.uint8, device=cuda)
    for n in bc.LISTS_N:
        assert dense.ivf_build_lists_workspace_bytes(n, nlist) <= ws.numel()
        for pattern in bc.LISTS_PATTERNS:
            lab = bc.labels(pattern, n, nlist)
            off, ids, longest = bc.lists(lab, nlist)
            lab_t = torch.from_numpy(lab).to(cuda)
            for _ in range(2 if n in (1025, 65537) else 1):                 # a second call on the same workspace: the same answer
                got_off, got_ids, got_longest = _build_lists_guarded(cuda, lab_t, nlist, ws)
                np.testing.assert_array_equal(got_off, off, err_msg=f"{pattern} n={n}")
                np.testing.assert_array_equal(got_ids[:len(ids)], ids, err_msg=f"{pattern} n={n}")
                assert (got_ids[len(ids):] == -99).all(), (pattern, n)      # the slots of the dropped rows are not written
                assert got_longest[0] == longest, (pattern, n)
    lab = bc.labels("skewed", 4000, nlist)                                  # the wrapper, with its own workspace
    off, ids, longest = bc.lists(lab, nlist)
    got = dense.ivf_build_lists(torch.from_numpy(lab).to(cuda), nlist)
    assert got[0].cpu().numpy().tolist() == off.tolist() and got[1].cpu().numpy().tolist() == ids.tolist() and int(got[2]) == longest


def test_build_lists_of_no_rows(cuda):
    off, ids, longest = dense.ivf_build_lists(torch.empty(0, dtype=torch.int32, device=cuda), 37)
    assert off.cpu().numpy().tolist() == [0] * 38 and ids.numel() == 0 and int(longest) == 0


def _index_docs(kind):
    rng = np.random.default_rng(31)
    if kind == "clustered":
        centres = rng.standard_normal((12, 32)).astype(np.float32) * 2
        d = (centres[rng.integers(0, 12, size=3000)] + rng.standard_normal((3000, 32))).astype(np.float32)
    else:                                                                   # 5 distinct rows: k-means leaves lists empty and repairs them
        d = rng.standard_normal((5, 32)).astype(np.float32)[rng.integers(0, 5, size=3000)]
    q = (d[rng.integers(0, 3000, size=40)] + 0.3 * rng.standard_normal((40, 32))).astype(np.float32)
    return d, q


@pytest.mark.parametrize("kind,nlist", [("clustered", 8), ("clustered", 37), ("duplicates", 8)])
def test_index_through_the_kernels_equals_the_host_build_and_the_oracle(cuda, monkeypatch, kind, nlist):
    d, q = _index_docs(kind)
    dt, qt = torch.from_numpy(d).to(cuda), torch.from_numpy(q).to(cuda)
    monkeypatch.setenv("MEVI_IVF_BUILD", "host")
    host = ivf.IVFFlatIndex(dt, nlist)
    monkeypatch.delenv("MEVI_IVF_BUILD")
    assert ivf.assign_wanted(3000, 32, nlist)
    index = ivf.IVFFlatIndex(dt, nlist)
    torch.cuda.synchronize()
    for name in ("centroids", "list_of", "offsets", "offsets_dev", "ids", "docs", "centroid_offsets"):
        a, b = getattr(index, name), getattr(host, name)
        assert a.dtype == b.dtype and a.device == b.device and a.shape == b.shape, name
        va, vb = a.cpu().numpy(), b.cpu().numpy()
        np.testing.assert_array_equal(va.view(np.uint32) if va.dtype == np.float32 else va, vb.view(np.uint32) if vb.dtype == np.float32 else vb,
                                      err_msg=name)
    assert index.max_list_len == host.max_list_len and type(index.max_list_len) is int
    assert index.offsets.device.type == "cpu" and index.ids.dtype == torch.int64 and index.list_of.dtype == torch.int32
    sizes = np.diff(index.offsets.numpy())
    if kind == "duplicates":
        assert (sizes == 0).any()                                           # the case does leave lists empty
    for nprobe, k in ((1, 10), (min(3, nlist), 50)):
        want = odense.ivf_flat_search(q, d, index.centroids.cpu().numpy(), k, nprobe)
        np.testing.assert_array_equal(index.list_of.cpu().numpy(), want[2])
        s, i = index.search(qt, k, nprobe)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(i.cpu().numpy(), want[1])
        np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
