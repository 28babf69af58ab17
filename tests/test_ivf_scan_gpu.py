"""The IVF-Flat device scan (mevi_ivf_scan_topk_f32; mevi_amd/ivf.py: IVFFlatIndex.search_scan / search / search_graph)
against oracle.dense.ivf_flat_search given the index's centroids.  Bar: scores identical as uint32 bits, ids identical --
both sides compute the sequential fmaf chain and order by (score desc, id asc), padding -FLT_MAX / -1."""
import numpy as np
import pytest
import torch

from mevi_amd import dense, ivf
from oracle import dense as odense

pytestmark = pytest.mark.gpu

PT, RB = dense.IVF_PAIR_TILE, dense.IVF_ROW_BLOCK


def _clustered(seed, nd, nq, dim):
    """The generator of test_ivf_flat_equals_the_oracle_given_its_centroids: 12 centres, unit noise."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((12, dim)).astype(np.float32) * 2
    d = (centres[rng.integers(0, 12, size=nd)] + rng.standard_normal((nd, dim))).astype(np.float32)
    q = (centres[rng.integers(0, 12, size=nq)] + rng.standard_normal((nq, dim))).astype(np.float32)
    return d, q


def _same(got, want):
    s, i = got
    torch.cuda.synchronize()
    np.testing.assert_array_equal(i.cpu().numpy(), want[1])
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), want[0].view(np.uint32))


def _check_index(cuda, d, q, centroids, k, nprobe):
    """The scan through the index (coarse call + scan call) equals the oracle; returns (index, oracle result)."""
    index = ivf.IVFFlatIndex(torch.from_numpy(d).to(cuda), len(centroids), centroids=torch.from_numpy(centroids))
    want = odense.ivf_flat_search(q, d, centroids, k, nprobe)
    assert np.array_equal(index.list_of.cpu().numpy(), want[2])
    assert index.scan_wanted(len(q), k, nprobe)
    _same(index.search_scan(torch.from_numpy(q).to(cuda), k, nprobe), want)
    if nprobe == len(centroids):
        fs, fi = odense.ip_topk_exact(q, d, k)
        np.testing.assert_array_equal(want[1], fi)
        np.testing.assert_array_equal(want[0].view(np.uint32), fs.view(np.uint32))
    return index, want


@pytest.mark.parametrize("dim,nq,nd,nlist,nprobe,k", [
    (64, 1, 3000, 8, 1, 10),
    (64, 1, 3000, 8, 8, 4096),         # one query, every list, k > nd: padding
    (64, 33, 5000, 8, 3, 1000),
    (64, 33, 3000, 5, 5, 1),
    (100, 90, 4000, 6, 6, 4096),       # dim % 32 != 0; k > nd
    (100, 90, 4000, 9, 1, 1000),       # k above the rows of a list: padding
    (768, 257, 3000, 10, 3, 10),
    (768, 257, 3000, 10, 1, 1),
])
def test_scan_equals_the_oracle_over_shapes(cuda, dim, nq, nd, nlist, nprobe, k):
    d, q = _clustered(dim * 7 + nq + nprobe, nd, nq, dim)
    _, want = _check_index(cuda, d, q, d[:nlist].copy(), k, nprobe)
    if k > nd or (nprobe == 1 and k == 1000):
        assert (want[1] == -1).any()                                   # the case does pad


def _axis_corpus(sizes, aims, dim=64, seed=5):
    """Hand-made lists: centroid l = 10 e_l; a document of list l = (5 + u) e_l + noise below 1 elsewhere, so its best centroid
    is l; a query aimed at list l likewise, with -5 on axis 4 so that list 4 is never among the best two."""
    rng = np.random.default_rng(seed)
    nlist = len(sizes)
    cent = np.zeros((nlist, dim), np.float32)
    cent[np.arange(nlist), np.arange(nlist)] = 10.0

    def rows(labels, avoid):
        x = (rng.random((len(labels), dim), dtype=np.float32) - 0.5)
        x[np.arange(len(labels)), labels] = 5.0 + rng.random(len(labels), dtype=np.float32)
        if avoid:
            x[labels != 4, 4] = -5.0
        return x

    lab = rng.permutation(np.repeat(np.arange(nlist), sizes))
    return rows(lab, False), rows(np.repeat(np.arange(nlist), aims), True), cent


@pytest.mark.parametrize("nprobe,k", [(1, 10), (1, 1000), (2, 10), (2, 1000)])
def test_scan_over_hand_made_list_geometry(cuda, nprobe, k):
    """An empty list (0), a list of one row (1), one list with 90 % of the rows (2), a list one row longer than the row block
    (3), a list no query probes (4), a list probed by one query more than the pair tile (5)."""
    sizes = [0, 1, 5400, RB + 1, 100, 200, 6000 - 5400 - 1 - (RB + 1) - 100 - 200]
    aims = [10, 5, 20, 10, 0, PT + 1, 10]
    d, q, cent = _axis_corpus(sizes, aims)
    index, want = _check_index(cuda, d, q, cent, k, nprobe)
    assert (index.offsets[1:] - index.offsets[:-1]).tolist() == sizes and index.max_list_len == 5400
    probe = odense.ip_topk_exact(q, cent, nprobe)[1]
    counts = np.bincount(probe.ravel(), minlength=len(sizes))
    assert counts[4] == 0 and counts[0] >= 10 and (counts[5] == PT + 1 if nprobe == 1 else counts[5] > PT)
    if nprobe == 1:
        assert (want[1][:10] == -1).all() and (want[1][10:15, 1:] == -1).all() and (want[1][10:15, 0] >= 0).all()


def test_scan_when_every_query_probes_the_same_list(cuda):
    sizes = [300, 2 * RB + 1, 2000, 500, 100]
    d, q, cent = _axis_corpus(sizes, [0, 2 * PT + 3, 0, 0, 0], seed=6)
    _check_index(cuda, d, q, cent, 100, 1)


def _expected_from_probe(q, d, list_of, probe, nlist, k):
    """oracle.dense.ivf_flat_search's selection for a given probe table (entries outside [0, nlist) are empty probes)."""
    out_s = np.full((len(q), k), -odense.FLT_MAX, np.float32)
    out_i = np.full((len(q), k), -1, np.int64)
    for i in range(len(q)):
        lists = [l for l in probe[i] if 0 <= l < nlist]
        rows = np.flatnonzero(np.isin(list_of, lists))
        if rows.size == 0:
            continue
        s = odense.pair_dot(q[i], d[rows])
        order = np.lexsort((rows, -s))[:k]
        out_s[i, :len(order)], out_i[i, :len(order)] = s[order], rows[order]
    return out_s, out_i


def _list_major(cuda, d, list_of, nlist):
    order = np.argsort(list_of, kind="stable")
    off = np.zeros(nlist + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(list_of, minlength=nlist))
    return (torch.from_numpy(d[order]).to(cuda), torch.from_numpy(off).to(cuda), torch.from_numpy(order.astype(np.int64)).to(cuda),
            int(np.diff(off).max()))


def test_probe_table_given_directly(cuda):
    """-1 and out-of-range entries are empty probes, a list named twice counts once, and two runs give the same bytes."""
    nlist, k = 6, 50
    d, q = _clustered(11, 3000, 40, 64)
    rng = np.random.default_rng(3)
    list_of = rng.integers(0, nlist, size=len(d))
    docs, off, ids, longest = _list_major(cuda, d, list_of, nlist)
    probe = rng.integers(0, nlist, size=(len(q), 4)).astype(np.int32)
    probe[::3, 1] = -1
    probe[1::5, 2] = nlist                     # past the last list
    probe[::4, 3] = probe[::4, 0]              # the same list twice
    probe[7] = -1                              # a query that probes nothing
    probe[8] = 2
    qt, pt = torch.from_numpy(q).to(cuda), torch.from_numpy(probe).to(cuda)
    want = _expected_from_probe(q, d, list_of, probe, nlist, k)
    a = dense.ivf_scan_topk(qt, docs, off, ids, longest, pt, k)
    _same(a, want)
    assert (want[1][7] == -1).all()
    b = dense.ivf_scan_topk(qt, docs, off, ids, longest, pt, k)
    torch.cuda.synchronize()
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()
    # row_ids = None: the id is the list-major row
    c = dense.ivf_scan_topk(qt, docs, off, None, longest, pt, k)
    torch.cuda.synchronize()
    rows = c[1].cpu().numpy()
    np.testing.assert_array_equal(np.where(rows >= 0, ids.cpu().numpy()[np.maximum(rows, 0)], -1)[:, 0], want[1][:, 0])


@pytest.mark.parametrize("k", [10, 150])
def test_ties_across_lists_come_out_by_ascending_id(cuda, k):
    """300 bit-identical rows spread over three lists, five rows above them: the k-th place cuts the run of equal scores, and
    the ids of the run must ascend across the lists.  A zero query scores every row +0: the lowest ids win."""
    rng = np.random.default_rng(17)
    d = rng.standard_normal((3000, 64)).astype(np.float32)
    v = rng.standard_normal(64).astype(np.float32)
    copies = rng.choice(3000, size=305, replace=False)
    d[copies[:300]] = v
    d[copies[300:]] = 1.5 * v
    list_of = rng.integers(0, 3, size=3000)
    assert min(np.bincount(list_of[copies[:300]], minlength=3)) > 50
    docs, off, ids, longest = _list_major(cuda, d, list_of, 3)
    q = np.stack([4 * v, np.zeros(64, np.float32), -v]).astype(np.float32)
    probe = np.tile(np.array([2, 0, 1], np.int32), (3, 1))
    want = _expected_from_probe(q, d, list_of, probe, 3, k)
    assert np.array_equal(want[1][0, :5], np.sort(copies[300:])) and np.array_equal(want[1][0, 5:], np.sort(copies[:300])[:k - 5])
    assert np.array_equal(want[1][1], np.arange(k))
    fs, fi = odense.ip_topk_exact(q, d, k)
    assert np.array_equal(fi, want[1]) and np.array_equal(fs.view(np.uint32), want[0].view(np.uint32))
    _same(dense.ivf_scan_topk(torch.from_numpy(q).to(cuda), docs, off, ids, longest, torch.from_numpy(probe).to(cuda), k), want)


@pytest.mark.parametrize("nlist,nprobe,k", [(16, 1, 50), (16, 4, 100), (7, 7, 30), (40, 3, 1000)])
def test_search_equals_search_lists(cuda, nlist, nprobe, k):
    """The device scan and the host loop over lists return the same bits (the parameter sets of the IVF test of test_dense_gpu)."""
    d, q = _clustered(nlist * 31 + nprobe, 6000, 90, 64)
    index = ivf.IVFFlatIndex(torch.from_numpy(d).to(cuda), nlist)
    qt = torch.from_numpy(q).to(cuda)
    a, b, c = index.search(qt, k, nprobe), index.search_lists(qt, k, nprobe), index.search_scan(qt, k, nprobe)
    torch.cuda.synchronize()
    for x in (a, c):
        assert torch.equal(x[1], b[1]) and torch.equal(x[0].view(torch.int32), b[0].view(torch.int32))


def test_search_chooses_its_path(cuda, monkeypatch):
    """`search` takes the device scan inside its envelope, the host loop when MEVI_IVF_SCAN=lists, when nprobe is beyond the
    kernel's 256 and when thousands of queries would make many candidate tiles over few long lists."""
    d, q = _clustered(41, 3000, 5, 64)
    index = ivf.IVFFlatIndex(torch.from_numpy(d).to(cuda), 8, centroids=torch.from_numpy(d[:8].copy()))
    assert index.scan_wanted(5, 10, 2) and index.scan_wanted(6980, 1000, 8)
    monkeypatch.setenv("MEVI_IVF_SCAN", "lists")
    assert not index.scan_wanted(5, 10, 2)
    qt = torch.from_numpy(q).to(cuda)
    _same(index.search(qt, 10, 2), odense.ivf_flat_search(q, d, d[:8], 10, 2))
    monkeypatch.delenv("MEVI_IVF_SCAN")
    assert not index.scan_wanted(5, 10, 257) and not index.scan_wanted(0, 10, 2)
    index.max_list_len = 250000                                  # the regime of a hundred long lists: 2 GiB / (16 x 1 MB) = 134 queries a tile
    assert index.scan_wanted(134 * ivf.SCAN_MAX_TILES, 1000, 16) and not index.scan_wanted(134 * ivf.SCAN_MAX_TILES + 1, 1000, 16)
    index.nlist = ivf.SCAN_ANY_TILES_NLIST
    assert index.scan_wanted(6980, 1000, 16)


def test_nprobe_times_k_above_the_merge_limit(cuda):
    """nprobe 32 x k 1000 > 16384: the scan selects over all probed rows at once, so the merge's limit does not bind."""
    d, q = _clustered(23, 20000, 6, 64)
    index, _ = _check_index(cuda, d, q, d[:64].copy(), 1000, 32)
    assert index.max_list_len < 20000


def test_graph_replay_follows_the_queries(cuda):
    """One captured search of 8 queries, replayed three times with new queries that move to other lists."""
    d, _ = _clustered(29, 3000, 8, 64)
    cent = d[:8].copy()
    index = ivf.IVFFlatIndex(torch.from_numpy(d).to(cuda), 8, centroids=torch.from_numpy(cent))
    graph = index.search_graph(8, 10, 2)
    seen = []
    for r in range(3):
        q = _clustered(100 + r, 8, 8, 64)[1]
        want = odense.ivf_flat_search(q, d, cent, 10, 2)
        _same(graph.run(torch.from_numpy(q).to(cuda)), want)
        seen.append(odense.ip_topk_exact(q, cent, 2)[1])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    with pytest.raises(ValueError):
        index.search_graph(ivf.GRAPH_MAX_QUERIES + 1, 10, 2)
