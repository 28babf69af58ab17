"""The scalar-quantised index end to end (mevi_amd/sq.py) against tests/sq_cases.py: the encoder byte for byte, the range bit for
bit, a flat index pinned completely by its corpus (no seed is involved), an IVF index pinned given its centroids, and the two
routes into it: dense.search and dense.profile."""
import functools

import numpy as np
import pytest
import torch

import sq_cases as sc
from oracle import dense as odense
from mevi_amd import dense, sq

pytestmark = pytest.mark.gpu

ND, DIM, NQ, NLIST = 3000, 48, 21, 8


@functools.lru_cache(maxsize=None)
def _corpus():
    """3000 x 48 rows of very different scale per column and 21 queries, read-only; 8 centroids and the reference's lists."""
    rng = np.random.default_rng(77)
    docs = (rng.standard_normal((ND, DIM)) * rng.uniform(0.05, 3.0, DIM) + rng.uniform(-2, 2, DIM)).astype(np.float32)
    q = rng.standard_normal((NQ, DIM)).astype(np.float32)
    cent = docs[rng.choice(ND, NLIST, replace=False)].copy()
    list_of = odense.ivf_flat_search(q[:1], docs, cent, 1, 1)[2].astype(np.int64)
    for a in (docs, q, cent, list_of):
        a.setflags(write=False)
    return docs, q, cent, list_of


def _dev(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a)).to(cuda)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("gather", [False, True])
def test_encoder_equals_the_reference_byte_for_byte(cuda, bits, residual, gather):
    """With and without residuals, with and without a gather order, over the trained range (so the rows holding each column's
    minimum and maximum are there: levels 0 and L) and over a SUPPLIED narrower range with a zero column (clamping, vdiff == 0)."""
    docs, _, cent, list_of = _corpus()
    cent_, list_ = (cent, list_of) if residual else (None, None)
    rows = np.random.default_rng(3).permutation(ND)[:1111].astype(np.int64) if gather else None
    vmin, vdiff = sc.train_range(docs, list_, cent_)
    narrow = (vmin + np.float32(0.3) * vdiff, np.float32(0.4) * vdiff)
    narrow[1][5] = 0.0
    for lo, df in ((vmin, vdiff), narrow):
        want = sc.encode(docs, lo, df, bits, list_, cent_, rows)
        got = dense.sq_encode(_dev(cuda, docs), _dev(cuda, rows), None if list_ is None else _dev(cuda, list_.astype(np.int32)),
                              _dev(cuda, cent_), _dev(cuda, lo), _dev(cuda, df), bits)
        torch.cuda.synchronize()
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        lev = sc.unpack(want, bits)
        assert lev.min() == 0 and lev.max() == (1 << bits) - 1 and (lev[:, 5] == 0).all() == (df[5] == 0)


@pytest.mark.parametrize("residual", [False, True])
def test_range_equals_numpy_bit_for_bit(cuda, residual):
    docs, _, cent, list_of = _corpus()
    cent_, list_ = (cent, list_of) if residual else (None, None)
    want = sc.train_range(docs, list_, cent_)
    for chunk in (1 << 18, 700):                      # one chunk, and five with a ragged last one
        got = sq.train_range(_dev(cuda, docs), None if list_ is None else _dev(cuda, list_.astype(np.int32)), _dev(cuda, cent_), chunk=chunk)
        assert np.array_equal(_bits(got[0]), want[0].view(np.uint32)) and np.array_equal(_bits(got[1]), want[1].view(np.uint32))


@functools.lru_cache(maxsize=None)
def _flat_reference(bits, k):
    docs, q, _, _ = _corpus()
    vmin, vdiff = sc.train_range(docs)
    codes = sc.encode(docs, vmin, vdiff, bits)
    off = np.array([0, ND], np.int64)
    want = sc.sq_expected(q, codes, vmin, vdiff, bits, off, None, np.zeros((NQ, 1), np.int32), None, k)
    return vmin, vdiff, codes, want


def _same(got, want):
    np.testing.assert_array_equal(np.asarray(got[1].cpu() if torch.is_tensor(got[1]) else got[1]), want[1])
    s = got[0].cpu().numpy() if torch.is_tensor(got[0]) else got[0]
    np.testing.assert_array_equal(s.view(np.uint32), want[0].view(np.uint32))


@pytest.mark.parametrize("bits", [8, 4])
def test_flat_index_is_pinned_by_its_corpus(cuda, bits):
    """'SQ8' / 'SQ4': range, codes and search results bit for bit from the reference; nothing is seeded."""
    docs, q, _, _ = _corpus()
    vmin, vdiff, codes, want = _flat_reference(bits, 50)
    index = sq.SQIndex(_dev(cuda, docs), None, bits)
    assert np.array_equal(_bits(index.vmin), vmin.view(np.uint32)) and np.array_equal(_bits(index.vdiff), vdiff.view(np.uint32))
    np.testing.assert_array_equal(index.codes.cpu().numpy(), codes)
    assert index.n_lists == 1 and index.max_list_len == ND and index.offsets.tolist() == [0, ND]
    _same(index.search(_dev(cuda, q), 50), want)
    _same(index.search(_dev(cuda, q), 50, nprobe=7), want)              # nprobe has nothing to choose from


@pytest.mark.parametrize("bits,nprobe", [(8, 1), (8, 3), (4, 3), (4, 20)])
def test_ivf_index_is_pinned_given_its_centroids(cuda, bits, nprobe):
    """Lists (the reference's assignment), range of the residuals, codes list-major and the search (coarse scores as biases)."""
    docs, q, cent, list_of = _corpus()
    index = sq.SQIndex(_dev(cuda, docs), NLIST, bits, centroids=_dev(cuda, cent))
    np.testing.assert_array_equal(index.list_of.cpu().numpy(), list_of)
    ids = np.argsort(list_of, kind="stable").astype(np.int64)
    off = np.concatenate([[0], np.cumsum(np.bincount(list_of, minlength=NLIST))]).astype(np.int64)
    np.testing.assert_array_equal(index.ids.cpu().numpy(), ids)
    assert index.offsets.tolist() == off.tolist() and index.max_list_len == int(np.diff(off).max())
    vmin, vdiff = sc.train_range(docs, list_of, cent)
    assert np.array_equal(_bits(index.vmin), vmin.view(np.uint32)) and np.array_equal(_bits(index.vdiff), vdiff.view(np.uint32))
    codes = sc.encode(docs, vmin, vdiff, bits, list_of, cent, ids)
    np.testing.assert_array_equal(index.codes.cpu().numpy(), codes)
    p = min(nprobe, NLIST)
    bias, lists = odense.ip_topk_exact(q, cent, p)
    want = sc.sq_expected(q, codes, vmin, vdiff, bits, off, ids, lists.astype(np.int32), bias, 50)
    _same(index.search(_dev(cuda, q), 50, nprobe), want)


def test_dense_search_routes_sq_strings_to_the_index(cuda, monkeypatch, capsys):
    """dense.search(..., 'SQ8') returns the flat index's lists -- the reference's, which differ from the exact search's because
    quantisation moves ranks on this corpus (asserted on the CPU) --, 'IVF8,SQ4' the lists of the index built from the same seed;
    MEVI_SQ=exact, 'SQ6' and topk = 5000 return the exact search's lists."""
    docs, q = (np.array(a) for a in _corpus()[:2])             # writable copies: dense.search wraps them as tensors
    monkeypatch.delenv("MEVI_SQ", raising=False)
    monkeypatch.delenv("MEVI_IVF_NPROBE", raising=False)
    k = 50
    exact = odense.ip_topk_exact(q, docs, k)
    _, _, _, want = _flat_reference(8, k)
    assert not np.array_equal(want[1], exact[1]) and (want[1] != exact[1]).any(1).sum() >= 3      # SQ8 does move ranks here
    got = dense.search(q, docs, DIM, k, "SQ8")
    _same(got, want)
    assert "Param SQ8 trained: False." in capsys.readouterr().out
    flat = dense.search(q, docs, DIM, k, "Flat")
    np.testing.assert_array_equal(flat[1], exact[1])
    got4 = dense.search(q, docs, DIM, k, "IVF8,SQ4")
    index = sq.SQIndex(_dev(cuda, docs), 8, 4)
    s, i = index.search(_dev(cuda, q), k, 1)
    np.testing.assert_array_equal(got4[1], i.cpu().numpy())
    np.testing.assert_array_equal(got4[0].view(np.uint32), _bits(s))
    assert not np.array_equal(got4[1], flat[1]) and (got4[1] >= 0).all()
    # the strings and shapes that keep the exact search
    for param, topk, env in (("SQ6", k, None), ("SQ8", k, "exact"), ("IVF8,SQ4", k, "exact")):
        if env:
            monkeypatch.setenv("MEVI_SQ", env)
        out = dense.search(q, docs, DIM, topk, param)
        monkeypatch.delenv("MEVI_SQ", raising=False)
        np.testing.assert_array_equal(out[1], flat[1])
        np.testing.assert_array_equal(out[0].view(np.uint32), flat[0].view(np.uint32))
    big = dense.search(q[:2], np.concatenate([docs, docs]), DIM, 5000, "SQ8")
    ref = dense.search(q[:2], np.concatenate([docs, docs]), DIM, 5000, "Flat")
    np.testing.assert_array_equal(big[1], ref[1])
    np.testing.assert_array_equal(big[0].view(np.uint32), ref[0].view(np.uint32))


@pytest.mark.parametrize("param", ["IVF8,SQ8", "SQ4"])
def test_dense_profile_times_train_and_add_of_an_sq_string(cuda, monkeypatch, param):
    docs, q = (np.array(a) for a in _corpus()[:2])
    monkeypatch.delenv("MEVI_SQ", raising=False)
    t = dense.profile(q, docs, DIM, 10, param, bs=[1, 4])
    assert set(t) == {"train", "add", "search_bs1", "search_bs4"}
    assert t["train"] > 0 and t["add"] > 0 and t["search_bs1"] > 0 and t["search_bs4"] > 0
