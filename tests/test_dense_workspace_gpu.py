"""The dense search's three entry points through the raw C ABI, inside a workspace of EXACTLY the bytes their `*_workspace_bytes`
functions name, with 4096 guard bytes on either side: every path that carves its own part of the workspace (guaranteed exact
repair, second f16 pass, exact fallback of the indexed search, the candidate counters of profiling level 2, the 8-bit pass and
its repeat through the f16 image) must stay inside it, return `dense.ip_topk`'s lists bit for bit, and refuse one byte less
before anything is launched.  The constructions are the smallest ones of tests/test_dense_gpu.py that force each path; the
statistics prove the path ran."""
import functools

import numpy as np
import pytest
import torch

from mevi_amd import dense, hip

GUARD = 4096
FILL = 0xA5
ERR_WORKSPACE = -3   # MEVI_ERR_WORKSPACE (include/mevi_hip.h)


def _stats():
    st = hip.IpTopkStats()
    hip.lib().mevi_ip_topk_get_stats(st)
    return st


@functools.lru_cache(maxsize=None)
def _case(name):
    """(queries, rows, k) as numpy arrays; seeds and recipes of tests/test_dense_gpu.py."""
    if name == "sorted rows":          # rows in ascending order of the score along one direction: every chunk floods the lists
        rng = np.random.default_rng(9)
        dim, nd = 32, 60000
        direction = rng.standard_normal(dim).astype(np.float32)
        scale = np.linspace(-1.0, 1.0, nd, dtype=np.float32)[:, None]
        d = scale * direction[None, :] + 1e-3 * rng.standard_normal((nd, dim)).astype(np.float32)
        q = np.stack([direction * (1 + 0.1 * j) for j in range(6)]).astype(np.float32)
        return np.concatenate([q, rng.standard_normal((10, dim)).astype(np.float32)]), d, 50
    if name == "250 near-copies":      # more than the first pass's survivors, fewer than the second's: proven by the second pass
        rng = np.random.default_rng(61)
        base = rng.standard_normal((1, 64), dtype=np.float32)
        d = np.concatenate([base + 1e-6 * rng.standard_normal((250, 64)).astype(np.float32), rng.standard_normal((8000, 64), dtype=np.float32)])
        d = d[rng.permutation(len(d))]
        return np.concatenate([base * 2, rng.standard_normal((7, 64), dtype=np.float32)]), d, 50
    if name == "5000 near-copies":     # more than either pass keeps: the exact fallback
        rng = np.random.default_rng(31)
        base = rng.standard_normal((1, 64), dtype=np.float32)
        d = np.concatenate([base + 1e-6 * rng.standard_normal((5000, 64)).astype(np.float32), rng.standard_normal((3000, 64), dtype=np.float32)])
        return np.concatenate([base * 2, rng.standard_normal((7, 64), dtype=np.float32)]), d, 50
    rng = np.random.default_rng(12)
    q = rng.standard_normal((9, 768), dtype=np.float32)
    d = rng.standard_normal((40000, 768), dtype=np.float32)
    if name == "50 distinct rows":     # every score 800 times: no survivor list of the 8-bit pass separates rank k from the rest
        d = d[:50][rng.integers(0, 50, len(d))].copy()
    else:
        assert name == "random rows"
    return q, d, 20


_REFERENCE = {}


def _reference(name, q, docs, k):
    """`dense.ip_topk` of a case's inputs, computed once (scores as int32 bits, ids)."""
    if name not in _REFERENCE:
        s, i = dense.ip_topk(q, docs, k)
        _REFERENCE[name] = (s.view(torch.int32).cpu(), i.cpu())
    return _REFERENCE[name]


def _index(docs):
    L = hip.lib()
    nd, dim = docs.shape
    index = torch.empty(L.mevi_ip_index_bytes(nd, dim), dtype=torch.uint8, device=docs.device)
    assert L.mevi_ip_index_build_f32(hip.ptr(docs), nd, dim, hip.ptr(index), index.numel(), hip.stream_ptr()) == 0
    return index


def _index8(docs, index):
    L = hip.lib()
    nd, dim = docs.shape
    index8 = torch.empty(L.mevi_ip_index8_bytes(nd, dim), dtype=torch.uint8, device=docs.device)
    assert L.mevi_ip_index8_build_f32(hip.ptr(docs), hip.ptr(index), nd, dim, hip.ptr(index8), index8.numel(), hip.stream_ptr()) == 0
    return index8


def _search_in_guarded_workspace(entry, name, cuda):
    """One search of `name`'s inputs through `entry` in a guarded workspace of exactly the required bytes; returns its statistics
    after checking the guards, the lists and the refusal of one byte less."""
    L = hip.lib()
    qn, dn, k = _case(name)
    q, docs = torch.from_numpy(qn).to(cuda), torch.from_numpy(dn).to(cuda)
    nq, dim = q.shape
    nd = docs.shape[0]
    if entry == "exact":
        need = L.mevi_ip_topk_workspace_bytes(nq, dim, k)

        def call(ws, nbytes, s, i):
            return L.mevi_ip_topk_f32(hip.ptr(q), nq, hip.ptr(docs), nd, dim, k, 0, hip.ptr(s), hip.ptr(i), ws, nbytes, hip.stream_ptr())
    elif entry == "indexed":
        need = L.mevi_ip_topk_indexed_workspace_bytes(nq, dim, k)
        index = _index(docs)

        def call(ws, nbytes, s, i):
            return L.mevi_ip_topk_indexed_f32(hip.ptr(q), nq, hip.ptr(docs), hip.ptr(index), nd, dim, k, 0, hip.ptr(s), hip.ptr(i), ws,
                                              nbytes, hip.stream_ptr())
    else:
        need = L.mevi_ip_topk_indexed8_workspace_bytes(nq, dim, k)
        index = _index(docs)
        index8 = _index8(docs, index)

        def call(ws, nbytes, s, i):
            return L.mevi_ip_topk_indexed8_f32(hip.ptr(q), nq, hip.ptr(docs), hip.ptr(index), hip.ptr(index8), nd, dim, k, 0, hip.ptr(s),
                                               hip.ptr(i), ws, nbytes, hip.stream_ptr())
    assert need > 0
    buf = torch.full((need + 2 * GUARD,), FILL, dtype=torch.uint8, device=cuda)
    ws = buf.data_ptr() + GUARD
    assert ws % 256 == 0

    def guards_intact():
        return bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + need:] == FILL).all())

    # one byte less: refused, and nothing that was launched wrote the outputs (or the workspace's surroundings)
    s = torch.full((nq, k), 7.0, dtype=torch.float32, device=cuda)
    i = torch.full((nq, k), -7, dtype=torch.int64, device=cuda)
    assert call(ws, need - 1, s, i) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((s == 7.0).all()) and bool((i == -7).all()) and guards_intact()

    assert call(ws, need, s, i) == 0
    st = _stats()
    torch.cuda.synchronize()
    assert guards_intact(), "the search wrote outside its workspace"
    es, ei = _reference(name, q, docs, k)
    assert torch.equal(i.cpu(), ei) and torch.equal(s.view(torch.int32).cpu(), es)
    return st


@pytest.mark.gpu
def test_exact_search_repairs_overflowed_queries_inside_its_workspace(cuda):
    st = _search_in_guarded_workspace("exact", "sorted rows", cuda)
    assert st.n_failed_queries >= 6, st.n_failed_queries


@pytest.mark.gpu
def test_indexed_search_runs_its_second_pass_inside_its_workspace(cuda):
    st = _search_in_guarded_workspace("indexed", "250 near-copies", cuda)
    assert st.n_second_pass_queries >= 1 and st.n_failed_queries == 0, (st.n_second_pass_queries, st.n_failed_queries)


@pytest.mark.gpu
def test_indexed_search_falls_back_to_the_exact_pass_inside_its_workspace(cuda):
    st = _search_in_guarded_workspace("indexed", "5000 near-copies", cuda)
    assert st.n_failed_queries >= 1, st.n_failed_queries


@pytest.mark.gpu
def test_candidate_counters_of_profiling_level_two_lie_inside_the_workspace(cuda):
    L = hip.lib()
    L.mevi_ip_topk_set_profiling(2)
    try:
        st = _search_in_guarded_workspace("indexed", "250 near-copies", cuda)
    finally:
        L.mevi_ip_topk_set_profiling(0)
    assert st.n_filter_candidates > 0 and st.n_second_pass_queries >= 1, (st.n_filter_candidates, st.n_second_pass_queries)


@pytest.mark.gpu
def test_8_bit_pass_and_its_repeat_through_the_f16_image_stay_inside_the_workspace(cuda):
    st = _search_in_guarded_workspace("indexed8", "50 distinct rows", cuda)
    assert st.n_i8_queries == 9 and st.n_i8_unproven > 0, (st.n_i8_queries, st.n_i8_unproven)
    st = _search_in_guarded_workspace("indexed8", "random rows", cuda)
    assert st.n_i8_queries == 9 and st.n_i8_unproven == 0, (st.n_i8_queries, st.n_i8_unproven)
