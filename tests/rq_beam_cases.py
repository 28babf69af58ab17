"""Cases and the two call paths of the fused beam encode tests (test helper, no tests here).

* `composition`  -- pq.beam_search as the per-level composition on the C ABI, through ctypes with a RAW codebook (any K, not
                    only 2**bits): mevi_rq_neg_dist_f32, then mevi_beam_step_f32(final_step = 2) or mevi_row_softmax_f32
                    (mode 1), the label gather, mevi_gather_sub_f32 -- what rq.ProductQuantization._beam_search_steps does.
* `fused`        -- mevi_rq_beam_encode_f32 with a fresh workspace, optional guard bands around labels / proba.
* `CASES`        -- (shape, R, pq): every (shape, R <= 16) of index_build_ref.BEAM_CASES / PQ_BEAM_CASES plus ADDED, the shapes
                    those lists do not reach.  Inputs: `inputs(shape, pq)` = index_build_ref.beam_case_inputs, with the
                    level ratio of ADDED_RATIO where the default leaves the reference alone too few decidable positions
                    (tests/test_rq_beam_encode_cpu.py holds that condition on the CPU).
"""
import functools

import numpy as np

import index_build_ref as ib

MAX_R = 16

# (n, dim, M, K), R, pq
ADDED = [
    ((257, 100, 3, 100), 5, False),     # K no power of two and no multiple of 32, dim no multiple of the 32-wide k slab
    ((64, 4, 2, 3), 9, False),          # the smallest dim; R = K^M: keep-all to the end
    ((33, 768, 4, 32), 3, False),       # the production shapes
    ((33, 768, 3, 256), 3, False),
    ((65, 768, 4, 32), 3, True),
    ((40, 64, 8, 8), 16, True),         # dsub = 8
]
ADDED_RATIO = {}

CASES = [(s, R, False) for s, Rs in ib.BEAM_CASES.items() for R in Rs if R <= MAX_R] + \
        [(s, R, True) for s, Rs in ib.PQ_BEAM_CASES.items() for R in Rs if R <= MAX_R] + ADDED


def case_id(case):
    shape, R, pq = case
    return f"{'pq' if pq else 'rq'}-{'x'.join(map(str, shape))}-R{R}"


@functools.lru_cache(maxsize=None)
def inputs(shape, pq=False):
    """(x f32 [n, dim], codebook) of a case, computed once; callers do not write to them."""
    if (shape, pq) in ADDED_RATIO:
        n, dim, M, K = shape
        return ib.clustered_inputs(n, dim, M, K, 1000 + sum(shape), pq=pq, ratio=ADDED_RATIO[(shape, pq)])
    return ib.beam_case_inputs(shape, pq)


@functools.lru_cache(maxsize=None)
def reference(shape, R, pq):
    """(labels, scores, cut gap) of the float64-softmax chain reference, computed once per case."""
    x, cb = inputs(shape, pq)
    chain = ib.pq_beam_search_chain if pq else ib.rq_beam_search_chain
    return chain(x, cb, R, return_cut_gap=True)


def tie_inputs(n=96, dim=32, M=3, K=16, seed=5):
    """Duplicated centroids (code c and c + K / 2 are the same vector at every level) and duplicated rows: every candidate
    score occurs at least twice per row, so each top-R step and each kept list is decided by beam * K + code alone."""
    rng = np.random.default_rng(seed)
    s = dim ** -0.5
    half = (rng.standard_normal((M, K // 2, dim)) * 2 * s).astype(np.float32)
    cb = np.concatenate([half, half], 1) / (2.0 ** np.arange(M, dtype=np.float32))[:, None, None]
    pick = rng.integers(0, K, size=(n // 2, M))
    x = sum(cb[j][pick[:, j]] for j in range(M)) + 0.5 * s * 0.25 * rng.standard_normal((n // 2, dim))
    x = np.concatenate([x, x]).astype(np.float32)
    return x, np.ascontiguousarray(cb, dtype=np.float32)


def _lib():
    from mevi_amd import hip

    return hip, hip.lib()


def composition(x, cb, R, pq):
    """(labels i32 [n, R', M], proba f32 [n, R']) of CUDA tensors x f32 [n, dim], cb f32 [M, K, dim or dsub]."""
    import torch

    hip, L = _lib()
    dev = x.device
    M, K, d = cb.shape
    n = x.shape[0]
    s = hip.stream_ptr()
    resid, nb = x, 1
    scores = torch.ones((n, 1), dtype=torch.float32, device=dev)
    labels = torch.zeros((n, 1, 0), dtype=torch.int32, device=dev)
    base = torch.arange(n, device=dev)[:, None]
    for j in range(M):
        rows = x[:, j * d:(j + 1) * d].contiguous() if pq else resid
        level = cb[j].contiguous()
        nd = torch.empty((rows.shape[0], K), dtype=torch.float32, device=dev)
        hip.check(L.mevi_rq_neg_dist_f32(hip.ptr(rows), rows.shape[0], d, hip.ptr(level), K, hip.ptr(nd), s), "mevi_rq_neg_dist_f32")
        if pq and nb > 1:
            nd = nd[:, None, :].expand(n, nb, K).reshape(n * nb, K).contiguous()
        if R < nb * K:
            sc = torch.empty((n, R), dtype=torch.float32, device=dev)
            parent = torch.empty((n, R), dtype=torch.int32, device=dev)
            code = torch.empty((n, R), dtype=torch.int32, device=dev)
            hip.check(L.mevi_beam_step_f32(hip.ptr(nd), hip.ptr(scores), n, nb, K, R, 2, hip.ptr(sc), hip.ptr(parent), hip.ptr(code), s),
                      "mevi_beam_step_f32")
            nbn = R
        else:
            sc = torch.empty((n * nb, K), dtype=torch.float32, device=dev)
            flat = scores.reshape(-1).contiguous()
            hip.check(L.mevi_row_softmax_f32(hip.ptr(nd), n * nb, K, 1, hip.ptr(flat), hip.ptr(sc), s), "mevi_row_softmax_f32")
            sc = sc.reshape(n, nb * K)
            parent = torch.arange(nb, device=dev, dtype=torch.int32).repeat_interleave(K)[None].expand(n, -1).contiguous()
            code = torch.arange(K, device=dev, dtype=torch.int32).repeat(nb)[None].expand(n, -1).contiguous()
            nbn = nb * K
        labels = torch.cat([torch.gather(labels, 1, parent.long()[:, :, None].expand(-1, -1, labels.shape[2])), code[:, :, None]], dim=2)
        if j != M - 1 and not pq:
            src = (base * nb + parent.long()).reshape(-1).contiguous()
            nxt = torch.empty((n * nbn, d), dtype=torch.float32, device=dev)
            hip.check(L.mevi_gather_sub_f32(hip.ptr(resid), hip.ptr(src), hip.ptr(level), hip.ptr(code.reshape(-1).contiguous()),
                                            n * nbn, d, hip.ptr(nxt), s), "mevi_gather_sub_f32")
            resid = nxt
        scores, nb = sc, nbn
    return labels, scores


SENTINEL_I, SENTINEL_F = -0x5A5A5A5B, -12345.0


def fused(x, cb, R, pq, want_proba=True, guard=0):
    """(labels i32 [n, R, M], proba f32 [n, R] or None) of mevi_rq_beam_encode_f32.  guard > 0: both outputs sit between
    `guard` sentinel elements on either side and the call returns (labels, proba, guards_intact)."""
    import torch

    hip, L = _lib()
    dev = x.device
    M, K, d = cb.shape
    n, dim = x.shape
    nbytes = L.mevi_rq_beam_encode_workspace_bytes(n, dim, M, K, R, int(pq))
    assert nbytes > 0, (x.shape, cb.shape, R, pq)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    # (one element more than asked for: an address to hand over even when n = 0)
    lab_buf = torch.full((n * R * M + 2 * guard + 1,), SENTINEL_I, dtype=torch.int32, device=dev)
    pr_buf = torch.full((n * R + 2 * guard + 1,), SENTINEL_F, dtype=torch.float32, device=dev)
    lab = lab_buf[guard:guard + n * R * M]
    pr = pr_buf[guard:guard + n * R]
    st = L.mevi_rq_beam_encode_f32(hip.ptr(x) if n else hip.ptr(cb), n, dim, hip.ptr(cb), M, K, R, int(pq), lab_buf.data_ptr() + 4 * guard,
                                   pr_buf.data_ptr() + 4 * guard if want_proba else None, hip.ptr(ws), nbytes, hip.stream_ptr())
    hip.check(st, "mevi_rq_beam_encode_f32")
    out = (lab.reshape(n, R, M), pr.reshape(n, R) if want_proba else None)
    if not guard:
        return out
    intact = bool((lab_buf[:guard] == SENTINEL_I).all() and (lab_buf[guard + n * R * M:] == SENTINEL_I).all() and
                  (pr_buf[:guard] == SENTINEL_F).all() and (pr_buf[guard + n * R:] == SENTINEL_F).all())
    if not want_proba:
        intact = intact and bool((pr_buf == SENTINEL_F).all())
    return out + (intact,)


def same_bits(a, b):
    import torch

    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))
