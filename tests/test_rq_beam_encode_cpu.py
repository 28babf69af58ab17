"""Host side of the fused beam encode (mevi_rq_beam_encode_workspace_bytes / _tile_docs / mevi_rq_beam_encode_f32): the
symbols exist and are bound, both queries are pure arithmetic, positive inside the envelope and 0 exactly outside, the
workspace does not grow with n, every documented refusal comes back with its code and a message that names the argument
before anything is launched (the pointers handed over are null or fake, so a launch would not go unnoticed) -- for n = 0
too -- and the inputs of the added GPU cases leave the reference alone enough decidable positions."""
import os
import re

import pytest

import index_build_ref as ib
import rq_beam_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
A = 1 << 20                                        # a fake, well-aligned device address: nothing may dereference it
NAMES = ("mevi_rq_beam_encode_workspace_bytes", "mevi_rq_beam_encode_tile_docs", "mevi_rq_beam_encode_f32")

# (dim, M, K, R, pq) outside the envelope, and the word the refusal names it with
OUTSIDE = [
    ((64, 3, 16, 17, 0), "R=17"), ((64, 3, 16, 0, 0), "R=0"), ((64, 3, 257, 3, 0), "K=257"), ((64, 3, 0, 1, 0), "K=0"),
    ((64, 9, 16, 3, 0), "M=9"), ((64, 0, 16, 1, 0), "M=0"), ((66, 3, 16, 3, 0), "dim=66"), ((4100, 3, 16, 3, 0), "dim=4100"),
    ((0, 3, 16, 3, 0), "dim=0"), ((64, 3, 16, 3, 1), "dim=64"),          # pq: 64 % 3 != 0
    ((24, 4, 16, 3, 1), "dim=24"),                                        # pq: dsub = 6
    ((32, 1, 8, 9, 0), "R=9"), ((32, 2, 3, 10, 0), "R=10"), ((64, 3, 16, 3, 2), "pq=2"),
]
INSIDE = [(768, 4, 32, 3, 0), (768, 3, 256, 3, 0), (768, 4, 32, 10, 0), (768, 4, 32, 3, 1), (40, 5, 16, 3, 1), (4, 1, 1, 1, 0),
          (4096, 8, 256, 16, 0), (32, 1, 8, 8, 0), (4, 2, 3, 9, 0), (100, 3, 100, 5, 0), (64, 8, 8, 16, 1), (32, 8, 2, 16, 0)]


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def test_symbols_are_declared_exported_and_bound(L):
    from mevi_amd import hip, rq

    text = open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in hip.exported_symbols() and callable(getattr(L, name))
    assert callable(rq.ProductQuantization._beam_search_steps) and callable(rq.ProductQuantization._beam_search_fused)


def test_queries_are_zero_exactly_outside_the_envelope(L):
    ws, tile = L.mevi_rq_beam_encode_workspace_bytes, L.mevi_rq_beam_encode_tile_docs
    for shape, _ in OUTSIDE:
        assert ws(1000, *shape) == 0 and tile(*shape) == 0, shape
    for shape in INSIDE:
        assert ws(1000, *shape) > 0 and tile(*shape) > 0, shape
        assert ws(0, *shape) > 0                                           # the refusals hold for n = 0 too
        assert ws(-1, *shape) == 0 and ws(1 << 31, *shape) == 0 and ws((1 << 31) - 1, *shape) > 0
    # R against K^M, at the edge
    assert tile(32, 1, 8, 8, 0) > 0 and tile(32, 1, 8, 9, 0) == 0
    assert tile(32, 2, 4, 16, 0) > 0 and tile(32, 2, 3, 9, 0) > 0 and tile(32, 2, 3, 10, 0) == 0
    assert tile(32, 8, 1, 1, 0) > 0 and tile(32, 8, 1, 2, 0) == 0


def test_tile_docs_follow_the_widest_level(L):
    """A distance pass holds 128 (document, beam) rows (64 above K = 128); a tile is as many whole passes of the widest
    level as fit that many documents, so that level 0 is one pass.  'pq' scores one row per document."""
    tile = L.mevi_rq_beam_encode_tile_docs
    assert tile(768, 4, 32, 1, 0) == 128 and tile(768, 4, 32, 3, 0) == 126 and tile(768, 4, 32, 10, 0) == 120
    assert tile(768, 4, 32, 16, 0) == 128 and tile(768, 3, 256, 3, 0) == 63 and tile(768, 3, 256, 16, 0) == 64
    assert tile(768, 1, 32, 16, 0) == 128                                  # M = 1: one beam enters the only level
    assert tile(768, 4, 32, 3, 1) == 128 and tile(768, 3, 256, 3, 1) == 64


def test_workspace_is_monotone_and_bounded_by_the_grid(L):
    ws = L.mevi_rq_beam_encode_workspace_bytes
    for shape in INSIDE:
        sizes = [ws(n, *shape) for n in (0, 1, 127, 128, 129, 65536, 1 << 20, 1 << 22, 1 << 23, 1 << 30, (1 << 31) - 1)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (shape, sizes)
        assert ws(1 << 22, *shape) == ws(1 << 23, *shape) == ws(1 << 30, *shape) <= 1 << 20, shape


def _call(L, x=A, n=300, dim=64, cb=A, M=3, K=16, R=3, pq=0, labels=A, proba=A, ws=A, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = L.mevi_rq_beam_encode_workspace_bytes(300, 64, 3, 16, 3, 0)
    return L.mevi_rq_beam_encode_f32(x, n, dim, cb, M, K, R, pq, labels, proba, ws, ws_bytes, None)


def _refused(L, code, *words, **kw):
    from mevi_amd import hip

    st = _call(L, **kw)
    msg = L.mevi_last_error().decode()
    assert st == code and msg.startswith("rq_beam_encode:") and all(w in msg for w in words), (kw, st, msg, words)
    with pytest.raises(hip.MeviHipError, match="rq_beam_encode"):
        hip.check(st, "mevi_rq_beam_encode_f32")


@pytest.mark.parametrize("n", [300, 0])
def test_refusals_come_before_any_launch(L, n):
    _refused(L, INVALID, "n=-1", n=-1)
    if n:
        _refused(L, UNSUPPORTED, "n=2147483648", n=1 << 31)
    for (dim, M, K, R, pq), word in OUTSIDE:
        _refused(L, UNSUPPORTED, word, n=n, dim=dim, M=M, K=K, R=R, pq=pq)
    for name, word in (("x", "null x"), ("cb", "null codebook"), ("labels", "null labels"), ("ws", "null workspace")):
        _refused(L, INVALID, word, n=n, **{name: None})
    for name, word in (("x", "x must be 16-byte aligned"), ("cb", "codebook must be 16-byte aligned")):
        for step in (4, 8):
            _refused(L, INVALID, word, n=n, **{name: A + step})
    need = L.mevi_rq_beam_encode_workspace_bytes(300, 64, 3, 16, 3, 0)
    _refused(L, WORKSPACE, "workspace", str(need), n=n, ws_bytes=need - 1)
    _refused(L, WORKSPACE, "workspace", str(need), n=n, ws_bytes=0)


def test_the_workspace_check_is_the_last_one(L):
    """A short workspace together with any other fault reports the other fault."""
    for kw, code in (({"R": 17}, UNSUPPORTED), ({"dim": 66}, UNSUPPORTED), ({"x": None}, INVALID), ({"cb": A + 4}, INVALID),
                     ({"labels": None}, INVALID), ({"ws": None}, INVALID)):
        assert _call(L, ws_bytes=0, **kw) == code, kw
        assert _call(L, n=0, ws_bytes=0, **kw) == code, kw


def test_no_rows_is_no_launch_and_a_null_proba_is_allowed(L):
    assert _call(L, n=0) == 0 and _call(L, n=0, proba=None) == 0


def test_routing_is_chosen_in_python(L, monkeypatch):
    from mevi_amd import rq

    import torch

    def obj(kind, M, bits, dim):
        return rq.ProductQuantization(kind, M, bits, "l2", dim, device=torch.device("cpu"))

    monkeypatch.delenv("MEVI_RQ_BEAM", raising=False)
    assert obj("rq", 4, 5, 768).beam_search_is_fused(3) and obj("rq", 3, 8, 768).beam_search_is_fused(16)
    assert obj("pq", 4, 5, 768).beam_search_is_fused(10)
    assert not obj("rq", 4, 5, 768).beam_search_is_fused(17) and not obj("rq", 4, 5, 768).beam_search_is_fused(40)
    assert not obj("rq", 1, 3, 32).beam_search_is_fused(9) and not obj("pq", 4, 5, 776).beam_search_is_fused(3)   # dsub = 194
    monkeypatch.setenv("MEVI_RQ_BEAM", "steps")
    assert not obj("rq", 4, 5, 768).beam_search_is_fused(3)
    # the library does not look at it: the C ABI has no environment variable
    assert "getenv" not in open(os.path.join(ROOT, "mevi_amd", "csrc", "rq_beam.hip")).read()


def test_the_case_list_reaches_what_it_names():
    cases = set(rc.CASES)
    assert all(R <= rc.MAX_R and R <= shape[3] ** shape[2] for shape, R, _ in cases)
    assert ((130, 768, 4, 32), 10, False) in cases                          # top-R from level 0 on ...
    assert any(K < R < K * K for (_, _, M, K), R, pq in cases if M >= 3)    # ... keep-all at level 0, then top-R
    assert any(R == K and M > 1 for (_, _, M, K), R, pq in cases)           # R == K: kept unsorted, top-R after it
    assert any(M == 1 and R == K for (_, _, M, K), R, pq in cases) and any(M == 8 for (_, _, M, K), R, pq in cases)
    assert any(K == 256 for (_, _, M, K), R, pq in cases) and any(K % 32 and K & (K - 1) for (_, _, M, K), R, pq in cases)
    assert any(dim == 4 and R == K ** M for (_, dim, M, K), R, pq in cases)
    assert any(pq and dim // M == 8 for (_, dim, M, K), R, pq in cases)


@pytest.mark.parametrize("case", rc.ADDED, ids=rc.case_id)
def test_added_inputs_leave_the_reference_decidable(case):
    """A CONDITION on the inputs of the added shapes: at GAP_RTOL the reference alone leaves >= FIRM_SHARE_MIN of the
    positions firm and at most MAX_CUT_EXCLUDED of the rows without a decidable top-R cut (beams_agree_rel asserts it)."""
    shape, R, pq = case
    lab, sc, cut = rc.reference(shape, R, pq)
    ok, share = ib.beams_agree_rel(lab, sc, lab, sc, ib.SCORE_RTOL, ib.GAP_RTOL, cut)
    print(f"{rc.case_id(case)}: firm share {share:.3f}, rows without a decidable cut {(cut <= ib.GAP_RTOL).mean():.3f}")
    assert ok and share >= ib.FIRM_SHARE_MIN, (case, share)


def test_tie_inputs_tie():
    """Every centroid has a twin, every row a twin: the reference's kept lists hold equal scores next to each other."""
    import numpy as np

    x, cb = rc.tie_inputs()
    n, K = len(x), cb.shape[1]
    assert np.array_equal(cb[:, :K // 2], cb[:, K // 2:]) and np.array_equal(x[:n // 2], x[n // 2:])
    lab, sc = ib.rq_beam_search_chain(x, cb, 6)
    assert (sc[:, 0::2] == sc[:, 1::2]).all()                               # pairs of equal scores ...
    assert (lab[:, 0::2, -1] + K // 2 == lab[:, 1::2, -1]).all()            # ... the lower code first
