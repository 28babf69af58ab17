"""Host side of the residual quantiser's beam-search encoder (include/mevi_hip_rq_errbeam.h, mevi_amd/rqindex.py) without a GPU: the
header and its bindings, the workspace and tile queries (pure arithmetic, positive inside the envelope, 0 just outside every
bound), every documented refusal with its status and a message naming the argument before anything is launched (the pointers
handed over are null or fake, for n = 0 too), the environment variables, and the reference of the GPU tests
(tests/rq_errbeam_cases.py): a beam of one is the greedy encoder, the walk agrees with float64 where nothing is near a tie, and the
quality condition of the GPU test holds for the reference alone."""
import os
import re

import numpy as np
import pytest

import aq_cases as ac
import rq_errbeam_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
A, A2 = 1 << 20, 1 << 30                           # fake, well-aligned, far apart device addresses: nothing may dereference them
STEP = ("mevi_rq_errbeam_step_workspace_bytes", "mevi_rq_errbeam_step_tile_docs", "mevi_rq_errbeam_step_f32")

# (dim, K, B, L) outside the envelope, and the word the refusal names it with
OUTSIDE = [((64, 0, 5, 5), "K=0"), ((64, 257, 5, 5), "K=257"), ((64, 16, 0, 5), "B=0"), ((64, 16, 17, 5), "B=17"),
           ((64, 16, 5, 0), "L=0"), ((64, 16, 5, 17), "L=17"), ((66, 16, 5, 5), "dim=66"), ((0, 16, 5, 5), "dim=0"),
           ((4100, 16, 5, 5), "dim=4100"), ((-4, 16, 5, 5), "dim=-4")]
INSIDE = [(4, 1, 1, 1), (4096, 256, 16, 16), (768, 256, 5, 5), (768, 256, 1, 5), (36, 16, 5, 5), (100, 33, 2, 16), (64, 2, 2, 5),
          (64, 128, 16, 1), (64, 129, 16, 1)]


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def test_header_is_included_exported_and_bound(L):
    from mevi_amd import dense, hip, rqindex

    assert '#include "mevi_hip_rq_errbeam.h"' in open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    raw = open(os.path.join(ROOT, "include", "mevi_hip_rq_errbeam.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mevi_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(STEP + ("mevi_rq_errbeam_codes_u8",))
    assert hip.exported_symbols("mevi_hip_rq_errbeam.h") == declared and declared == sorted(hip._RQ_ERRBEAM_SIGNATURES)
    for other in ("mevi_hip.h", "mevi_hip_aq.h", "mevi_hip_refine.h", "mevi_hip_ivfpq.h", "mevi_hip_opq_encode.h"):
        assert not set(declared) & set(hip.exported_symbols(other)), other
    assert all(callable(getattr(L, n)) for n in declared)
    for name in declared:                          # argument counts of the declarations = those of the signature table
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text, flags=re.S).group(1)
        assert len([a for a in args.split(",") if a.strip()]) == len(hip._RQ_ERRBEAM_SIGNATURES[name][1]), name
    for name in ("rq_errbeam_step", "rq_errbeam_codes", "rq_errbeam_step_workspace_bytes", "rq_errbeam_step_tile_docs"):
        assert callable(getattr(dense, name))
    for name in ("encode_walk", "beam_step", "beam_step_composed", "train_codebook_beam"):
        assert callable(getattr(rqindex, name))
    assert "getenv" not in open(os.path.join(ROOT, "mevi_amd", "csrc", "rq_errbeam.hip")).read()   # the C ABI reads no environment


def test_queries_are_host_arithmetic_and_zero_just_outside_every_bound(L):
    ws, tile = L.mevi_rq_errbeam_step_workspace_bytes, L.mevi_rq_errbeam_step_tile_docs
    for shape, _ in OUTSIDE:
        assert ws(1000, *shape) == 0 and tile(*shape) == 0, shape
    for shape in INSIDE:
        dim, K, B, Lb = shape
        assert ws(1000, *shape) > 0 and ws(0, *shape) > 0, shape
        assert ws(-1, *shape) == 0, shape
        most = ((1 << 31) - 1) // B                                      # n * B < 2^31
        assert ws(most, *shape) > 0 and ws(most + 1, *shape) == 0, shape
        assert ws(1, *shape) == ws(most, *shape) <= 1 << 20, shape       # the ticket of a persistent grid: independent of n
        assert tile(*shape) == (128 if K <= 128 else 64) // B, shape     # the rows of one distance pass, whole documents
    assert tile(768, 256, 5, 5) == 12 and tile(768, 256, 16, 16) == 4 and tile(768, 32, 5, 5) == 25 and tile(768, 256, 1, 5) == 64


def _step(L, x=A, n=300, B=5, dim=64, cent=A, K=16, Lb=5, parent=A, code=A, err=A, out=A2, ws=A, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = L.mevi_rq_errbeam_step_workspace_bytes(300, 64, 16, 5, 5)
    return L.mevi_rq_errbeam_step_f32(x, n, B, dim, cent, K, Lb, parent, code, err, out, ws, ws_bytes, None)


def _refused(L, status, *words, **kw):
    from mevi_amd import hip

    st = _step(L, **kw)
    msg = L.mevi_last_error().decode()
    assert st == status and msg.startswith("rq_errbeam_step:") and all(w in msg for w in words), (kw, st, msg, words)
    with pytest.raises(hip.MeviHipError, match="rq_errbeam_step"):
        hip.check(st, "mevi_rq_errbeam_step_f32")


@pytest.mark.parametrize("n", [300, 0])
def test_step_refusals_come_before_any_launch(L, n):
    _refused(L, INVALID, "n=-1", n=-1)
    if n:
        _refused(L, UNSUPPORTED, "n=2147483648", n=1 << 31)
        _refused(L, UNSUPPORTED, "31 bits", n=(1 << 31) // 5 + 1)
    for (dim, K, B, Lb), word in OUTSIDE:
        _refused(L, UNSUPPORTED, word, n=n, dim=dim, K=K, B=B, Lb=Lb)
    for name, word in (("x", "null res_in"), ("cent", "null centroids"), ("parent", "null parent"), ("code", "null code"),
                       ("ws", "null workspace")):
        _refused(L, INVALID, word, n=n, **{name: None})
    for name, word in (("x", "res_in must be 16-byte aligned"), ("cent", "centroids must be 16-byte aligned"),
                       ("out", "res_out must be 16-byte aligned")):
        for step in (4, 8):
            _refused(L, INVALID, word, n=n, **{name: (A2 if name == "out" else A) + step})
    _refused(L, INVALID, "err must be 4-byte aligned", n=n, err=A + 2)
    _refused(L, INVALID, "workspace must be 4-byte aligned", n=n, ws=A + 2)
    if n:                                          # the rows written must not be the rows read
        _refused(L, INVALID, "overlaps", out=A)
        _refused(L, INVALID, "overlaps", out=A + 300 * 5 * 64 * 4 - 16)
        assert _step(L, n=0, out=A + 300 * 5 * 64 * 4) == 0             # ... the next byte after them is fine (no launch: n = 0)
    need = L.mevi_rq_errbeam_step_workspace_bytes(300, 64, 16, 5, 5)
    _refused(L, WORKSPACE, "workspace", str(need), n=n, ws_bytes=need - 1)
    _refused(L, WORKSPACE, "workspace", str(need), n=n, ws_bytes=0)


def test_the_workspace_check_is_the_last_one_and_what_is_optional(L):
    for kw, code in (({"Lb": 17}, UNSUPPORTED), ({"dim": 66}, UNSUPPORTED), ({"x": None}, INVALID), ({"cent": A + 4}, INVALID),
                     ({"parent": None}, INVALID), ({"ws": None}, INVALID)):
        assert _step(L, ws_bytes=0, **kw) == code, kw
        assert _step(L, n=0, ws_bytes=0, **kw) == code, kw
    # the order of the envelope's refusals: K, B, L, dim
    for kw, word in (({"K": 0, "B": 0, "Lb": 0, "dim": 0}, "K=0"), ({"B": 0, "Lb": 0, "dim": 0}, "B=0"), ({"Lb": 0, "dim": 0}, "L=0")):
        assert _step(L, **kw) == UNSUPPORTED and word in L.mevi_last_error().decode(), kw
    assert _step(L, n=0) == 0 and _step(L, n=0, err=None) == 0 and _step(L, n=0, out=None) == 0


def test_backtrack_refusals_come_before_any_launch(L):
    def codes(parent=A, code=A, M=8, n=10, stride=5, out=A, cstride=8):
        return L.mevi_rq_errbeam_codes_u8(parent, code, M, n, stride, out, cstride, None), L.mevi_last_error().decode()

    for n in (10, 0):
        for kw, status, word in (({"M": 0}, INVALID, "M=0"), ({"stride": 0}, INVALID, "row_stride=0"), ({"cstride": 7}, INVALID, "code_stride=7"),
                                 ({"stride": 257}, UNSUPPORTED, "row_stride=257"), ({"M": 65537, "cstride": 65537}, UNSUPPORTED, "M=65537")):
            st, msg = codes(n=n, **kw)
            assert st == status and word in msg and msg.startswith("rq_errbeam_codes:"), (kw, st, msg)
    assert codes(n=-1)[0] == INVALID and codes(n=1 << 31)[0] == UNSUPPORTED
    for name in ("parent", "code", "out"):
        st, msg = codes(**{name: None})
        assert st == INVALID and "null" in msg, name
    assert codes(n=0, parent=None, code=None, out=None)[0] == 0


def test_environment_variables_are_parsed_strictly(monkeypatch):
    from mevi_amd import rqindex

    for name in ("MEVI_RQINDEX_BEAM", "MEVI_RQINDEX_TRAIN_BEAM"):
        monkeypatch.delenv(name, raising=False)
        assert rqindex.env_beam(name) == 1
        for text, want in (("1", 1), ("5", 5), ("16", 16), (" 7 ", 7)):
            monkeypatch.setenv(name, text)
            assert rqindex.env_beam(name) == want
        for text in ("0", "17", "x", "", "5.0", "-1"):
            monkeypatch.setenv(name, text)
            with pytest.raises(ValueError, match=name):
                rqindex.env_beam(name)
        monkeypatch.delenv(name)
    for beam in (0, 17, "5", 2.0, True):
        with pytest.raises(ValueError, match="beam"):
            rqindex.check_beam(beam)
    monkeypatch.setenv("MEVI_RQINDEX_BEAM_STEP", "both")
    with pytest.raises(ValueError, match="MEVI_RQINDEX_BEAM_STEP"):
        rqindex.beam_step_is_fused(10, 64, 16, 5, 5)
    monkeypatch.setenv("MEVI_RQINDEX_BEAM_STEP", "steps")
    assert not rqindex.beam_step_is_fused(10, 64, 16, 5, 5)
    monkeypatch.delenv("MEVI_RQINDEX_BEAM_STEP")
    assert rqindex.beam_step_is_fused(10, 64, 16, 5, 5) and rqindex.beam_step_is_fused(10, 4096, 256, 16, 16)
    assert not rqindex.beam_step_is_fused(10, 4100, 16, 5, 5)           # outside the call's envelope: the composition


def test_docstrings_state_what_is_built():
    from mevi_amd import rqindex

    doc = re.sub(r"\s+", " ", rqindex.__doc__)
    for word in ("MEVI_RQINDEX_BEAM", "MEVI_RQINDEX_TRAIN_BEAM", "MEVI_RQINDEX_BEAM_STEP=steps", "max_beam_size", "reconstruction error"):
        assert word in doc, word
    assert "beam encoding" not in doc.split("Not built:")[1]


def test_a_beam_of_one_is_the_greedy_encoder():
    """walk_expected(L = 1) = aq_cases.chained_encode, with duplicate centroids (the lowest index wins in both)."""
    rng = np.random.default_rng(31)
    for dim, M, K, n in ((36, 12, 16, 300), (32, 9, 7, 150), (4, 3, 1, 20), (64, 4, 256, 100)):
        x = rng.standard_normal((n, dim)).astype(np.float32)
        book = (rng.standard_normal((M, K, dim)) * (0.7 ** np.arange(M))[:, None, None]).astype(np.float32)
        book[:, K - 1] = book[:, 0]
        assert np.array_equal(ec.walk_expected(x, book, 1), ac.chained_encode(x, book).astype(np.uint8)), (dim, M, K)


def test_step_expected_is_sorted_tie_broken_and_hands_on_the_right_rows():
    x, cent = ec.random_step(3, 9, 5, 36, 16)
    cent[7] = cent[2]                                  # a duplicated centroid
    x[:, 3] = x[:, 1]                                  # a duplicated beam row
    x[4] = 0.0                                         # all-zero rows: every beam ties
    for Lb in (1, 5, 16):
        parent, code, err, out = ec.step_expected(x, cent, Lb)
        assert parent.shape == code.shape == err.shape == (9, Lb) and out.shape == (9, Lb, 36)
        flat = parent.astype(np.int64) * 16 + code
        assert (np.diff(err, axis=1) >= 0).all() and (flat[:, 1:][np.diff(err, axis=1) == 0] > flat[:, :-1][np.diff(err, axis=1) == 0]).all()
        assert (code != 7).all() or Lb > 1             # the twin is never first
        for i in range(9):
            for l in range(Lb):
                assert np.array_equal(out[i, l], x[i, parent[i, l]] - cent[code[i, l]])
    parent, code, err, _ = ec.step_expected(x, cent, 16)
    assert (parent[4, :5] == np.arange(5)).all() and (code[4, :5] == code[4, 0]).all()     # zero rows: beams in order
    # Lo == B * K and L > B * K: everything kept, sorted
    x2, c2 = ec.random_step(4, 6, 2, 8, 2)
    for Lb in (4, 5, 16):
        parent, code, err, out = ec.step_expected(x2, c2, Lb)
        assert err.shape == (6, 4) and (np.diff(err, axis=1) >= 0).all()
        assert (np.sort(parent.astype(int) * 2 + code, axis=1) == np.arange(4)).all()


def test_codes_expected_follows_the_parents():
    parent, code = ec.random_trace(8, 9, 40, 5, 7)
    got = ec.codes_expected(parent, code)
    for i in range(40):
        p = 0
        for j in range(8, -1, -1):
            assert got[i, j] == code[j, i, p]
            p = parent[j, i, p]
    one = ec.codes_expected(parent[:1], code[:1])
    assert np.array_equal(one[:, 0], code[0, :, 0])


def test_walk_expected_agrees_with_float64_where_nothing_is_near_a_tie():
    rng = np.random.default_rng(13)                    # (an input chosen for its gaps: ten times the bound below)
    x = rng.standard_normal((40, 16)).astype(np.float32)
    book = (rng.standard_normal((6, 8, 16)) * (0.6 ** np.arange(6))[:, None, None]).astype(np.float32)
    for Lb in (1, 3, 5):
        want, gap = ec.walk_float64(x, book, Lb)
        # every term of an error is positive, so roundings count relatively: 16 fmas and a subtraction per element in the chain, and
        # one rounded subtraction per element and earlier level in the row -- (17 + 2 * 6) * 2^-24 on either side of a comparison
        assert gap > 2 * (17 + 2 * 6) * 2.0 ** -24, gap
        assert np.array_equal(ec.walk_expected(x, book, Lb), want), Lb


def test_quality_condition_holds_for_the_reference_alone(capsys):
    """The condition of tests/test_rqindex_beam_gpu.py on the CPU: on the seeded anisotropic corpus, over a greedy-trained codebook, the
    float64 mean reconstruction error of the beam-5 codes is strictly below that of the greedy codes.  (No per-row claim.)"""
    x, book = ec.aniso_corpus()
    greedy = ec.recon_error64(x, book, ec.walk_expected(x, book, 1))
    beam = ec.recon_error64(x, book, ec.walk_expected(x, book, 5))
    with capsys.disabled():
        print(f"\nbeam-5 / greedy mean squared error on the anisotropic corpus: {beam.mean() / greedy.mean():.4f}; "
              f"rows worse under the beam: {(beam > greedy).mean():.3f}")
    assert beam.mean() < greedy.mean()
