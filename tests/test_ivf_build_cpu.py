"""Host side of the IVF-Flat build (mevi_ivf_assign_f32, mevi_ivf_build_lists): the symbols exist and are bound, both workspace
queries are pure arithmetic, positive and monotone inside the envelope and 0 outside, every documented refusal comes back
with its code and a message that names the argument before anything is launched (the pointers handed over are null or fake,
so a launch would not go unnoticed), MEVI_IVF_BUILD is read in Python, and the hand-made cases of the GPU tests do what
their names say according to the oracle."""
import glob
import os
import re

import numpy as np
import pytest

import ivf_build_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
A = 1 << 20                                        # a fake, well-aligned device address: nothing may dereference it


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def test_symbols_are_declared_exported_and_bound(L):
    from mevi_amd import dense, hip

    text = open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    for name in ("mevi_ivf_assign_workspace_bytes", "mevi_ivf_assign_f32", "mevi_ivf_build_lists_workspace_bytes", "mevi_ivf_build_lists"):
        assert re.search(r"\b%s\(" % name, text), name
        assert name in hip.exported_symbols() and callable(getattr(L, name))
    assert callable(dense.ivf_assign) and callable(dense.ivf_build_lists)


def test_python_constants_are_the_headers():
    from mevi_amd import dense

    text = open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    for macro, value in (("MEVI_IVF_ASSIGN_ROWS", dense.IVF_ASSIGN_ROWS), ("MEVI_IVF_ASSIGN_COLS", dense.IVF_ASSIGN_COLS),
                         ("MEVI_IVF_ASSIGN_SPLIT_WGS", dense.IVF_ASSIGN_SPLIT_WGS), ("MEVI_IVF_BUILD_MAX_NLIST", dense.IVF_BUILD_MAX_NLIST),
                         ("MEVI_IVF_LISTS_TILE", dense.IVF_LISTS_TILE)):
        assert int(re.search(r"#define %s (\d+)" % macro, text).group(1)) == value, macro
    assert (dense.IVF_ASSIGN_ROWS, dense.IVF_ASSIGN_COLS, dense.IVF_BUILD_MAX_NLIST) == (256, 128, 262144)


def _monotone(f, base_shapes, grids):
    for axis, values in enumerate(grids):
        for other in base_shapes:
            sizes = []
            for v in values:
                shape = list(other)
                shape[axis] = v
                sizes.append(f(*shape))
            assert all(s > 0 for s in sizes), (axis, other, sizes)
            assert sizes == sorted(sizes), (axis, other, sizes)              # never shrinks when an argument grows


def test_assign_workspace_query(L):
    from mevi_amd import dense

    f = L.mevi_ivf_assign_workspace_bytes
    assert f(8841823, 768, 4096) == dense.ivf_assign_workspace_bytes(8841823, 768, 4096) > 0
    edge = dense.IVF_ASSIGN_ROWS * (dense.IVF_ASSIGN_SPLIT_WGS - 1)          # the last n whose centroid walk is split
    _monotone(f, [(8841823, 768, 4096), (1, 4, 1), (3000, 32, 37)],
              [[0, 1, 255, 256, 257, edge, edge + 1, 8841823, (1 << 31) - 1], [4, 28, 32, 36, 64, 768, 1024, 4096],
               [1, 2, 127, 128, 129, 4096, 262144]])
    for shape in [(-1, 64, 8), (1 << 31, 64, 8), (100, 0, 8), (100, 66, 8), (100, 2, 8), (100, 64, 0), (100, 64, -1), (100, 64, 262145)]:
        assert f(*shape) == 0, shape


def test_build_lists_workspace_query(L):
    from mevi_amd import dense

    f = L.mevi_ivf_build_lists_workspace_bytes
    assert f(8841823, 4096) == dense.ivf_build_lists_workspace_bytes(8841823, 4096) >= 16 * 8841823
    T = dense.IVF_LISTS_TILE
    _monotone(f, [(8841823, 4096), (1, 1), (3000, 37)],
              [[0, 1, 2, T - 1, T, T + 1, 65537, 300000, 8841823, (1 << 31) - 1], [1, 2, 100, 1024, 1025, 4096, 262144]])
    for shape in [(-1, 8), (1 << 31, 8), (100, 0), (100, -1), (100, 262145)]:
        assert f(*shape) == 0, shape


def _refused(L, st, code, words, prefix):
    from mevi_amd import hip

    msg = L.mevi_last_error().decode()
    assert st == code and msg.startswith(prefix) and all(w in msg for w in words), (st, msg, words)
    with pytest.raises(hip.MeviHipError, match=prefix[:-1]):
        hip.check(st, prefix)


def test_assign_refusals_come_before_any_launch(L):
    def call(x=A, n=300, dim=64, cent=A, nlist=100, out=A, best=A, ws=A, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.mevi_ivf_assign_workspace_bytes(300, 64, 100)
        return L.mevi_ivf_assign_f32(x, n, dim, cent, nlist, out, best, ws, ws_bytes, None)

    def refused(code, *words, **kw):
        _refused(L, call(**kw), code, words, "ivf_assign:")

    refused(INVALID, "n=-1", n=-1)
    refused(UNSUPPORTED, "n=2147483648", n=1 << 31)
    refused(UNSUPPORTED, "dim=66", "multiple of 4", dim=66)
    refused(INVALID, "dim=0", dim=0)
    refused(UNSUPPORTED, "nlist=0", nlist=0)
    refused(UNSUPPORTED, "nlist=262145", nlist=262145)
    for name, word in (("x", "x is null"), ("cent", "centroids is null"), ("out", "list_of is null"), ("ws", "workspace is null")):
        refused(INVALID, word, **{name: None})
    for name, step, word in (("x", 8, "x is not"), ("cent", 4, "centroids is not"), ("out", 2, "list_of is not"), ("best", 2, "best_score is not"),
                             ("ws", 128, "workspace is not")):
        refused(INVALID, word, "aligned", **{name: A + step})
    need = L.mevi_ivf_assign_workspace_bytes(300, 64, 100)
    refused(WORKSPACE, "workspace", str(need), ws_bytes=need - 1)
    refused(WORKSPACE, "workspace", str(need), ws_bytes=0)
    # no rows: nothing to do, whatever the pointers; a shape outside the envelope is still refused
    assert call(n=0, x=None, cent=None, out=None, best=None, ws=None, ws_bytes=0) == 0
    refused(UNSUPPORTED, "dim=66", n=0, dim=66)


def test_build_lists_refusals_come_before_any_launch(L):
    def call(lab=A, n=3000, nlist=37, off=A, ids=A, longest=A, ws=A, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.mevi_ivf_build_lists_workspace_bytes(3000, 37)
        return L.mevi_ivf_build_lists(lab, n, nlist, off, ids, longest, ws, ws_bytes, None)

    def refused(code, *words, **kw):
        _refused(L, call(**kw), code, words, "ivf_build_lists:")

    refused(INVALID, "n=-1", n=-1)
    refused(UNSUPPORTED, "n=2147483648", n=1 << 31)
    refused(UNSUPPORTED, "nlist=0", nlist=0)
    refused(UNSUPPORTED, "nlist=262145", nlist=262145)
    for name, word in (("lab", "list_of is null"), ("off", "list_offsets is null"), ("ids", "row_ids is null"),
                       ("longest", "max_list_len is null"), ("ws", "workspace is null")):
        refused(INVALID, word, **{name: None})
    for name, step, word in (("lab", 2, "list_of is not"), ("off", 4, "list_offsets is not"), ("ids", 4, "row_ids is not"),
                             ("longest", 4, "max_list_len is not"), ("ws", 128, "workspace is not")):
        refused(INVALID, word, "aligned", **{name: A + step})
    need = L.mevi_ivf_build_lists_workspace_bytes(3000, 37)
    refused(WORKSPACE, "workspace", str(need), ws_bytes=need - 1)
    refused(WORKSPACE, "workspace", str(need), ws_bytes=0)


def test_build_path_is_chosen_in_python(L, monkeypatch):
    from mevi_amd import ivf

    monkeypatch.delenv("MEVI_IVF_BUILD", raising=False)
    assert ivf.build_path() == "device" and ivf.assign_wanted(3000, 32, 37)
    assert not ivf.assign_wanted(3000, 30, 37) and not ivf.assign_wanted(0, 32, 37) and not ivf.assign_wanted(3000, 32, 262145)
    monkeypatch.setenv("MEVI_IVF_BUILD", "host")
    assert ivf.build_path() == "host" and not ivf.assign_wanted(3000, 32, 37)
    # the library does not look at it: the C ABI has no environment variable
    for src in glob.glob(os.path.join(ROOT, "mevi_amd", "csrc", "*")):
        assert '"MEVI_IVF_BUILD"' not in open(src).read(), src
    assert "getenv" not in open(os.path.join(ROOT, "mevi_amd", "csrc", "ivf_build.hip")).read()


def test_the_hand_made_cases_do_what_their_names_say():
    x, cent, winner = bc.tie_case(120)
    lab, score = bc.nearest(x, cent)
    np.testing.assert_array_equal(lab, winner)                              # the lowest copy wins, rows of zeros go to list 0
    for group in bc.TIE_GROUPS:
        rows = np.flatnonzero(winner == group[0])
        for other in group[1:]:                                             # every copy attains the row's maximum, bit for bit
            tied = np.einsum("ij,ij->i", x[rows].astype(np.float64), cent[np.full(len(rows), other)].astype(np.float64))
            assert np.all(np.abs(tied - score[rows]) < 1e-3 * np.abs(score[rows]) + 1e-6)
            np.testing.assert_array_equal(cent[other], cent[group[0]])
    cases = bc.range_cases()
    lab, score = bc.nearest(*cases["all_negative"])
    assert (score < 0).all()
    lab, score = bc.nearest(*cases["near_float_max"])
    assert np.isfinite(score).all() and (score > 2.5e38).all()
    lab, score = bc.nearest(*cases["all_near_minus_float_max"])
    assert np.isfinite(score).all() and (score < -1.4e38).all()
    for nlist in (100, 130, 257):
        lab, _ = bc.nearest(*cases[f"last_column_{nlist}"])
        assert (lab == nlist - 1).all()
    for pattern in bc.LISTS_PATTERNS:
        for nlist in (1, 2, 100, 1025):
            lab = bc.labels(pattern, 5000, nlist)
            off, ids, longest = bc.lists(lab, nlist)
            ok = (lab.astype(np.int64) >= 0) & (lab.astype(np.int64) < nlist)
            assert off[-1] == ok.sum() == len(ids) and longest == np.diff(off).max()
            assert (pattern == "out_of_range") == (not ok.all())
            np.testing.assert_array_equal(lab[ids], np.sort(lab[ok], kind="stable"))
            assert all((np.diff(ids[a:b]) > 0).all() for a, b in zip(off[:-1], off[1:]))      # ids ascend inside a list
