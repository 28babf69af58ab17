"""Host side of the IVF-Flat device scan (mevi_ivf_scan_workspace_bytes / mevi_ivf_scan_topk_f32): the workspace query is
pure arithmetic, monotone and capped, and every documented refusal comes back with its code and a message before anything
is launched (the pointers handed over here are null or fake, so a launch would not go unnoticed)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def test_python_constants_are_the_headers():
    from mevi_amd import dense

    text = open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    assert int(re.search(r"#define MEVI_IVF_SCAN_PAIR_TILE (\d+)", text).group(1)) == dense.IVF_PAIR_TILE
    assert int(re.search(r"#define MEVI_IVF_SCAN_ROW_BLOCK (\d+)", text).group(1)) == dense.IVF_ROW_BLOCK
    assert "#define MEVI_IVF_SCAN_WORKSPACE_CAP (((size_t)2 << 30) + ((size_t)160 << 20))" in text
    assert dense.IVF_WORKSPACE_CAP == (2 << 30) + (160 << 20)


def test_workspace_query_is_host_arithmetic_monotone_and_capped(L):
    from mevi_amd import dense

    f = L.mevi_ivf_scan_workspace_bytes
    base = (6980, 16, 1000, 768, 100, 200000)
    at_c2 = f(*base)
    assert 0 < at_c2 <= dense.IVF_WORKSPACE_CAP
    assert at_c2 == f(*base) == dense.ivf_scan_workspace_bytes(*base)
    # the tile is the number of queries whose candidate scores fit 2 GiB, at most 4096 and at most nq
    tile = L.mevi_ivf_scan_query_tile
    assert tile(*base) == dense.ivf_scan_query_tile(*base) == (2 << 30) // (16 * 200000 * 4)
    assert tile(6980, 1, 10, 64, 8, 1000) == 4096 and tile(33, 1, 10, 64, 8, 1000) == 33 and tile(8, 257, 10, 64, 8, 1000) == 0
    grids = [[1, 2, 31, 32, 33, 64, 65, 4096, 4097, 6980, 100000], [1, 2, 3, 16, 255, 256], [1, 10, 1000, 4096],
             [4, 64, 100, 768, 1024], [1, 2, 100, 4096, 4097, 262144], [0, 1, 127, 128, 129, 5000, 200000, 2000000]]
    for axis, values in enumerate(grids):
        for other in (base, (1, 1, 1, 4, 1, 1), (33, 3, 10, 64, 8, 3000)):
            sizes = []
            for v in values:
                shape = list(other)
                shape[axis] = v
                sizes.append(f(*shape))
            assert all(s > 0 for s in sizes), (axis, sizes)
            assert sizes == sorted(sizes), (axis, sizes)                    # never shrinks when an argument grows
            assert max(sizes) <= dense.IVF_WORKSPACE_CAP
    assert f(1, 256, 4096, 1024, 262144, (2 << 30) // (4 * 256)) <= dense.IVF_WORKSPACE_CAP      # the largest shape of the envelope
    assert f(1 << 40, 256, 4096, 1024, 262144, (2 << 30) // (4 * 256)) <= dense.IVF_WORKSPACE_CAP
    # outside the envelope: 0
    for shape in [(0, 1, 1, 64, 8, 100), (8, 0, 1, 64, 8, 100), (8, 257, 1, 64, 8, 100), (8, 1, 0, 64, 8, 100), (8, 1, 4097, 64, 8, 100),
                  (8, 1, 1, 66, 8, 100), (8, 1, 1, 64, 0, 100), (8, 1, 1, 64, 262145, 100), (8, 256, 1, 64, 8, (2 << 30) // (4 * 256) + 4)]:
        assert f(*shape) == 0, shape


def test_refusals_come_before_any_launch(L):
    from mevi_amd import hip

    A = 1 << 20                                    # a fake, well-aligned device address: nothing may dereference it

    def call(q=A, nq=8, docs=A, off=A, ids=A, nd=5000, nlist=8, longest=1000, dim=64, probe=A, nprobe=2, k=10, out_s=A, out_i=A,
             ws=A, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = L.mevi_ivf_scan_workspace_bytes(nq, nprobe, k, dim, nlist, longest)
        st = L.mevi_ivf_scan_topk_f32(q, nq, docs, off, ids, nd, nlist, longest, dim, probe, nprobe, k, out_s, out_i, ws, ws_bytes, None)
        return st, L.mevi_last_error().decode()

    def refused(code, word, **kw):
        st, msg = call(**kw)
        assert st == code and word in msg and msg.startswith("ivf_scan:"), (kw, st, msg)
        with pytest.raises(hip.MeviHipError, match="ivf_scan"):
            hip.check(st, "mevi_ivf_scan_topk_f32")

    refused(UNSUPPORTED, "multiple of 4", dim=66)
    refused(UNSUPPORTED, "k=0", k=0)
    refused(UNSUPPORTED, "k=4097", k=4097)
    refused(UNSUPPORTED, "nprobe=0", nprobe=0)
    refused(UNSUPPORTED, "nprobe=257", nprobe=257)
    refused(UNSUPPORTED, "32 bits", nd=1 << 31)
    refused(UNSUPPORTED, "envelope", nlist=262145)
    refused(UNSUPPORTED, "envelope", nd=(1 << 31) - 1, longest=(2 << 30) // (4 * 256) + 4, nprobe=256)
    for name in ("q", "docs", "off", "probe", "out_s", "out_i", "ws"):
        refused(INVALID, "null", **{name: None})
    for name, step in (("q", 8), ("docs", 4), ("off", 4), ("ids", 4), ("out_i", 4), ("probe", 2), ("out_s", 2), ("ws", 128)):
        refused(INVALID, "align", **{name: A + step})
    refused(INVALID, "max_list_len", longest=5001)
    need = L.mevi_ivf_scan_workspace_bytes(8, 2, 10, 64, 8, 1000)
    refused(WORKSPACE, str(need), ws_bytes=need - 1)
    refused(WORKSPACE, str(need), ws_bytes=0)
    # no queries: nothing to do, whatever the pointers
    assert call(nq=0, q=None, ws=None, ws_bytes=0)[0] == 0
