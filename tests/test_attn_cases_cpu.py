"""The attention case table (tests/attn_cases.py) without a GPU: every case takes the kernel it names -- asked of the
launchers' own decision functions (mevi_attention*_route) --, every route and every dispatch boundary is covered from both
sides, and the float64 restatement (tests/attn_ref64.py) is finite on every case and equals a literal triple loop."""
import collections
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import attn_cases as A
import attn_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = [c for c in A.CASES if not c.refused]


@pytest.fixture(scope="module")
def lib():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip


def test_route_names_are_the_header_enum(lib):
    text = open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"MEVI_ATTN_ROUTE_([A-Z0-9_]+) = (\d+)", text)}
    assert enum == lib.ATTN_ROUTES
    assert lib.attn_route_name(67) == "FEW_KEYS_STAGED64+3" and lib.attn_route_name(102) == "FEW_KEYS_STAGED96+6"
    assert lib.attn_route_name(-2) == "REFUSED(-2)" and lib.attn_route_name(2) == "TILE"


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_case_takes_the_route_it_names(lib, case):
    from mevi_amd import ops

    route, _ = A.call(case, A.make_inputs(case), "cpu", ops, route_only=True)
    assert lib.attn_route_name(route) == case.route, case.note


def test_every_route_and_every_boundary_is_covered_from_both_sides(lib):
    n = collections.Counter(c.route for c in A.CASES)
    names = [k for k in lib.ATTN_ROUTES if not k.startswith("FEW_KEYS_STAGED")]
    names += [f"FEW_KEYS_STAGED64+{tk}" for tk in range(1, 8)] + [f"FEW_KEYS_STAGED96+{tk}" for tk in range(1, 7)]
    for r in names:
        assert n[r] >= 2, (r, n[r])
    assert n["REFUSED(-2)"] >= 4

    def has(form, route, **kw):
        return any(c.form == form and c.route == route and all(getattr(c, k) == v for k, v in kw.items()) for c in A.CASES)

    sq = lambda S, route, dh=64: has("padded", route, tq=S, tk=S, dh=dh, kv_div=1)       # noqa: E731
    # whole sequences, 64-wide heads: 1 | 2..32 | 33..64 | 65..128 | 129..212 | 213..256 | 257
    assert sq(1, "FEW_KEYS_STAGED64+1") and sq(2, "MFMA16_SELF") and sq(32, "MFMA16_SELF") and sq(33, "TILE")
    assert sq(64, "TILE") and sq(65, "MFMA") and sq(128, "MFMA") and sq(129, "TILE")
    assert sq(212, "TILE") and sq(213, "GENERIC") and sq(256, "GENERIC") and has("padded", "REFUSED(-2)", tk=257)
    assert sq(15, "MFMA16_SELF") and sq(16, "MFMA16_SELF") and sq(17, "MFMA16_SELF") and sq(31, "MFMA16_SELF")
    # the tile LDS limit at 128-wide heads, the smallest tile, the generic kernel below it
    assert sq(106, "TILE", 128) and sq(107, "GENERIC", 128) and sq(8, "TILE", 8) and sq(7, "GENERIC", 32)
    # a few rows against shared keys: tk 8 | 9..32 | 33, kv_div 32 | 33, the group kernel's LDS limit
    one = lambda tk, route, **kw: has("padded", route, tq=1, tk=tk, **kw)       # noqa: E731
    assert one(8, "FEW_KEYS", kv_div=1, mask="") and one(9, "MFMA16_SHARED", kv_div=1) and one(1, "MFMA16_SHARED", mask="ones")
    assert one(32, "MFMA16_SHARED") and one(33, "GROUP", kv_div=10) and one(33, "GENERIC", kv_div=1)
    assert one(16, "MFMA16_SHARED") and one(17, "MFMA16_SHARED")
    for div in (2, 16, 17, 32):
        assert has("padded", "MFMA16_SHARED", kv_div=div), div
    assert one(20, "GROUP", kv_div=33)
    assert one(119, "GROUP", kv_div=10) and one(120, "GENERIC", kv_div=10) and one(128, "GENERIC", kv_div=10)
    assert one(255, "GENERIC") and one(256, "GENERIC")
    # the staged few-keys kernels against the direct one
    assert one(7, "FEW_KEYS_STAGED64+7") and one(8, "FEW_KEYS", dh=64) and one(6, "FEW_KEYS_STAGED96+6", dh=96)
    assert one(7, "FEW_KEYS", dh=96) and one(8, "FEW_KEYS", dh=96)
    # caches: 8 | 9..16 | 17
    assert has("cached", "FEW_KEYS", tk=8, dh=64) and has("cached", "MFMA16_INDEXED", tk=9) and has("cached", "MFMA16_INDEXED", tk=16)
    assert has("cached", "REFUSED(-2)", tk=17) and has("cached", "KEYS16", tk=9, dh=32) and has("cached", "KEYS16", tk=16, dh=128)
    # packed sequences: 32 | 33..64 | 65..128 | 129..212 | 213
    longest = lambda L, route, dh=64: any(c.form == "varlen" and c.route == route and c.dh == dh and     # noqa: E731
                                          (c.max_len or max(c.lens, default=0)) == L for c in A.CASES)
    assert longest(32, "MFMA16_SELF") and longest(33, "VARLEN_SHORT64") and longest(64, "VARLEN_SHORT64")
    assert longest(128, "MFMA") and longest(128, "H16") and longest(129, "VARLEN") and longest(212, "VARLEN")
    assert longest(213, "REFUSED(-2)") and longest(40, "VARLEN", 32) and longest(50, "VARLEN", 128)


def test_every_kernel_sees_every_input_kind_and_both_image_bounds():
    fam = collections.defaultdict(set)
    for c in RUN:
        fam[c.family] |= {c.kind, "split_" + c.split if c.split else "f32", "holes" if c.mask not in ("", "prefix", "ones") else "-"}
    for c in RUN:      # the f32 passage kernel writes an image only under MEVI_ATTN_PASSAGE=f32: the child's cases count for it
        for _, _, route in c.env:
            fam[route.split("+")[0]] |= {"split_" + c.split if c.split else "f32"}
    for f, seen in fam.items():
        want = {"benign", "big_v", "tiny_v", "split_tight", "split_loose"} | ({"peaked"} if f != "H16" else set())
        assert want <= seen, (f, want - seen)
    for f in ("MFMA16_SELF", "MFMA16_SHARED", "FEW_KEYS", "GROUP", "GENERIC", "TILE", "MFMA", "H16"):      # the forms with a key mask
        assert "holes" in fam[f], f
    outs = collections.Counter(c.form if c.form != "kvpacked" else "padded" for c in RUN if c.out_slice)
    assert all(outs[f] >= 2 for f in ("padded", "varlen", "cached")), outs
    for c in RUN:      # no fully masked row: a key mask keeps a real key per kv batch, and a causal case keeps key 0
        m = A.make_inputs(c)["key_mask"]
        assert m is None or bool((m.sum(1) > 0).all()), c.name
        assert not (c.causal and m is not None) or bool(m[:, 0].all()), c.name      # key 0 is causal for every query
        if c.mask.startswith("blank"):
            assert int(m[:, :int(c.mask[5:])].sum()) == 0, c.name


@pytest.mark.parametrize("case", RUN, ids=lambda c: c.name)
def test_restatement_is_finite_and_f32_differs_from_f64(case):
    d = A.make_inputs(case)
    fn = A.reference(case, d)
    r64, r32 = fn(torch.float64, "cpu"), fn(torch.float32, "cpu")
    assert r64.dtype == torch.float64 and r32.dtype == torch.float32 and r64.shape == r32.shape
    assert torch.isfinite(r64).all() and torch.isfinite(r32).all()
    e_32 = (r32.double() - r64).abs().max().item()
    single_key = case.tk == 1 or (case.lens and max(case.lens) == 1)
    if single_key:      # softmax over one key is exactly 1 and the context exactly that key's V row, in any precision
        assert e_32 == 0.0
    else:
        assert e_32 > 0.0


@pytest.mark.parametrize("name", ["generic-tq4-tk9-causal", "few-dh32-div3-tk5", "tile-dh8-S8", "few-dh4-tk8"])
def test_restatement_equals_a_literal_triple_loop(name):
    c = A.BY_NAME[name]
    d = A.make_inputs(c)
    assert c.form == "padded"
    want = R.triple_loop(d["q"], d["k"], d["v"], c.H, kv_div=c.kv_div, bias=d["bias"], q_pos0=c.q_pos0, key_mask=d["key_mask"],
                         causal=c.causal, scale=c.scale)
    got = A.reference(c, d)(torch.float64, "cpu")
    assert (got - want).abs().max().item() <= 1e-13 * max(1.0, want.abs().max().item())


def test_packed_and_cached_restatements_equal_the_padded_one():
    """The three other layouts are the padded form on re-arranged rows: sequence by sequence, and on the gathered caches."""
    c = A.BY_NAME["short64-L33"]
    d = A.make_inputs(c)
    got = A.reference(c, d)(torch.float64, "cpu")
    at = 0
    for a, b in zip(d["off"][:-1], d["off"][1:]):
        if b > a:
            one = R.padded(d["q"][None, a:b], d["k"][None, a:b], d["v"][None, a:b], c.H, bias=d["bias"][:, :b - a, :b - a].contiguous())
            assert (one(torch.float64, "cpu")[0] - got[at:at + b - a]).abs().max().item() <= 1e-14
            at += b - a
    assert at == got.shape[0]
    c = A.BY_NAME["group-packed-dh32"]
    d = A.make_inputs(c)
    got = A.reference(c, d)(torch.float64, "cpu")
    L = max(c.lens)
    k, v = torch.zeros((c.nb, L, c.H * c.dh)), torch.zeros((c.nb, L, c.H * c.dh))
    m = torch.zeros((c.nb, L), dtype=torch.int64)
    for i, (a, b) in enumerate(zip(d["off"][:-1], d["off"][1:])):
        k[i, :b - a], v[i, :b - a], m[i, :b - a] = d["k"][a:b], d["v"][a:b], 1
    one = R.padded(d["q"], k, v, c.H, kv_div=c.kv_div, bias=d["bias"], key_mask=m)(torch.float64, "cpu")
    assert (one - got).abs().max().item() <= 1e-14
    c = A.BY_NAME["cached-dh32-tk9"]
    d = A.make_inputs(c)
    got = A.reference(c, d)(torch.float64, "cpu")
    want = torch.zeros_like(got)
    for b in range(c.nb):
        kg = torch.stack([d["k"][int(d["key_rows"][b, j]), j] for j in range(c.tk)])[None]
        vg = torch.stack([d["v"][int(d["key_rows"][b, j]), j] for j in range(c.tk)])[None]
        want[b] = R.triple_loop(d["q"][b][None, None], kg, vg, c.H, bias=d["bias"], q_pos0=c.q_pos0, causal=True)[0, 0]
    assert (got - want).abs().max().item() <= 1e-13


@pytest.mark.parametrize("switch", ["MEVI_ATTN_SHORT", "MEVI_ATTN_FEW_KEYS", "MEVI_ATTN_PASSAGE"])
def test_switches_move_the_cases_that_name_them(lib, switch):
    """The three environment switches are read once per process: a fresh child answers for the cases that name the switch."""
    value = {"MEVI_ATTN_SHORT": "chain", "MEVI_ATTN_FEW_KEYS": "direct", "MEVI_ATTN_PASSAGE": "f32"}[switch]
    want = {c.name: e[2] for c in A.CASES for e in c.env if e[:2] == (switch, value)}
    assert len(want) >= 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "attn_f64_child.py"), switch, value, "--routes-only"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    got = {j["case"]: j["route"] for j in map(json.loads, (l for l in r.stdout.splitlines() if l.startswith("{")))}
    assert got == want
    assert all(A.BY_NAME[n].route != r for n, r in want.items())      # the switch does change these cases' kernel
