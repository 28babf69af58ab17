"""The two block-streaming attention kernels (mevi_amd/csrc/attention_long.hip) against float64, on the 128-key blocks.

Inputs, layouts and the float64 restatement are those of tests/attn_cases.py and tests/attn_ref64.py; the bar is the project's
own (tests/f64_bar.py):

    e_hip <= 4 e_32 + 2^-22 max |ref64|

with ref32 in CHAIN order (blocked=False): the f32 matrix cores are bitwise an fmaf chain over k and both kernels accumulate
the context over the keys in ascending blocks.  e_32_blocked (the library matmul form) is recorded beside it as a property,
not as a condition.  Then the bit-level invariants the two-sweep softmax makes true: packed = padded on the real rows,
kv_off = key mask, alone = inside a batch, and an out= slice leaves every byte outside it untouched."""
import numpy as np
import pytest
import torch

import attn_cases as A
import f64_bar

pytestmark = pytest.mark.gpu


def case(name, form="padded", **kw):
    kw.setdefault("H", 2)
    kw.setdefault("route", "LONG_MFMA")
    return A.Case(name="long-" + name, form=form, **kw)


def prefix_mask(lens, S):
    return (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).to(torch.int64)


def run(c, d, dev, out=None):
    """The case through ops.attention_long / attention_long_varlen -> (route name, context on the device: the rows of the
    reference)."""
    from mevi_amd import hip, ops

    hd = c.H * c.dh
    to = lambda x: None if x is None else x.to(dev)     # noqa: E731
    kw = dict(bias=to(d["bias"]), causal=c.causal, scale=c.scale)
    if out is not None:
        kw["out"] = out
    if c.form == "varlen":
        off = d["off"]
        q, k, v = A._nan_slices([d["q"], d["k"], d["v"]], dev, (off[0], off[-1]))
        args = (q, k, v, torch.tensor(off, dtype=torch.int64, device=dev), c.max_len or max(c.lens), c.H)
        route = ops.attention_long_varlen_route(*args, **kw)
        got = ops.attention_long_varlen(*args, **kw)
        return hip.attn_route_name(route), got[off[0]:off[-1]]
    if c.form == "kvpacked":
        off = d["off"]
        k, v = A._nan_slices([d["k"], d["v"]], dev, (off[0], off[-1]))
        kw.update(kv_off=torch.tensor(off, dtype=torch.int64, device=dev), kv_longest=c.tk or max(c.lens))
    else:
        kv = torch.cat([d["k"], d["v"]], -1).to(dev)       # K | V side by side, as the fused projections hold them
        k, v = kv[..., :hd], kv[..., hd:]
        kw.update(key_mask=to(d["key_mask"]))
    args = (to(d["q"]), k, v, c.H)
    kw.update(kv_div=c.kv_div, q_pos0=c.q_pos0)
    route = ops.attention_long_route(*args, **kw)
    return hip.attn_route_name(route), ops.attention_long(*args, **kw)


def hold(c, d, dev, record_property, valid=None):
    ref64, ref32 = f64_bar.refs(c.name, A.reference(c, d))
    blocked = A.reference(c, d, blocked=True)(torch.float32, "cpu")
    route, got = run(c, d, dev)
    torch.cuda.synchronize()
    assert route == c.route
    assert got.shape == ref64.shape
    e_blocked = (blocked.double() - ref64.cpu()).abs().max().item()
    record_property(c.name + "/e_32_blocked", e_blocked)
    print(f"{c.name}: route {route}  e_32_blocked {e_blocked:.3e}")
    f64_bar.check(c.name, got, ref64, ref32, valid, record_property)
    return got


# ---- LONG_MFMA ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [129, 256, 257, 384, 385, 513])
def test_matrix_core_kernel_with_the_bias_table(cuda, S, record_property):
    c = case(f"mfma-S{S}", nb=3, tq=S, tk=S)
    hold(c, A.make_inputs(c), cuda, record_property)


def test_matrix_core_kernel_right_padded_lengths_in_one_batch(cuda, record_property):
    S = 385
    lens = (S, 257, 129, 128, 1)
    c = case("mfma-prefix", nb=len(lens), tq=S, tk=S, mask="ones")
    d = A.make_inputs(c)
    d["key_mask"] = prefix_mask(lens, S)
    hold(c, d, cuda, record_property)


def test_matrix_core_kernel_holes_and_a_blank_leading_block(cuda, record_property):
    S = 300
    c = case("mfma-holes", nb=3, tq=S, tk=S, mask="holes")
    d = A.make_inputs(c)
    d["key_mask"][1, :128] = 0          # the first key block of one row wholly masked: its maximum so far is s - 1e9
    d["key_mask"][1, 200] = 1
    assert int(d["key_mask"][1, :128].sum()) == 0 and bool((d["key_mask"].sum(1) > 0).all())
    hold(c, d, cuda, record_property)


def test_matrix_core_kernel_peaked_logits(cuda, record_property):
    c = case("mfma-peaked", nb=3, tq=300, tk=300, kind="peaked")
    hold(c, A.make_inputs(c), cuda, record_property)


def test_matrix_core_kernel_causal(cuda, record_property):
    c = case("mfma-causal", nb=3, tq=300, tk=300, causal=True)
    hold(c, A.make_inputs(c), cuda, record_property)


def test_matrix_core_kernel_shifted_query_positions(cuda, record_property):
    """q_pos0 moves the bias rows and the causal edge (key j allowed iff j <= q_pos0 + t); the table is wider than tk and odd"""
    c = case("mfma-qpos7", nb=2, tq=260, tk=260, q_pos0=7, causal=True, bias_pad=3)
    hold(c, A.make_inputs(c), cuda, record_property)


def test_matrix_core_kernel_packed_sequences(cuda, record_property):
    c = case("mfma-packed", form="varlen", lens=(385, 257, 129, 0, 128, 1), off0=3)
    hold(c, A.make_inputs(c), cuda, record_property)


# ---- LONG_ROWS ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dh", [8, 96, 128])
def test_rows_kernel_head_widths(cuda, dh, record_property):
    c = case(f"rows-dh{dh}", route="LONG_ROWS", dh=dh, nb=2, tq=260, tk=260, mask="prefix", scale=dh ** -0.5)
    hold(c, A.make_inputs(c), cuda, record_property)


@pytest.mark.parametrize("kv_div", [1, 3])
@pytest.mark.parametrize("tk", [257, 300, 513])
def test_rows_kernel_one_query_behind_a_key_mask(cuda, tk, kv_div, record_property):
    c = case(f"rows-tq1-tk{tk}-div{kv_div}", route="LONG_ROWS", dh=64, nb=3 * kv_div, tq=1, tk=tk, kv_div=kv_div, mask="ones")
    d = A.make_inputs(c)
    d["key_mask"] = prefix_mask((tk, 1, 257), tk)
    hold(c, d, cuda, record_property)


@pytest.mark.parametrize("kv_div", [1, 3])
def test_rows_kernel_one_query_against_packed_keys(cuda, kv_div, record_property):
    c = case(f"rows-kvoff-div{kv_div}", form="kvpacked", route="LONG_ROWS", dh=64, nb=3, kv_div=kv_div, lens=(300, 1, 257), off0=5)
    hold(c, A.make_inputs(c), cuda, record_property)


def test_rows_kernel_late_queries_causal(cuda, record_property):
    c = case("rows-tq5-qpos295", route="LONG_ROWS", dh=64, nb=3, tq=5, tk=300, q_pos0=295, causal=True)
    hold(c, A.make_inputs(c), cuda, record_property)


def test_rows_kernel_packed_sequences(cuda, record_property):
    c = case("rows-packed-dh8", form="varlen", route="LONG_ROWS", dh=8, lens=(300, 1, 0, 257), off0=2)
    hold(c, A.make_inputs(c), cuda, record_property)


# ---- bit-level invariants ------------------------------------------------------------------------------------------------------

def _packed_twin(c, d, lens):
    """The varlen case whose sequences are the real rows of the padded case (c, d) with right-padded lengths `lens`"""
    v = case(c.name[5:] + "-as-packed", form="varlen", route=c.route, dh=c.dh, lens=tuple(lens), off0=1, causal=c.causal, scale=c.scale)
    rows = 1 + sum(lens) + 2
    dv = dict(bias=d["bias"], key_mask=None, key_rows=None, off=A._offsets(v))
    for name in ("q", "k", "v"):
        t = torch.zeros((rows, c.H * c.dh))
        for b, (a, e) in enumerate(zip(dv["off"][:-1], dv["off"][1:])):
            t[a:e] = d[name][b, :e - a]
        dv[name] = t
    return v, dv


@pytest.mark.parametrize("dh,route", [(64, "LONG_MFMA"), (8, "LONG_ROWS")])
def test_packed_equals_padded_on_the_real_rows(cuda, dh, route):
    S, lens = 385, (385, 257, 129, 128, 1)
    c = case(f"inv-packed-{dh}", route=route, dh=dh, nb=len(lens), tq=S, tk=S, mask="ones", causal=dh == 8)
    d = A.make_inputs(c)
    d["key_mask"] = prefix_mask(lens, S)
    r1, padded = run(c, d, cuda)
    v, dv = _packed_twin(c, d, lens)
    r2, packed = run(v, dv, cuda)
    assert r1 == r2 == route
    real = torch.cat([padded[b, :n] for b, n in enumerate(lens)])
    assert torch.isfinite(packed).all() and torch.equal(real, packed)


@pytest.mark.parametrize("kv_div", [1, 3])
def test_packed_keys_equal_masked_keys(cuda, kv_div):
    lens = (300, 1, 257)
    c = case(f"inv-kvoff-{kv_div}", form="kvpacked", route="LONG_ROWS", dh=64, nb=3, kv_div=kv_div, lens=lens, off0=5)
    d = A.make_inputs(c)
    r1, packed = run(c, d, cuda)
    m = case(f"inv-kvmask-{kv_div}", route="LONG_ROWS", dh=64, nb=3 * kv_div, tq=1, tk=300, kv_div=kv_div, mask="ones")
    dm = dict(d, key_mask=prefix_mask(lens, 300), off=None)
    for name in ("k", "v"):
        t = torch.randn((3, 300, c.H * c.dh))                # padded rows hold finite junk: their weight is an exact zero
        for b, (a, e) in enumerate(zip(d["off"][:-1], d["off"][1:])):
            t[b, :e - a] = d[name][a:e]
        dm[name] = t
    r2, masked = run(m, dm, cuda)
    assert r1 == r2 == "LONG_ROWS"
    assert torch.isfinite(masked).all() and torch.equal(packed, masked)


@pytest.mark.parametrize("dh,route,tq", [(64, "LONG_MFMA", 300), (96, "LONG_ROWS", 300), (64, "LONG_ROWS", 1)])
def test_a_sequence_alone_equals_the_same_sequence_inside_a_batch(cuda, dh, route, tq):
    c = case(f"inv-alone-{dh}-{tq}", route=route, dh=dh, nb=3, tq=tq, tk=300, mask="prefix")
    d = A.make_inputs(c)
    _, batch = run(c, d, cuda)
    for b in (1, 2):
        one = case(f"inv-alone-{dh}-{tq}-{b}", route=route, dh=dh, nb=1, tq=tq, tk=300, mask="prefix")
        d1 = dict(d, q=d["q"][b:b + 1], k=d["k"][b:b + 1], v=d["v"][b:b + 1], key_mask=d["key_mask"][b:b + 1])
        r, alone = run(one, d1, cuda)
        assert r == route and torch.equal(alone[0], batch[b])


@pytest.mark.parametrize("form,dh,route", [("padded", 64, "LONG_MFMA"), ("padded", 96, "LONG_ROWS"), ("varlen", 64, "LONG_MFMA"),
                                           ("varlen", 8, "LONG_ROWS")])
def test_an_out_slice_with_a_larger_row_stride_keeps_its_surroundings(cuda, form, dh, route):
    if form == "padded":
        c = case(f"inv-out-{dh}", route=route, dh=dh, nb=2, tq=260, tk=260, mask="prefix")
        shape = (2, 260)
    else:
        c = case(f"inv-out-packed-{dh}", form="varlen", route=route, dh=dh, lens=(260, 3, 129), off0=2)
        shape = (2 + 260 + 3 + 129 + 2,)
    d = A.make_inputs(c)
    hd = c.H * dh
    r0, plain = run(c, d, cuda)
    wide = torch.full((*shape, hd + 8), A.SENTINEL, dtype=torch.float32, device=cuda)
    r1, got = run(c, d, cuda, out=wide[..., 4:4 + hd])
    # (the slice starts 16 bytes into a row of hd + 8 floats: still aligned, the matrix-core route stays)
    assert r0 == r1 == route and torch.equal(plain, got)
    ref = torch.full_like(wide, A.SENTINEL)
    if form == "padded":
        ref[..., 4:4 + hd] = plain
    else:
        ref[2:2 + 392, 4:4 + hd] = plain
    assert torch.equal(ref.view(torch.int32), wide.view(torch.int32))


# ---- refusals and empty calls ---------------------------------------------------------------------------------------------------

def test_refusals_raise_with_their_status(cuda):
    from mevi_amd import hip, ops

    def qkv(nb, tq, tk, hd):
        return (torch.zeros((nb, tq, hd), device=cuda), torch.zeros((nb, tk, hd), device=cuda), torch.zeros((nb, tk, hd), device=cuda))

    with pytest.raises(hip.MeviHipError, match=r"status -2: .*tk=2049"):
        ops.attention_long(*qkv(1, 1, 2049, 128), 2)
    with pytest.raises(hip.MeviHipError, match=r"status -2: .*dh=132"):
        ops.attention_long(*qkv(1, 4, 300, 264), 2)
    with pytest.raises(hip.MeviHipError, match=r"status -1: .*bias table too small"):
        ops.attention_long(*qkv(1, 300, 300, 128), 2, bias=torch.zeros((2, 300, 299), device=cuda))
    with pytest.raises(hip.MeviHipError, match=r"status -1: .*bias table too small"):
        ops.attention_long(*qkv(1, 5, 300, 128), 2, bias=torch.zeros((2, 300, 300), device=cuda), q_pos0=296)
    off = torch.tensor([0, 2049], dtype=torch.int64, device=cuda)
    x = torch.zeros((2049, 128), device=cuda)
    with pytest.raises(hip.MeviHipError, match=r"status -2: .*max_len=2049"):
        ops.attention_long_varlen(x, x, x, off, 2049, 2)
    # the existing calls keep their envelope
    with pytest.raises(hip.MeviHipError, match=r"status -2: .*tk=257 > 256"):
        ops.attention(*qkv(1, 257, 257, 128), 2)
    with pytest.raises(hip.MeviHipError, match="status -2:"):
        ops.attention_varlen(x[:213 * 3, :], x[:213 * 3], x[:213 * 3], torch.tensor([0, 213, 426, 639], device=cuda), 213, 2)
    torch.cuda.synchronize()


def test_empty_calls_return_empty_contexts(cuda):
    from mevi_amd import ops

    e = torch.zeros((0, 300, 128), device=cuda)
    assert ops.attention_long(e, e, e, 2).shape == (0, 300, 128)
    x = torch.zeros((0, 128), device=cuda)
    assert ops.attention_long_varlen(x, x, x, torch.zeros(1, dtype=torch.int64, device=cuda), 300, 2).shape == (0, 128)
    torch.cuda.synchronize()
