"""The case table of tests/test_attn_f64_gpu.py and tests/test_attn_cases_cpu.py (TEST INFRASTRUCTURE ONLY): every attention
kernel of mevi_amd/csrc/t5_ops.hip at its dispatch edges, each case naming the ROUTE it must take (hip.ATTN_ROUTES; the
launchers' own decision functions answer through ops.attention*_route), plus what builds a case's inputs, runs it through
mevi_amd.ops and measures it against tests/attn_ref64.py.

Forms: `padded` (ops.attention), `kvpacked` (ops.attention with kv_off), `varlen` (ops.attention_varlen), `cached`
(ops.attention_cached).  Input kinds:
    benign   N(0, 1) throughout
    peaked   q scaled so that the logits' standard deviation is 30, bias entries uniform in [-40, 0], two keys per row tied to
             within 1e-3 (logit and bias)
    big_v    V scaled by 1e4, odd key rows the negation of the even row before them
    tiny_v   V scaled by 1e-6
    holes    (a mask kind) a non-prefix key mask; every kv batch keeps a real key, so no row is fully masked
The packed forms read q | k | v as column slices of one wider buffer whose rows before off[0] and after off[-1] are NaN.

Two shapes that look like they belong elsewhere, with the launcher's arithmetic: tk = 120, kv_div = 10, dh = 64 needs
(120 * 132 + 640) * 4 = 65 920 B > 65 536 B of LDS in the group kernel, so 119 is the last group shape and 120 takes the generic
kernel; and tq = tk = 1 is a decode step (few-keys kernel), not the generic kernel."""
import dataclasses
import math
import zlib
from dataclasses import dataclass

import numpy as np
import torch

import attn_ref64 as R

UNSUPPORTED = -2      # MEVI_ERR_UNSUPPORTED


@dataclass(frozen=True)
class Case:
    name: str
    form: str                 # padded | kvpacked | varlen | cached
    route: str                # hip.attn_route_name of the expected route, or "REFUSED(status)"
    H: int = 3
    dh: int = 64
    nb: int = 0               # padded: rows; kvpacked: number of kv batches (rows = nb * kv_div); cached: rows
    tq: int = 1
    tk: int = 0               # padded / cached: keys; kvpacked: kv_longest (0: the longest length)
    kv_div: int = 1
    lens: tuple = ()          # varlen / kvpacked: the sequences' lengths
    max_len: int = 0          # varlen (0: the longest length)
    off0: int = 0             # varlen / kvpacked: off[0]
    kind: str = "benign"
    mask: str = ""            # padded: "" | prefix | ones | holes | blank16 | blank32 | blank64
    causal: bool = False
    scale: float = 1.0
    q_pos0: int = 0
    bias: bool = True
    bias_pad: int = 0         # extra bias columns (bias_ld > tk)
    order: str = "random"     # cached: key_rows random | repeat_desc (repeats, descending rows)
    split: str = ""           # "" (f32 output) | tight | loose (37 x): the context as the split image
    out_slice: bool = False   # out= a column slice of a sentinel-filled buffer
    mask_as: str = ""         # how the key mask is handed over: "" (int64, contiguous, on the device) | bool | host | strided32
    env: tuple = ()           # ((switch, value, route under the switch), ...): run in a fresh child process
    seed: str = ""            # cases with the same seed share inputs (and references); default: the name
    note: str = ""

    @property
    def inputs_key(self):
        return self.seed or self.name

    @property
    def family(self):
        return self.route.split("+")[0]

    @property
    def refused(self):
        return self.route.startswith("REFUSED") or self.route == "NONE"


def _var(base, suffix, **kw):
    kw.setdefault("seed", base.inputs_key if set(kw) <= {"split", "out_slice", "env", "route", "note", "mask_as"} else "")
    return dataclasses.replace(base, name=f"{base.name}-{suffix}", **kw)


def _family(base, kinds=("peaked", "big_v", "tiny_v"), holes=False, split_route=None, splits=True):
    """base + one variant per input kind + the split-image pair (tight, 37 x loose)"""
    out = [base] + [_var(base, kd, kind=kd) for kd in kinds]
    if holes:
        out.append(_var(base, "holes", mask="holes"))
    if splits:
        r = split_route or base.route
        out += [_var(base, "img_tight", split="tight", route=r), _var(base, "img_loose", split="loose", route=r)]
    return out


def _table():
    P = lambda name, nb, tq, tk, route, **kw: Case(name, "padded", route, nb=nb, tq=tq, tk=tk, **kw)       # noqa: E731
    V = lambda name, lens, route, **kw: Case(name, "varlen", route, lens=tuple(lens), **kw)                  # noqa: E731
    K = lambda name, lens, kv_div, route, **kw: Case(name, "kvpacked", route, nb=len(lens), lens=tuple(lens),  # noqa: E731
                                                     kv_div=kv_div, **kw)
    C = lambda name, nb, tk, route, **kw: Case(name, "cached", route, nb=nb, tk=tk, causal=True,             # noqa: E731
                                               q_pos0=tk - 1, **kw)
    chain = "MEVI_ATTN_SHORT", "chain"
    direct = "MEVI_ATTN_FEW_KEYS", "direct"
    f32 = "MEVI_ATTN_PASSAGE", "f32"
    t = []

    # ---- attention_mfma16_kernel, mode 0: whole sequences of 2 .. 32 tokens, 64-wide heads (four pairs per workgroup) ----------
    for S, nb, H in ((2, 3, 3), (15, 2, 3), (16, 1, 3), (31, 5, 3), (32, 7, 2)):
        t.append(P(f"self16-S{S}", nb, S, S, "MFMA16_SELF", H=H, mask="prefix" if S > 2 else "",
                   env=((*chain, "GENERIC"),) if S == 2 else ()))
    t += _family(P("self16-S17", 3, 17, 17, "MFMA16_SELF", mask="prefix", env=((*chain, "TILE"),)), holes=True)
    t.append(P("self16-S17-causal", 2, 17, 17, "MFMA16_SELF", causal=True, scale=0.5))
    t.append(P("self16-S32-blank16", 3, 32, 32, "MFMA16_SELF", mask="blank16"))
    t.append(P("self16-S32-out", 3, 32, 32, "MFMA16_SELF", out_slice=True))
    t += _family(V("self16-varlen", (32, 1, 0, 16, 17), "MFMA16_SELF", env=((*chain, "VARLEN_SHORT64"),)))
    t.append(V("self16-varlen-out", (31, 1, 0, 16, 17, 2), "MFMA16_SELF", off0=5, out_slice=True, causal=True))
    t.append(P("self-S1", 3, 1, 1, "FEW_KEYS_STAGED64+1", note="S = 1 is a decode step: below the mfma16 range"))

    # ---- attention_mfma16_kernel, mode 1: <= 32 rows against <= 32 shared keys -------------------------------------------------
    t.append(P("shared16-tk1-mask", 5, 1, 1, "MFMA16_SHARED", mask="ones", env=((*chain, "FEW_KEYS_STAGED64+1"),)))
    t.append(P("shared16-tk9", 5, 1, 9, "MFMA16_SHARED", env=((*chain, "GENERIC"),)))
    t.append(P("shared16-tk16-div2", 6, 1, 16, "MFMA16_SHARED", kv_div=2, mask="prefix"))
    t += _family(P("shared16-tk17-div16", 48, 1, 17, "MFMA16_SHARED", kv_div=16, mask="prefix", env=((*chain, "GROUP"),)),
                 holes=True)
    t.append(P("shared16-tk32-div17", 51, 1, 32, "MFMA16_SHARED", kv_div=17, mask="blank16"))
    t.append(P("shared16-tk9-div32-causal", 96, 1, 9, "MFMA16_SHARED", kv_div=32, causal=True, q_pos0=5, H=2))
    t.append(P("shared16-tk32-div32", 32, 1, 32, "MFMA16_SHARED", kv_div=32, mask="holes"))
    t.append(K("shared16-packed", (1, 9, 5), 2, "MFMA16_SHARED", off0=3, env=((*chain, "GROUP"),)))
    t.append(K("shared16-packed-div1", (32, 1, 17, 2, 8), 1, "MFMA16_SHARED", off0=3, kind="peaked"))
    t.append(P("shared16-tk8", 5, 1, 8, "FEW_KEYS", note="no mask, kv_div 1, tk <= 8: below mode 1"))
    t.append(P("shared16-tk20-div33", 66, 1, 20, "GROUP", kv_div=33, H=2, note="kv_div 33 is outside mode 1"))

    # ---- attention_few_keys_kernel (direct): tq 1, <= 8 keys, eight pairs per wave ---------------------------------------------
    for dh in (4, 32, 128):
        for tk in (1, 8):
            t.append(P(f"few-dh{dh}-tk{tk}", 5, 1, tk, "FEW_KEYS", dh=dh, causal=tk > 1, q_pos0=tk - 1))
    t += _family(P("few-dh64-tk8", 5, 1, 8, "FEW_KEYS", causal=True, q_pos0=7))
    t.append(P("few-dh96-tk7", 3, 1, 7, "FEW_KEYS", dh=96, H=2, causal=True, q_pos0=6, scale=96 ** -0.5))
    t.append(P("few-dh96-tk8", 3, 1, 8, "FEW_KEYS", dh=96, H=2))
    t.append(P("few-dh32-div3-tk5", 9, 1, 5, "FEW_KEYS", dh=32, kv_div=3, mask="holes"))
    t.append(P("few-S1-dh32", 3, 1, 1, "FEW_KEYS", dh=32, note="tq = tk = 1 is a decode step, not the generic kernel"))

    # ---- attention_few_keys_staged_kernel<tk, 64 | 96>: once through ops.attention, once through the caches --------------------
    for dh, top in ((64, 7), (96, 6)):
        for tk in range(1, top + 1):
            edge = tk in (1, top)
            e = ((*direct, "FEW_KEYS"),) if edge else ()
            p = P(f"staged{dh}-tk{tk}", 5, 1, tk, f"FEW_KEYS_STAGED{dh}+{tk}", dh=dh, causal=tk > 1, q_pos0=tk - 1, env=e)
            t += _family(p) if (dh, tk) in ((64, 7), (96, 6)) else [p]
            t.append(C(f"staged{dh}-cached-tk{tk}", 7, tk, f"FEW_KEYS_STAGED{dh}+{tk}", dh=dh,
                       split=("tight", "loose")[tk % 2] if not edge else "", order="repeat_desc" if tk % 3 == 0 else "random"))

    # ---- attention_group_kernel: the kv_div rows of a query share K | V (LDS (tk (2 dh + 4) + kv_div dh) 4 <= 65536) -----------
    for tk in (33, 64, 65):
        t.append(P(f"group-tk{tk}-div10", 20, 1, tk, "GROUP", kv_div=10, mask="prefix", H=2))
    t += _family(P("group-tk119-div10", 20, 1, 119, "GROUP", kv_div=10, mask="prefix", H=2,
                   note="65 392 B: the last shape that fits"), holes=True)
    t.append(P("group-tk120-div10", 20, 1, 120, "GENERIC", kv_div=10, mask="prefix", H=2, note="65 920 B does not fit"))
    t.append(P("group-dh32-tk9", 6, 1, 9, "GROUP", dh=32, kv_div=3, mask="holes"))
    t.append(K("group-packed-dh32", (1, 9, 30), 4, "GROUP", dh=32, off0=3))
    t.append(P("group-tk64-out", 20, 1, 64, "GROUP", kv_div=10, H=2, out_slice=True, mask="blank32"))

    # ---- attention_kernel (generic) --------------------------------------------------------------------------------------------
    t += _family(P("generic-tk128-div10", 20, 1, 128, "GENERIC", kv_div=10, mask="prefix", H=2,
                   note="group LDS 70 144 B > 65 536 B"), holes=True)
    for tk in (33, 255, 256):
        t.append(P(f"generic-tq1-tk{tk}", 3, 1, tk, "GENERIC", H=2, mask="blank64" if tk == 255 else "prefix"))
    t.append(P("generic-S7-dh32", 3, 7, 7, "GENERIC", dh=32))
    t.append(P("generic-S213", 2, 213, 213, "GENERIC", H=2, mask="prefix", note="tile LDS 164 436 B > 160 KiB"))
    t.append(P("generic-S256", 1, 256, 256, "GENERIC", H=2, causal=True))
    t.append(P("generic-tq7-tk200", 2, 7, 200, "GENERIC", H=2, mask="holes"))
    t.append(P("generic-tq4-tk9-causal", 3, 4, 9, "GENERIC", causal=True, q_pos0=5))
    t.append(P("generic-dh128-S107", 2, 107, 107, "GENERIC", dh=128, H=2))
    t.append(K("generic-packed-div1", (40, 1, 33), 1, "GENERIC", off0=3, H=2))

    # ---- attention_tile_kernel: tq = tk >= 8, LDS tk (3 dh + 1) 4 <= 160 KiB ---------------------------------------------------
    t += _family(P("tile-S33", 3, 33, 33, "TILE", mask="prefix"), holes=True)
    for S in (63, 64, 129, 212):
        t.append(P(f"tile-S{S}", 2, S, S, "TILE", H=2, mask="prefix" if S != 129 else "blank64", causal=S == 63))
    t.append(P("tile-dh128-S106", 2, 106, 106, "TILE", dh=128, H=2))
    t.append(P("tile-dh8-S8", 3, 8, 8, "TILE", dh=8))
    t.append(P("tile-dh32-S256", 1, 256, 256, "TILE", dh=32, H=2, mask="prefix"))
    t.append(P("tile-S33-out", 3, 33, 33, "TILE", out_slice=True, causal=True, scale=0.5))
    # key masks the wrapper has to convert (bool, on the host, int32 with a stride): the copy must outlive the launch
    t.append(P("tile-S33-mask_bool", 3, 33, 33, "TILE", mask="prefix", mask_as="bool", seed="tile-S33"))
    t.append(P("tile-S33-holes-mask_host", 3, 33, 33, "TILE", mask="holes", mask_as="host", seed="tile-S33-holes"))
    t.append(P("generic-tk128-div10-holes-mask_strided32", 20, 1, 128, "GENERIC", kv_div=10, mask="holes", H=2,
               mask_as="strided32", seed="generic-tk128-div10-holes"))
    t.append(P("shared16-tk17-div16-holes-mask_bool", 48, 1, 17, "MFMA16_SHARED", kv_div=16, mask="holes", mask_as="bool",
               seed="shared16-tk17-div16-holes"))
    t.append(P("passage-S96-holes-mask_host", 2, 96, 96, "MFMA", mask="holes", mask_as="host", seed="passage-S96-holes"))
    t.append(P("passage-S96-holes-img-mask_strided32", 2, 96, 96, "H16", mask="holes", mask_as="strided32", split="tight",
               seed="passage-S96-holes"))

    # ---- attention_mfma_kernel (f32 output) and attention_h16_kernel (image output): 65 .. 128 tokens, 64-wide heads -----------
    for S in (65, 127, 128):
        b = P(f"passage-S{S}", 2, S, S, "MFMA", mask="prefix")
        t += [b, _var(b, "img_tight", split="tight", route="H16")]
    t += _family(P("passage-S96", 2, 96, 96, "MFMA", mask="prefix"), holes=True, splits=False)
    t.append(P("passage-S96-img_tight", 2, 96, 96, "H16", mask="prefix", split="tight", seed="passage-S96", env=((*f32, "MFMA"),)))
    t.append(P("passage-S96-img_loose", 2, 96, 96, "H16", mask="prefix", split="loose", seed="passage-S96", env=((*f32, "MFMA"),)))
    for kd in ("big_v", "tiny_v"):      # (`peaked` stays off the f16 kernel: its operand scaling has no derived bar for it)
        t.append(P(f"passage-S96-{kd}-img", 2, 96, 96, "H16", mask="prefix", kind=kd, split="tight", seed=f"passage-S96-{kd}"))
    t.append(P("passage-S96-holes-img", 2, 96, 96, "H16", mask="holes", split="loose", seed="passage-S96-holes"))
    b = P("passage-S96-causal", 2, 96, 96, "MFMA", causal=True, scale=0.5)
    t += [b, _var(b, "img", split="tight", route="H16")]
    b = P("passage-S128-blank64", 2, 128, 128, "MFMA", mask="blank64")
    t += [b, _var(b, "img", split="loose", route="H16")]
    b = V("passage-varlen", (128, 65, 1, 0, 97), "MFMA")
    t += [b, _var(b, "img", split="tight", route="H16", env=((*f32, "MFMA"),))]

    # ---- attention_varlen_short_kernel<64>: packed sequences of 33 .. 64 tokens, 64-wide heads ---------------------------------
    t += _family(V("short64-L33", (33, 1, 20, 0, 7, 2), "VARLEN_SHORT64"))
    t.append(V("short64-L64", (64, 33, 5, 1, 40), "VARLEN_SHORT64", causal=True, scale=0.5))
    t.append(V("short64-L64-out", (64, 3, 34), "VARLEN_SHORT64", off0=5, out_slice=True))

    # ---- attention_varlen_kernel -----------------------------------------------------------------------------------------------
    t += _family(V("varlen-dh32-L40", (40, 3, 17, 1, 9), "VARLEN", dh=32, note="four waves per workgroup, 15 pairs"))
    t.append(V("varlen-L129", (129, 70, 2), "VARLEN", H=2, note="one wave per workgroup"))
    t.append(V("varlen-L212", (212, 5), "VARLEN", H=2, causal=True))
    t.append(V("varlen-dh128-L50", (50, 49, 1), "VARLEN", dh=128, H=2))
    t.append(V("varlen-dh32-off5", (40, 0, 33), "VARLEN", dh=32, off0=5))

    # ---- ancestor-indexed caches -----------------------------------------------------------------------------------------------
    for tk in (1, 8):
        t.append(C(f"cached-dh32-tk{tk}", 7, tk, "FEW_KEYS", dh=32, bias_pad=3))
    t.append(C("cached-dh64-tk8", 7, 8, "FEW_KEYS", order="repeat_desc", out_slice=True))
    for tk in (9, 16):
        t += _family(C(f"cached-dh64-tk{tk}", 7, tk, "MFMA16_INDEXED", env=((*chain, "KEYS16"),)),
                     kinds=("peaked", "big_v", "tiny_v") if tk == 9 else (), splits=tk == 9)
        t.append(C(f"cached-dh32-tk{tk}", 7, tk, "KEYS16", dh=32, order="repeat_desc" if tk == 9 else "random"))
        t.append(C(f"cached-dh128-tk{tk}", 7, tk, "KEYS16", dh=128, H=2, bias_pad=5))
    t += _family(C("cached-dh32-tk12", 7, 12, "KEYS16", dh=32))
    t.append(C("cached-dh64-tk16-desc", 6, 16, "MFMA16_INDEXED", order="repeat_desc", bias_pad=4, out_slice=True))

    # ---- refusals (the status, not a fault) and empty calls --------------------------------------------------------------------
    t.append(P("refuse-tk257", 2, 1, 257, f"REFUSED({UNSUPPORTED})", H=2))
    t.append(P("refuse-dh132", 2, 4, 4, f"REFUSED({UNSUPPORTED})", dh=132, H=2))
    t.append(C("refuse-cached-tk17", 3, 17, f"REFUSED({UNSUPPORTED})"))
    t.append(V("refuse-varlen-L213", (213, 4), f"REFUSED({UNSUPPORTED})", H=2, note="213 x 193 x 4 B = 164 436 B > 160 KiB"))
    t.append(P("empty-padded", 0, 4, 4, "NONE"))
    t.append(V("empty-varlen", (), "NONE", max_len=8))
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "duplicate case names"


# ---- inputs ----------------------------------------------------------------------------------------------------------------

def _offsets(c):
    off = [c.off0]
    for n in c.lens:
        off.append(off[-1] + n)
    return off


def _mask(c, rng, nkv, tk):
    if not c.mask:
        return None
    m = np.ones((nkv, tk), np.int64)
    if c.mask == "prefix":
        for b in range(nkv):
            m[b, rng.integers(1, tk + 1):] = 0
        m[0] = 1                                           # one batch with every key real
    elif c.mask != "ones":
        m = (rng.random((nkv, tk)) < 0.5).astype(np.int64)
        blank = {"holes": 0, "blank16": 16, "blank32": 32, "blank64": 64}[c.mask]
        assert blank < tk, c.name
        m[:, :blank] = 0                                   # a whole leading block of keys masked: the running maximum starts at -1e9
        for b in range(nkv):
            m[b, rng.integers(blank, tk)] = 1              # at least one real key per kv batch
            if blank == 0:
                m[b, rng.integers(0, tk)] = 0              # and at least one hole
        if blank == 0 and tk > 1:
            m[:, 0] = 1 - m[:, 1]                          # never a prefix mask
            m[m.sum(1) == 0, 1] = 1
    return torch.from_numpy(m)


def make_inputs(c):
    """The f32 host tensors of a case: dict(q, k, v, bias, key_mask, off, key_rows); k / v of a cached case are the caches."""
    rng = np.random.default_rng(zlib.crc32(c.inputs_key.encode()))
    f = lambda *s: torch.zeros(s).copy_(torch.from_numpy(rng.standard_normal(s).astype(np.float32)))     # noqa: E731
    H, dh, hd = c.H, c.dh, c.H * c.dh
    d = dict(bias=None, key_mask=None, off=None, key_rows=None)
    if c.form == "padded":
        nkv = c.nb // c.kv_div
        d.update(q=f(c.nb, c.tq, hd), k=f(nkv, c.tk, hd), v=f(nkv, c.tk, hd), key_mask=_mask(c, rng, nkv, c.tk))
        brows, bcols, key_axis = c.q_pos0 + c.tq, c.tk, 1
    elif c.form == "kvpacked":
        off = _offsets(c)
        rows = off[-1] + 2
        d.update(q=f(c.nb * c.kv_div, 1, hd), k=f(rows, hd), v=f(rows, hd), off=off)
        brows, bcols, key_axis = c.q_pos0 + 1, c.tk or max(c.lens), 0
    elif c.form == "varlen":
        off = _offsets(c)
        rows = off[-1] + 2
        d.update(q=f(rows, hd), k=f(rows, hd), v=f(rows, hd), off=off)
        brows = bcols = c.max_len or max(c.lens)
        key_axis = 0
    else:
        rows, T = 11, c.tk + 2
        kr = rng.integers(0, rows, (c.nb, c.tk))
        if c.order == "repeat_desc":
            kr = np.sort(rng.integers(0, max(2, rows // 3), (c.nb, c.tk)), 1)[:, ::-1].copy()     # few distinct rows, descending
        if c.kind in ("peaked", "big_v") and c.tk > 1:
            kr[:, 1::2] = kr[:, :(c.tk // 2) * 2:2]         # pairs of positions from one cache row (ties / negated rows line up)
        d.update(q=f(c.nb, hd), k=f(rows, T, hd), v=f(rows, T, hd), key_rows=torch.from_numpy(kr.astype(np.int32)))
        brows, bcols, key_axis = c.q_pos0 + 1, c.tk, 1
    if c.bias:
        d["bias"] = f(H, brows, bcols + c.bias_pad)
    k, v = d["k"], d["v"]
    nkeys = k.shape[key_axis]
    pairs = [(j, j + 1) for j in range(0, nkeys - 1, 2)]
    if c.form in ("kvpacked", "varlen"):                     # pairs inside a sequence only
        pairs = [(a + j, a + j + 1) for a, b in zip(d["off"][:-1], d["off"][1:]) for j in range(0, b - a - 1, 2)]
    ev = torch.tensor([p[0] for p in pairs], dtype=torch.long)
    od = ev + 1
    if c.kind == "peaked":
        d["q"] = d["q"] * (30.0 / (math.sqrt(dh) * c.scale))
        if c.bias:
            d["bias"] = torch.from_numpy((-40.0 * rng.random(tuple(d["bias"].shape))).astype(np.float32))
        first = pairs[:1]                                    # two tied keys per row: the first two keys (of every sequence)
        if key_axis == 0:
            first = [(a, a + 1) for a, b in zip(d["off"][:-1], d["off"][1:]) if b - a >= 2]
        for a, b in first:
            tiny = 1e-6 * f(*k.select(key_axis, a).shape)
            k.select(key_axis, b).copy_(k.select(key_axis, a) + tiny)
        if c.bias and d["bias"].shape[2] > 1:
            d["bias"][:, :, 1] = d["bias"][:, :, 0] + 5e-4
    elif c.kind == "big_v":
        v.mul_(1e4)
        if len(pairs):
            v.index_copy_(key_axis, od, -v.index_select(key_axis, ev))
    elif c.kind == "tiny_v":
        v.mul_(1e-6)
    else:
        assert c.kind == "benign", c.kind
    return d


def reference(c, d, blocked=False):
    """fn(dtype, device) of tests/attn_ref64.py for the case; its rows are the rows `call` returns"""
    kw = dict(bias=d["bias"], causal=c.causal, scale=c.scale, blocked=blocked)
    if c.form == "padded":
        return R.padded(d["q"], d["k"], d["v"], c.H, kv_div=c.kv_div, q_pos0=c.q_pos0, key_mask=d["key_mask"], **kw)
    if c.form == "kvpacked":
        return R.packed_keys(d["q"], d["k"], d["v"], d["off"], c.H, kv_div=c.kv_div, q_pos0=c.q_pos0, **kw)
    if c.form == "varlen":
        return R.packed_self(d["q"], d["k"], d["v"], d["off"], c.H, **kw)
    return R.cached(d["q"], d["k"], d["v"], d["key_rows"], c.H, q_pos0=c.q_pos0, **kw)


# ---- the call ----------------------------------------------------------------------------------------------------------------

SENTINEL = -123456.75


def _nan_slices(parts, dev, live):
    """The [rows, w] tensors `parts` as column slices of one NaN-filled buffer (4 spare columns on either side); rows outside
    live = (first, last) are NaN too."""
    rows, w = parts[0].shape
    buf = torch.full((rows, len(parts) * w + 8), float("nan"), dtype=torch.float32, device=dev)
    out = []
    for i, p in enumerate(parts):
        s = buf[:, 4 + i * w:4 + (i + 1) * w]
        s[live[0]:live[1]] = p[live[0]:live[1]].to(dev)
        out.append(s)
    return out


def _hand_over(mask, how, dev):
    """The key mask as a caller may pass it: ops.attention converts anything but a contiguous int64 device tensor, and the
    converted copy has to outlive the launch."""
    if mask is None or how == "host":
        return mask
    mask = mask.to(dev)
    if how == "bool":
        return mask.bool()
    if how == "strided32":
        wide = torch.zeros((mask.shape[0], 2 * mask.shape[1]), dtype=torch.int32, device=dev)
        wide[:, ::2] = mask
        return wide[:, ::2]
    assert how == "", how
    return mask


def call(c, d, dev, ops, route_only=False):
    """Run the case through mevi_amd.ops on `dev`.  The arguments are built ONCE: ops.attention*_route is asked about the very
    tensors (and out= slice) that are then launched, so the route is that of this launch by construction.  route_only: stop
    after the question (host tensors will do) and return (route, None).
    -> (context as float64 [rows of the reference, H*dh], info) with info = dict(route, exp: the image's exponent or None,
    untouched: whether every byte outside an out= slice kept its sentinel, or None)."""
    H, hd = c.H, c.H * c.dh
    to = lambda x: None if x is None else x.to(dev)     # noqa: E731
    kw = dict(bias=to(d["bias"]), causal=c.causal, scale=c.scale)
    live = None
    if c.form == "padded":
        kv = torch.cat([d["k"], d["v"]], -1).to(dev)       # K | V side by side, as the caches and the fused projections hold them
        args = (to(d["q"]), kv[..., :hd], kv[..., hd:], H)
        kw.update(kv_div=c.kv_div, q_pos0=c.q_pos0, key_mask=_hand_over(d["key_mask"], c.mask_as, dev))
        fn, rt, shape = ops.attention, ops.attention_route, (c.nb, c.tq, hd)
    elif c.form == "kvpacked":
        off = d["off"]
        k, v = _nan_slices([d["k"], d["v"]], dev, (off[0], off[-1]))
        args = (to(d["q"]), k, v, H)
        kw.update(kv_div=c.kv_div, q_pos0=c.q_pos0, kv_off=torch.tensor(off, dtype=torch.int64, device=dev),
                  kv_longest=c.tk or max(c.lens))
        fn, rt, shape = ops.attention, ops.attention_route, (c.nb * c.kv_div, 1, hd)
    elif c.form == "varlen":
        off = d["off"]
        live = (off[0], off[-1])
        q, k, v = _nan_slices([d["q"], d["k"], d["v"]], dev, live)
        args = (q, k, v, torch.tensor(off, dtype=torch.int64, device=dev), c.max_len or max(c.lens, default=1), H)
        fn, rt, shape = ops.attention_varlen, ops.attention_varlen_route, (d["q"].shape[0], hd)
    else:
        kv = torch.cat([d["k"], d["v"]], -1).to(dev)
        args = (to(d["q"]), kv[..., :hd], kv[..., hd:], to(d["key_rows"]), H)
        kw.update(q_pos0=c.q_pos0)
        fn, rt, shape = ops.attention_cached, ops.attention_cached_route, (c.nb, hd)
    wide = None
    if c.split:
        vmax = float(d["v"].abs().max()) if d["v"].numel() else 1.0
        kw["split_bound"] = vmax * (37.0 if c.split == "loose" else 1.0)
    elif c.out_slice:
        wide = torch.full((*shape[:-1], hd + 8), SENTINEL, dtype=torch.float32, device=dev)
        kw["out"] = wide[..., 4:4 + hd]
    route = rt(*args, **kw)
    if route_only:
        return route, None
    got = fn(*args, **kw)
    info = dict(route=route, exp=None, untouched=None)
    if c.split:
        kp = got.img.shape[1] // 2
        e = got.exp.to(torch.float64)
        assert (e == e[:1]).all()
        h = got.img.view(torch.float16).to(torch.float64)
        got = ((h[:, :hd] + h[:, kp:kp + hd]) * torch.pow(2.0, -e)[:, None]).reshape(shape)
        info["exp"] = int(e[0]) if e.numel() else 0
    if wide is not None:
        ref = torch.full_like(wide, SENTINEL)
        ref[..., 4:4 + hd] = wide[..., 4:4 + hd]
        if live is not None:                               # rows outside the sequences are nobody's
            ref[:live[0], 4:4 + hd] = SENTINEL
            ref[live[1]:, 4:4 + hd] = SENTINEL
        info["untouched"] = bool(torch.equal(ref.view(torch.int32), wide.view(torch.int32)))
    got = got.double()
    if live is not None:
        got = got[live[0]:live[1]]
    return got.reshape(-1, hd), info


# ---- the bar -----------------------------------------------------------------------------------------------------------------

FACTOR = 4.0


def errors(got, ref64, ref32):
    got, ref64, ref32 = got.double().cpu().reshape(-1), ref64.double().cpu().reshape(-1), ref32.double().cpu().reshape(-1)
    return (got - ref64).abs().max().item(), (ref32 - ref64).abs().max().item(), ref64.abs().max().item()


def bar(e_32, max_ref, exp=None):
    """f64_bar's  factor * e_32 + 2^-22 max |ref64|, plus -- for a context written as the split image with exponent `exp` -- the
    image's own quantisation 2^(15 - exp) 2^-21 (22 significant bits below the image's 2^15; the term of
    test_ops_gpu.py::test_attention_context_written_as_split_image)."""
    return FACTOR * e_32 + 2.0 ** -22 * max_ref + (2.0 ** (15 - exp) * 2.0 ** -21 if exp is not None else 0.0)


_BLOCKED = {}


def measure(c, dev, ops, hip, refs):
    """Run a case and hold it against float64: dict(case, route, e_hip, e_32, max_ref, bar, exp, untouched, ok) plus the tensors
    got / ref64 / ref32.  `refs` is f64_bar.refs (one float64 and one float32 restatement per set of inputs, shared).

    The bar is f64_bar's (see `bar`).  attention_h16_kernel alone, whose products are f16 pairs, keeps the formula of
    test_ops_gpu.py::test_split_precision_passage_attention_scales_its_operands with both errors taken against float64:
    e_hip <= 1.5 e_f32_kernel + 2^-20 max |V|, e_f32_kernel being the f32 matrix-core kernel's error on the same inputs (that
    kernel is then held to the usual bar as a case of its own).  The matrix-core routes also record e_32_blocked, the error
    of the restatement with library matmuls in float32 (see attn_ref64._attend).  For attention_mfma_kernel that IS e_32 (the
    chain order was introduced for kernels whose error it explains; nothing ties the 32 x 32 x 2 kernel to it, and it passes
    without); for the 16 x 16 kernels it is information beside the chain's e_32."""
    d = make_inputs(c)
    got, info = call(c, d, dev, ops)
    route = hip.attn_route_name(info["route"])
    ref64, ref32 = refs(c.inputs_key, reference(c, d))
    e_hip, e_32, max_ref = errors(got, ref64, ref32)
    m = dict(case=c.name, route=route, e_hip=e_hip, e_32=e_32, max_ref=max_ref, exp=info["exp"], untouched=info["untouched"],
             finite=bool(torch.isfinite(got).all()))
    if route == "H16":
        twin = dataclasses.replace(c, split="", out_slice=False)
        g32, _ = call(twin, d, dev, ops)
        m["e_f32_kernel"] = errors(g32, ref64, ref32)[0]
        m["bar"] = 1.5 * m["e_f32_kernel"] + 2.0 ** -20 * float(d["v"].abs().max())
    else:
        m["bar"] = bar(e_32, max_ref, info["exp"])
    if route.startswith("MFMA") or route == "H16":      # the matrix-core kernels: what a blocked f32 matmul reference says
        if c.inputs_key not in _BLOCKED:
            _BLOCKED[c.inputs_key] = reference(c, d, blocked=True)(torch.float32, "cpu")
        m["e_32_blocked"] = errors(got, ref64, _BLOCKED[c.inputs_key])[1]
    if route == "MFMA":      # no chain twin, no miss to explain: the plain matmul restatement is its yardstick
        m["e_32_chain"], ref32 = e_32, _BLOCKED[c.inputs_key]
        m["e_32"] = e_32 = m["e_32_blocked"]
        m["bar"] = bar(e_32, max_ref, info["exp"])
    m["ok"] = m["finite"] and e_hip <= m["bar"] and info["untouched"] is not False
    m.update(got=got, ref64=ref64.reshape(got.shape), ref32=ref32.reshape(got.shape))
    return m
