"""The route functions of the long attention calls (include/mevi_hip_attn_long.h) without a GPU: pure host arithmetic on
fake aligned addresses through ctypes -- which kernel a shape takes, every refusal with its status and the word that names
the argument, the accepted key counts on either side of the old 256-key limit, and the old entry point's unchanged refusal."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 1 << 20                    # fake 16-byte aligned device addresses (never read)
Q, K, V, OUT, BIAS, MASK, OFF = (BASE * i for i in range(1, 8))


@pytest.fixture(scope="module")
def hip():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip


def padded(hip, S=300, tq=None, nb=3, H=2, dh=64, kv_div=1, q=Q, k=K, v=V, out=OUT, bias=None, brows=0, bld=0, q_pos0=0,
           kv_off=None, strides=None):
    """mevi_attention_long_route for contiguous [nb, tq, H*dh] / [nb / kv_div, S, H*dh] operands (strides: overrides by name)"""
    tq = S if tq is None else tq
    hd = H * dh
    st = dict(q_bs=tq * hd, q_ts=hd, k_bs=S * hd, k_ts=hd, v_bs=S * hd, v_ts=hd, o_bs=tq * hd, o_ts=hd)
    st.update(strides or {})
    return hip.lib().mevi_attention_long_route(q, st["q_bs"], st["q_ts"], k, st["k_bs"], st["k_ts"], v, st["v_bs"], st["v_ts"], out,
                                               st["o_bs"], st["o_ts"], nb, tq, S, H, dh, kv_div, bias, brows, bld, q_pos0, None, 0,
                                               1.0, kv_off)


def varlen(hip, max_len=300, nseq=3, H=2, dh=64, q=Q, k=K, v=V, out=OUT, off=OFF, bias=None, brows=0, bld=0, ts=None, o_ts=None):
    hd = H * dh
    ts = hd if ts is None else ts
    return hip.lib().mevi_attention_long_varlen_route(q, ts, k, ts, v, ts, out, hd if o_ts is None else o_ts, off, nseq, max_len, H,
                                                      dh, bias, brows, bld, 0, 1.0)


def message(hip):
    return hip.lib().mevi_last_error().decode()


def test_the_header_names_the_routes_and_the_limit(hip):
    text = open(os.path.join(ROOT, "include", "mevi_hip_attn_long.h")).read()
    assert '#include "mevi_hip_attn_long.h"' in open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"MEVI_ATTN_ROUTE_([A-Z0-9_]+) = (\d+)", text)}
    assert enum == hip.ATTN_LONG_ROUTES == {"LONG_MFMA": 13, "LONG_ROWS": 14}
    assert not set(enum.values()) & set(hip.ATTN_ROUTES.values())
    assert int(re.search(r"#define MEVI_ATTN_LONG_MAX_KEYS (\d+)", text).group(1)) == hip.ATTN_LONG_MAX_KEYS == 2048
    assert hip.attn_route_name(13) == "LONG_MFMA" and hip.attn_route_name(14) == "LONG_ROWS"
    declared = sorted(set(re.findall(r"\b(mevi_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert declared == hip.exported_symbols("mevi_hip_attn_long.h") and len(declared) == 4
    assert all(hasattr(hip.lib(), n) for n in declared) and not set(declared) & set(hip.exported_symbols())


def test_self_attention_on_64_wide_heads_takes_the_matrix_cores(hip):
    name = hip.attn_route_name
    for S in (1, 128, 129, 256, 257, 513, 2048):
        assert name(padded(hip, S)) == "LONG_MFMA", S
        assert name(varlen(hip, S)) == "LONG_MFMA", S
    assert name(padded(hip, 300, bias=BIAS, brows=300, bld=300)) == "LONG_MFMA"
    assert name(padded(hip, 300, bias=BIAS, brows=310, bld=301, q_pos0=10)) == "LONG_MFMA"      # an odd table width is fine


@pytest.mark.parametrize("why,kw", [
    ("dh8", dict(dh=8)), ("dh96", dict(dh=96)), ("dh128", dict(dh=128)),
    ("tq!=tk", dict(tq=1)), ("tq5", dict(tq=5, q_pos0=295)),
    ("kv_div", dict(tq=1, nb=6, kv_div=3)), ("kv_div-self", dict(nb=6, kv_div=3)),
    ("kv_off", dict(tq=1, kv_off=OFF)), ("kv_off-self", dict(kv_off=OFF)),
    ("q+4", dict(q=Q + 4)), ("k+4", dict(k=K + 4)), ("v+4", dict(v=V + 4)), ("out+8", dict(out=OUT + 8)),
    ("v_ts", dict(strides=dict(v_ts=130))), ("v_bs", dict(strides=dict(v_bs=300 * 128 + 2))),
    ("o_ts", dict(strides=dict(o_ts=129))), ("o_bs", dict(strides=dict(o_bs=300 * 128 + 1))),
])
def test_each_of_these_alone_takes_the_rows_kernel(hip, why, kw):
    assert hip.attn_route_name(padded(hip, 300, **kw)) == "LONG_ROWS", why


def test_packed_sequences_off_the_matrix_core_shape_take_the_rows_kernel(hip):
    name = hip.attn_route_name
    for kw in (dict(dh=8), dict(dh=96), dict(dh=128), dict(q=Q + 4), dict(out=OUT + 4), dict(o_ts=129)):
        assert name(varlen(hip, 300, **kw)) == "LONG_ROWS", kw


def test_key_counts_on_both_sides_of_the_old_limit_are_accepted(hip):
    for tk in (1, 256, 257, 2048):
        for kw in (dict(), dict(tq=1), dict(dh=8), dict(tq=1, nb=6, kv_div=3)):
            assert padded(hip, tk, **kw) in (13, 14), (tk, kw)
        assert varlen(hip, tk) == 13 and varlen(hip, tk, dh=96) == 14


@pytest.mark.parametrize("status,word,call", [
    (-2, "tk=2049", lambda h: padded(h, 2049)),
    (-2, "tk=2049", lambda h: padded(h, 2049, tq=1, dh=8)),
    (-2, "dh=132", lambda h: padded(h, 300, dh=132)),
    (-2, "max_len=2049", lambda h: varlen(h, 2049)),
    (-2, "dh=132", lambda h: varlen(h, 300, dh=132)),
    (-1, "null pointer", lambda h: padded(h, 300, q=None)),
    (-1, "null pointer", lambda h: padded(h, 300, k=None)),
    (-1, "null pointer", lambda h: padded(h, 300, v=None)),
    (-1, "null pointer", lambda h: padded(h, 300, out=None)),
    (-1, "seq_off", lambda h: varlen(h, 300, off=None)),
    (-1, "strides", lambda h: padded(h, 300, strides=dict(q_ts=130))),
    (-1, "strides", lambda h: padded(h, 300, strides=dict(k_ts=129))),
    (-1, "strides", lambda h: padded(h, 300, strides=dict(k_bs=300 * 128 + 2))),
    (-1, "strides", lambda h: padded(h, 300, dh=6)),
    (-1, "negative stride", lambda h: padded(h, 300, strides=dict(v_ts=-128))),
    (-1, "strides", lambda h: varlen(h, 300, ts=130)),
    (-1, "bias table too small", lambda h: padded(h, 300, bias=BIAS, brows=299, bld=300)),
    (-1, "bias table too small", lambda h: padded(h, 300, bias=BIAS, brows=300, bld=299)),
    (-1, "bias table too small", lambda h: padded(h, 300, tq=5, q_pos0=296, bias=BIAS, brows=300, bld=300)),
    (-1, "bias table too small", lambda h: varlen(h, 300, bias=BIAS, brows=300, bld=299)),
    (-1, "bad shape", lambda h: padded(h, 300, kv_div=0)),
    (-1, "bad shape", lambda h: varlen(h, 0)),
])
def test_refusals_come_with_their_status_and_their_word(hip, status, word, call):
    assert call(hip) == status
    assert word in message(hip), message(hip)


def test_empty_calls_launch_nothing(hip):
    assert padded(hip, 300, nb=0) == 0 and padded(hip, 300, nb=0, q=None, out=None) == 0
    assert varlen(hip, 300, nseq=0) == 0 and varlen(hip, 300, nseq=0, off=None) == 0
    assert hip.attn_route_name(0) == "NONE"
    # ... but a shape outside the envelope is refused even when empty, as by the existing calls
    assert padded(hip, 2049, nb=0) == -2


def test_the_existing_entry_points_keep_their_envelope(hip):
    hd, S = 128, 257
    r = hip.lib().mevi_attention_route(Q, S * hd, hd, K, S * hd, hd, V, S * hd, hd, OUT, S * hd, hd, 3, S, S, 2, 64, 1, None, 0, 0,
                                       0, None, 0, 1.0, None, None, 0, 0)
    assert hip.attn_route_name(r) == "REFUSED(-2)" and "tk=257 > 256" in message(hip)
    hd = 3 * 64
    r = hip.lib().mevi_attention_varlen_route(Q, hd, K, hd, V, hd, OUT, hd, OFF, 3, 213, 3, 64, None, 0, 0, 0, 1.0, None, 0, 0)
    assert hip.attn_route_name(r) == "REFUSED(-2)"
    assert hip.attn_route_name(hip.lib().mevi_attention_route(Q, 256 * hd, hd, K, 256 * hd, hd, V, 256 * hd, hd, OUT, 256 * hd, hd, 3,
                                                              256, 256, 3, 64, 1, None, 0, 0, 0, None, 0, 1.0, None, None, 0, 0)) == "GENERIC"
