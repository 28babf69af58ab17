"""Every attention kernel of mevi_amd/csrc/t5_ops.hip against float64, at its dispatch edges.

Each case of tests/attn_cases.py names the kernel it must take; the test asks the launcher's own decision function
(ops.attention*_route) that it does, runs it, and holds the context to the project's float64 bar (tests/f64_bar.py):

    e_hip <= 4 e_32 + 2^-22 max |ref64|                 e_hip = max |hip - ref64|,  e_32 = max |ref32 - ref64|

ref64 / ref32 being tests/attn_ref64.py in float64 on the GPU and in float32 on the host, over EVERY output element (no row
of any case is fully masked).  ref32 sums in the kernels' chain order; for attention_mfma_kernel it is the plain matmul form.  A context written as the split image adds the image's quantisation 2^(15 - e) 2^-21;
attention_h16_kernel keeps the bar of test_ops_gpu.py::test_split_precision_passage_attention_scales_its_operands
(1.5 e_f32kernel + 2^-20 max |V|), both errors against float64.  The measured e_hip, e_32 and bar of every case go into the
junit properties.  Cases that name an environment switch run once more under it in a fresh child process
(tools/attn_f64_child.py), which is how the scalar-chain kernels behind MEVI_ATTN_SHORT=chain, the direct few-keys kernel at
staged shapes and the f32 passage kernel with image output are reached."""
import json
import os
import subprocess
import sys

import pytest
import torch

import attn_cases as A
import f64_bar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SHOWN = ("route", "e_hip", "e_32", "bar", "max_ref", "exp", "untouched", "e_f32_kernel", "e_32_blocked", "e_32_chain")


@pytest.mark.parametrize("case", [c for c in A.CASES if not c.refused], ids=lambda c: c.name)
def test_attention_against_float64(cuda, case, record_property):
    from mevi_amd import hip, ops

    m = A.measure(case, cuda, ops, hip, f64_bar.refs)
    record_property(case.name, {k: m[k] for k in _SHOWN if k in m})
    assert m["route"] == case.route
    assert m["finite"]
    if case.out_slice:
        assert m["untouched"] is True, "bytes outside the out= slice were written"
    if m["exp"] is None and m["route"] != "H16":
        f64_bar.check(case.name + "/f64_bar", m["got"], m["ref64"], m["ref32"], None, record_property, factor=A.FACTOR)
    assert m["e_hip"] <= m["bar"], (case.name, m["e_hip"], m["e_32"], m["bar"])


@pytest.mark.parametrize("case", [c for c in A.CASES if c.refused], ids=lambda c: c.name)
def test_refusals_and_empty_calls_return_a_status(cuda, case):
    """Outside the envelope the call returns the status its route function names, before any launch; an empty call launches
    nothing and returns an empty context."""
    from mevi_amd import hip, ops

    d = A.make_inputs(case)
    route = hip.attn_route_name(A.call(case, d, cuda, ops, route_only=True)[0])
    assert route == case.route
    if case.route == "NONE":
        got, _ = A.call(case, d, cuda, ops)
        assert got.numel() == 0
    else:
        status = case.route[len("REFUSED("):-1]
        with pytest.raises(hip.MeviHipError, match=f"status {status}:"):
            A.call(case, d, cuda, ops)
    torch.cuda.synchronize()


@pytest.mark.parametrize("switch,value", [("MEVI_ATTN_SHORT", "chain"), ("MEVI_ATTN_FEW_KEYS", "direct"), ("MEVI_ATTN_PASSAGE", "f32")])
def test_attention_against_float64_under_a_switch(cuda, switch, value, record_property):
    want = {c.name: e[2] for c in A.CASES for e in c.env if e[:2] == (switch, value)}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "attn_f64_child.py"), switch, value], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    got = {j["case"]: j for j in map(json.loads, (l for l in r.stdout.splitlines() if l.startswith("{")))}
    assert sorted(got) == sorted(want)
    for name, m in got.items():
        record_property(f"{name}[{switch}={value}]", {k: m[k] for k in _SHOWN if k in m})
    for name, m in got.items():
        assert m["route"] == want[name], name
        assert m["finite"] and m["e_hip"] <= m["bar"], (name, m["e_hip"], m["e_32"], m["bar"])
