"""The float64 bar shared by tests/test_t5_f64_gpu.py and tests/test_bert_f64_gpu.py (TEST INFRASTRUCTURE ONLY):

    e_hip <= factor * e_32 + 2^-22 max |ref64|        (factor 4; derivation in test_t5_f64_gpu.py's docstring)

with e_hip = max |hip - ref64| and e_32 = max |ref32 - ref64| over the positions `valid`; ref64 / ref32 are one dtype-generic
restatement run in float64 (on the GPU) and in float32 (on the host) on the same f32 inputs."""
import torch

_CACHE = {}


def check(name, hip, ref64, ref32, valid, record_property, factor=4.0):
    """The per-block bar of the module docstring over the rows / positions `valid` (bool, None: all)."""
    hip, ref64, ref32 = hip.double().cpu(), ref64.double().cpu(), ref32.double().cpu()
    if valid is not None:
        hip, ref64, ref32 = hip[valid], ref64[valid], ref32[valid]
    assert torch.isfinite(hip).all(), name
    e_hip = (hip - ref64).abs().max().item()
    e_32 = (ref32 - ref64).abs().max().item()
    bar = factor * e_32 + 2.0 ** -22 * ref64.abs().max().item()
    record_property(name, {"e_hip": e_hip, "e_32": e_32, "bar": bar, "max_ref": ref64.abs().max().item()})
    print(f"{name}: e_hip {e_hip:.3e}  e_32 {e_32:.3e}  bar {bar:.3e}  max {ref64.abs().max().item():.3e}")
    assert e_hip <= bar, (name, e_hip, e_32, bar)
    return e_hip, e_32


def refs(key, fn):
    """(ref64 on the GPU, ref32 on the host) of fn(dtype, device): computed once per key, shared by the tests that need it."""
    if key not in _CACHE:
        _CACHE[key] = (fn(torch.float64, "cuda"), fn(torch.float32, "cpu"))
    return _CACHE[key]
