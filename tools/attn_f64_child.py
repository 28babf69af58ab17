"""Helper of tests/test_attn_f64_gpu.py and tests/test_attn_cases_cpu.py: the attention cases whose kernel changes under an
environment switch, run in a process of their own (MEVI_ATTN_SHORT, MEVI_ATTN_FEW_KEYS and MEVI_ATTN_PASSAGE are read once
per process).

    python tools/attn_f64_child.py MEVI_ATTN_SHORT chain [--routes-only]

sets the switch before the library loads, runs every case of tests/attn_cases.py that names (switch, value) and prints one
JSON line per case: the route taken, and -- unless --routes-only, which needs no GPU -- e_hip, e_32 and the bar against the
float64 restatement.  The parent asserts; the exit status only says that every case ran."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    switch, value = argv[0], argv[1]
    routes_only = "--routes-only" in argv[2:]
    os.environ[switch] = value
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import attn_cases as A
    import f64_bar
    from mevi_amd import hip, ops

    for c in A.CASES:
        if not any(e[:2] == (switch, value) for e in c.env):
            continue
        if routes_only:
            route = hip.attn_route_name(A.call(c, A.make_inputs(c), "cpu", ops, route_only=True)[0])
            print(json.dumps({"case": c.name, "route": route}), flush=True)
            continue
        m = A.measure(c, "cuda", ops, hip, f64_bar.refs)
        print(json.dumps({k: v for k, v in m.items() if k not in ("got", "ref64", "ref32")}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
