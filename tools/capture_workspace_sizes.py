"""Record what the dense search's five `*_bytes` entry points return over a grid of shapes, as
tests/golden/ip_workspace_bytes.json (compared entry by entry by tests/test_abi_cpu.py).

The footprints are behaviour (a corpus index is tens of GB), so the file pins them to the commit BEFORE a change of the
host code: build that commit's library and point --lib at it, never at the branch under test.

    python tools/capture_workspace_sizes.py --lib <parent build>/libmevi_hip.so --source "parent commit <sha>"

Pure host arithmetic: no GPU needed.
"""
import argparse
import ctypes
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NQ = [0, 1, 31, 32, 33, 64, 65, 128, 129, 1024, 1025, 6980]
DIM = [4, 36, 64, 100, 128, 160, 256, 768, 896, 960, 1024, 1028]
K = [1, 10, 32, 100, 1000, 1323, 1365, 4096, 4097]
ND = [0, 1, 255, 256, 257, 65536, 8841823]

SEARCH = ["mevi_ip_topk_workspace_bytes", "mevi_ip_topk_indexed_workspace_bytes", "mevi_ip_topk_indexed8_workspace_bytes"]
INDEX = ["mevi_ip_index_bytes", "mevi_ip_index8_bytes"]


def compute(L, nq=NQ, dim=DIM, k=K, nd=ND):
    """{entry point: flat list}; search sizes in (nq, dim, k) order, index sizes in (nd, dim) order, last axis fastest."""
    out = {}
    for name in SEARCH:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int64] * 3
        out[name] = [fn(a, b, c) for a in nq for b in dim for c in k]
    for name in INDEX:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int64] * 2
        out[name] = [fn(a, b) for a in nd for b in dim]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", required=True, help="libmevi_hip.so built from the commit the sizes are pinned to")
    ap.add_argument("--source", required=True, help='what --lib was built from, e.g. "parent commit 5f9044a"')
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ip_workspace_bytes.json"))
    a = ap.parse_args()
    rec = {"header": f"written by tools/capture_workspace_sizes.py from a build of {a.source} (never from the branch under test); "
                     "search sizes in (nq, dim, k) order, index sizes in (nd, dim) order, last axis fastest",
           "nq": NQ, "dim": DIM, "k": K, "nd": ND}
    rec.update(compute(ctypes.CDLL(os.path.abspath(a.lib))))
    with open(a.out, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print(a.out, {n: len(v) for n, v in rec.items() if n.startswith("mevi_")})


if __name__ == "__main__":
    main()
