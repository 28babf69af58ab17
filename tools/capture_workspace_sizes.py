"""Record what the dense search's five `*_bytes` entry points return over a grid of shapes, as
tests/golden/ip_workspace_bytes.json, or (--what scan) what the eight `mevi_{ivf,sq,ivfpq,pqfs}_scan_{workspace_bytes,query_tile}`
entry points of the list scans return, as tests/golden/scan_workspace_sizes.json (both compared entry by entry by
tests/test_abi_cpu.py).

The footprints are behaviour (a corpus index is tens of GB), so the file pins them to the commit BEFORE a change of the
host code: build that commit's library and point --lib at it, never at the branch under test.

    python tools/capture_workspace_sizes.py [--what scan] --lib <parent build>/libmevi_hip.so --source "parent commit <sha>"

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


# The list scans: (nq, nprobe, k, dim, *format, nlist, max_list_len).  The grid is SCAN_FORMATS x SCAN_NQ x SCAN_NPROBE x SCAN_LEN
# (last axis fastest) at k = SCAN_K and nlist = SCAN_NLIST: nq across the 4096 queries of a tile, the candidate cap of 2 GiB at
# nprobe 256 (2097152 rows inside, 2097156 outside) and tiling by it from nprobe 16 x 200000 rows on, the 128 MiB table cap of
# IVF-PQ (2048 and 1365 queries), m at both ends.  SCAN_EDGES: the last value inside and the first outside every other bound.
SCAN_NQ = [0, 1, 33, 4096, 4097, 6980]
SCAN_NPROBE = [1, 16, 256, 257]
SCAN_LEN = [-1, 0, 1000, 200000, 2097152, 2097156]
SCAN_K, SCAN_NLIST = 10, 100
SCAN_FORMATS = {"ivf": [(768,)], "sq": [(768, 8), (64, 4)], "ivfpq": [(16, 4, 16), (768, 64, 256), (768, 96, 256)],
                "pqfs": [(32, 8), (768, 96)]}
SCAN_EDGES = {
    "ivf": [(8, 2, 0, 64, 8, 1000), (8, 2, 4096, 64, 8, 1000), (8, 2, 4097, 64, 8, 1000), (8, 2, 10, 64, 0, 1000),
            (8, 2, 10, 64, 262144, 1000), (8, 2, 10, 64, 262145, 1000), (8, 0, 10, 64, 8, 1000), (8, 2, 10, 0, 8, 1000),
            (8, 2, 10, 4, 8, 1000), (8, 2, 10, 66, 8, 1000)],
    "sq": [(8, 2, 0, 64, 8, 8, 1000), (8, 2, 4096, 64, 8, 8, 1000), (8, 2, 4097, 64, 8, 8, 1000), (8, 2, 10, 64, 8, 0, 1000),
           (8, 2, 10, 64, 8, 262144, 1000), (8, 2, 10, 64, 8, 262145, 1000), (8, 0, 10, 64, 8, 8, 1000), (8, 2, 10, 64, 6, 8, 1000),
           (8, 2, 10, 64, 16, 8, 1000), (8, 2, 10, 4, 8, 8, 1000), (8, 2, 10, 4, 4, 8, 1000), (8, 2, 10, 20, 4, 8, 1000),
           (8, 2, 10, 4096, 8, 8, 1000), (8, 2, 10, 4100, 8, 8, 1000)],
    "ivfpq": [(8, 2, 0, 64, 16, 256, 8, 1000), (8, 2, 4096, 64, 16, 256, 8, 1000), (8, 2, 4097, 64, 16, 256, 8, 1000),
              (8, 2, 10, 64, 16, 256, 0, 1000), (8, 2, 10, 64, 16, 256, 262144, 1000), (8, 2, 10, 64, 16, 256, 262145, 1000),
              (8, 0, 10, 64, 16, 256, 8, 1000), (8, 2, 10, 64, 0, 256, 8, 1000), (8, 2, 10, 64, 2, 256, 8, 1000),
              (8, 2, 10, 72, 18, 256, 8, 1000), (8, 2, 10, 800, 100, 16, 8, 1000), (8, 2, 10, 64, 16, 0, 8, 1000),
              (8, 2, 10, 64, 16, 1, 8, 1000), (8, 2, 10, 64, 16, 257, 8, 1000), (8, 2, 10, 68, 16, 256, 8, 1000),
              (8, 2, 10, 96, 16, 256, 8, 1000)],
    "pqfs": [(8, 2, 0, 64, 16, 8, 1000), (8, 2, 4096, 64, 16, 8, 1000), (8, 2, 4097, 64, 16, 8, 1000), (8, 2, 10, 64, 16, 0, 1000),
             (8, 2, 10, 64, 16, 262144, 1000), (8, 2, 10, 64, 16, 262145, 1000), (8, 0, 10, 64, 16, 8, 1000), (8, 2, 10, 64, 4, 8, 1000),
             (8, 2, 10, 48, 12, 8, 1000), (8, 2, 10, 256, 64, 8, 1000), (8, 2, 10, 288, 72, 8, 1000), (8, 2, 10, 416, 104, 8, 1000),
             (8, 2, 10, 68, 16, 8, 1000), (8, 2, 10, 96, 16, 8, 1000)],
}


def scan_shapes(family):
    """The family's shapes: its grid, then its edges."""
    grid = [(nq, nprobe, SCAN_K, fmt[0], *fmt[1:], SCAN_NLIST, longest) for fmt in SCAN_FORMATS[family] for nq in SCAN_NQ
            for nprobe in SCAN_NPROBE for longest in SCAN_LEN]
    return grid + SCAN_EDGES[family]


def compute_scan(L):
    """{entry point: flat list over scan_shapes(family)} for the eight entry points."""
    out = {}
    for family in SCAN_FORMATS:
        for what, restype in (("workspace_bytes", ctypes.c_size_t), ("query_tile", ctypes.c_int64)):
            fn = getattr(L, f"mevi_{family}_scan_{what}")
            shapes = scan_shapes(family)
            fn.restype, fn.argtypes = restype, [ctypes.c_int64] * len(shapes[0])
            out[f"mevi_{family}_scan_{what}"] = [fn(*s) for s in shapes]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", required=True, help="libmevi_hip.so built from the commit the sizes are pinned to")
    ap.add_argument("--source", required=True, help='what --lib was built from, e.g. "parent commit 5f9044a"')
    ap.add_argument("--what", choices=["ip", "scan"], default="ip", help="the dense search's sizes, or the list scans'")
    ap.add_argument("--out", help="default: tests/golden/ip_workspace_bytes.json, or scan_workspace_sizes.json with --what scan")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "tests", "golden", "ip_workspace_bytes.json" if a.what == "ip" else "scan_workspace_sizes.json")
    L = ctypes.CDLL(os.path.abspath(a.lib))
    if a.what == "scan":
        rec = {"header": f"written by tools/capture_workspace_sizes.py --what scan from a build of {a.source} (never from the branch "
                         "under test); per family the grid formats x nq x nprobe x max_list_len (last axis fastest) at k and nlist, "
                         "then the edges; arguments in the entry point's order",
               "nq": SCAN_NQ, "nprobe": SCAN_NPROBE, "max_list_len": SCAN_LEN, "k": SCAN_K, "nlist": SCAN_NLIST,
               "formats": {f: [list(t) for t in v] for f, v in SCAN_FORMATS.items()},
               "edges": {f: [list(t) for t in v] for f, v in SCAN_EDGES.items()}}
        rec.update(compute_scan(L))
    else:
        rec = {"header": f"written by tools/capture_workspace_sizes.py from a build of {a.source} (never from the branch under test); "
                         "search sizes in (nq, dim, k) order, index sizes in (nd, dim) order, last axis fastest",
               "nq": NQ, "dim": DIM, "k": K, "nd": ND}
        rec.update(compute(L))
    with open(a.out, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print(a.out, {n: len(v) for n, v in rec.items() if n.startswith("mevi_")})


if __name__ == "__main__":
    main()
