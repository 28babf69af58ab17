"""CPU-side checks: the C-ABI library loads and exports every symbol include/mevi_hip.h
declares; host-only entry points behave; the product path refuses to run without a GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "mevi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mevi_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    L = hip.lib()
    declared = _declared_symbols()
    assert declared, "no declarations parsed from include/mevi_hip.h"
    for name in declared:
        assert hasattr(L, name), f"{name} declared in mevi_hip.h but not exported"
    assert sorted(hip.exported_symbols()) == declared
    assert L.mevi_abi_version() == 1


def test_workspace_queries_are_pure_host_arithmetic():
    from mevi_amd import hip

    L = hip.lib()
    a = L.mevi_ip_topk_workspace_bytes(6980, 768, 1000)
    assert a > 2 * 6980 * 4096 * 8
    assert L.mevi_ip_topk_workspace_bytes(6980, 768, 5000) == 0   # k > 4096 unsupported
    assert L.mevi_ip_topk_workspace_bytes(0, 768, 10) == 0
    # the image width the host computes without a foreign call is the library's
    from mevi_amd import ops

    for k in list(range(1, 300)) + [767, 768, 769, 2048, 3072, 3073, 100000]:
        assert ops.split_kp(k) == L.mevi_split_kp(k), k


def test_workspace_and_index_sizes_are_those_of_the_recorded_commit():
    """The five `*_bytes` entry points of the dense search over a grid of shapes (zeros for unsupported shapes included)
    against tests/golden/ip_workspace_bytes.json, recorded by tools/capture_workspace_sizes.py from the commit before the
    host code's layouts were rewritten: the footprint of a search and of an index is behaviour.  The same for the workspace bytes
    and the query tile of the four list scans (tests/golden/scan_workspace_sizes.json)."""
    import json

    from mevi_amd import hip

    with open(os.path.join(ROOT, "tests", "golden", "ip_workspace_bytes.json")) as f:
        rec = json.load(f)
    assert "parent commit" in rec["header"]
    nq, dim, k, nd = rec["nq"], rec["dim"], rec["k"], rec["nd"]
    assert nq == [0, 1, 31, 32, 33, 64, 65, 128, 129, 1024, 1025, 6980]
    assert dim == [4, 36, 64, 100, 128, 160, 256, 768, 896, 960, 1024, 1028]
    assert k == [1, 10, 32, 100, 1000, 1323, 1365, 4096, 4097]
    assert nd == [0, 1, 255, 256, 257, 65536, 8841823]
    L = hip.lib()
    search = [(a, b, c) for a in nq for b in dim for c in k]
    index = [(a, b) for a in nd for b in dim]
    for name, shapes in (("mevi_ip_topk_workspace_bytes", search), ("mevi_ip_topk_indexed_workspace_bytes", search),
                         ("mevi_ip_topk_indexed8_workspace_bytes", search), ("mevi_ip_index_bytes", index),
                         ("mevi_ip_index8_bytes", index)):
        want = rec[name]
        assert len(want) == len(shapes), name
        got = [getattr(L, name)(*s) for s in shapes]
        wrong = [(s, g, w) for s, g, w in zip(shapes, got, want) if g != w]
        assert not wrong, f"{name}: {len(wrong)} of {len(shapes)} differ, first {wrong[:3]} (shape, now, recorded)"
        assert any(w > 0 for w in want), name

    # The list scans: workspace bytes and query tile of the four families (tests/golden/scan_workspace_sizes.json, recorded from
    # the commit before their host code was shared): per family the grid formats x nq x nprobe x max_list_len, then the edges.
    with open(os.path.join(ROOT, "tests", "golden", "scan_workspace_sizes.json")) as f:
        rec = json.load(f)
    assert "parent commit" in rec["header"]
    assert rec["nq"] == [0, 1, 33, 4096, 4097, 6980] and rec["nprobe"] == [1, 16, 256, 257]
    assert rec["max_list_len"] == [-1, 0, 1000, 200000, 2097152, 2097156] and (rec["k"], rec["nlist"]) == (10, 100)
    assert rec["formats"] == {"ivf": [[768]], "sq": [[768, 8], [64, 4]], "ivfpq": [[16, 4, 16], [768, 64, 256], [768, 96, 256]],
                              "pqfs": [[32, 8], [768, 96]]}
    assert {f: len(e) for f, e in rec["edges"].items()} == {"ivf": 10, "sq": 14, "ivfpq": 16, "pqfs": 14}
    for family, formats in rec["formats"].items():
        shapes = [(a, b, rec["k"], *fmt, rec["nlist"], c) for fmt in formats for a in rec["nq"] for b in rec["nprobe"]
                  for c in rec["max_list_len"]] + [tuple(e) for e in rec["edges"][family]]
        for what in ("workspace_bytes", "query_tile"):
            name = f"mevi_{family}_scan_{what}"
            want = rec[name]
            assert len(want) == len(shapes), name
            got = [getattr(L, name)(*s) for s in shapes]
            wrong = [(s, g, w) for s, g, w in zip(shapes, got, want) if g != w]
            assert not wrong, f"{name}: {len(wrong)} of {len(shapes)} differ, first {wrong[:3]} (shape, now, recorded)"
            edges = want[-len(rec["edges"][family]):]
            assert any(w > 0 for w in edges) and any(w == 0 for w in edges) and any(w > 0 for w in want[:-len(edges)]), name


def test_product_path_fails_loudly_without_gpu():
    import torch

    from mevi_amd import dense, hip

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(hip.MeviHipError):
        dense.search(np.zeros((2, 8), np.float32), np.zeros((4, 8), np.float32), 8, 2, "Flat")


def test_product_never_imports_oracle():
    """The product path must not import, link, dlopen or execute anything under oracle/."""
    pkg = os.path.join(ROOT, "mevi_amd")
    cli = [os.path.join(ROOT, f) for f in os.listdir(ROOT)
           if f.endswith(".py") and f not in ("bench.py", "__graft_entry__.py")]
    files = cli[:]
    for dirpath, _, fs in os.walk(pkg):
        files += [os.path.join(dirpath, f) for f in fs if f.endswith((".py", ".hip", ".h", ".cpp"))]
    pat = re.compile(r"^\s*(from|import)\s+oracle\b|#include\s+[\"<][^\">]*oracle|libmevi_oracle|dlopen", re.M)
    for f in files:
        assert not pat.search(open(f).read()), f


def test_bench_starts_its_ranks_itself_and_reports_their_failure():
    """`python bench.py --gpus 2` outside a launcher: the parent starts two ranks through
    torch.distributed.run as a child process -- it never imports torch itself, so it cannot have touched the GPU -- and
    hands their exit status on.  Without a GPU both ranks fail loudly (no CPU fallback), so the status is non-zero."""
    import subprocess
    import sys

    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: the GPU suite runs the real thing")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode != 0
    assert r.stderr.count("no MI355X visible") >= 2, r.stderr[-1500:]          # both ranks got as far as the GPU check
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
    src = open(os.path.join(ROOT, "bench.py")).read()
    head = src[:src.index("def late_imports")]
    assert "import torch" not in head and "mevi_amd" not in head.split('"""', 2)[2]   # nothing GPU-capable before the spawn


def test_bench_line_is_compact_and_keeps_the_certificate_in_config():
    """The ONE stdout line must fit the driver's 8 KB tail and carry the MRR@10-match certificate and the chain's rate in
    `config`: checked on a recorded full record."""
    import contextlib
    import io
    import json
    import tempfile

    import bench

    with open(os.path.join(ROOT, "profiles", "r03_bench_n1.json")) as f:
        rec = json.load(f)
    old = os.environ.get("MEVI_BENCH_DETAIL")
    os.environ["MEVI_BENCH_DETAIL"] = os.path.join(tempfile.mkdtemp(), "d.json")
    try:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            bench.print_line(rec)
        with open(os.environ["MEVI_BENCH_DETAIL"]) as f:
            full = json.load(f)
    finally:
        if old is None:
            del os.environ["MEVI_BENCH_DETAIL"]
        else:
            os.environ["MEVI_BENCH_DETAIL"] = old
    out = buf.getvalue()
    assert out.count("\n") == 1 and len(out) < 8192
    line = json.loads(out)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["config"]["workload"].startswith("C2") and line["roofline"]["kernel"] == "ip_filter_h1_kernel"
    m = line["config"]["mrr10_match"]
    assert m["dense_lists_identical"] is True and m["beams_identical"] is True and m["chain_mrr10_abs_diff"] == 0.0
    assert line["config"]["chain_c4"]["queries_per_s"] > 0
    assert "per_batch" in full["dense_small_batch"] and "per_batch" not in line.get("dense_small_batch", {})


def test_bench_dump_outputs_fits_the_budget_and_is_reproducible(tmp_path):
    """--dump-outputs at the bench's full size (6980 lists of 1000): a seeded sample of query rows under 64 MB, f32 scores
    and ids as exact f64, the same rows on every run; a small output is written whole."""
    import torch

    import bench

    rng = np.random.default_rng(7)
    nq, k = bench.N_QUERIES, bench.TOPK
    s = torch.from_numpy(rng.standard_normal((nq, k), dtype=np.float32))
    i = torch.from_numpy(rng.integers(0, bench.N_DOCS, (nq, k)))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), s, i)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["ids.npy", "query_rows.npy", "scores.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    for f in files:
        assert open(tmp_path / "a" / f, "rb").read() == open(tmp_path / "b" / f, "rb").read(), f
    rows = np.load(tmp_path / "a" / "query_rows.npy")
    sc, ids = np.load(tmp_path / "a" / "scores.npy"), np.load(tmp_path / "a" / "ids.npy")
    assert rows.dtype == np.float64 and sc.dtype == np.float32 and ids.dtype == np.float64
    assert 4096 < len(rows) < nq and (np.diff(rows) > 0).all() and sc.shape == ids.shape == (len(rows), k)
    r = rows.astype(np.int64)
    assert np.array_equal(sc, s.numpy()[r]) and np.array_equal(ids.astype(np.int64), i.numpy()[r])

    bench.dump_outputs(str(tmp_path / "small"), s[:50], i[:50])
    assert np.array_equal(np.load(tmp_path / "small" / "query_rows.npy"), np.arange(50))
    assert np.array_equal(np.load(tmp_path / "small" / "ids.npy").astype(np.int64), i.numpy()[:50])


def test_bench_refuses_zero_timed_steps():
    """ms_per_step is the time of one timed step, so there must be at least one (checked before anything is imported)."""
    import subprocess
    import sys

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr
