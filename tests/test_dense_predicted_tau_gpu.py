"""Large batches of the indexed dense search predict their filter thresholds launch by launch (csrc/ip_topk.hip: plan_pass,
run_pass; DESIGN 4.1b'): after the exact launches have seen ~50 k rows, every further launch runs under the r-th key of the
query's list, r chosen so that the list is expected to hold c_s K' keys above it, with a margin that depends on the dispersion D
the pass measured on its last exact launch.  Exactness never rests on the prediction: sample_check_kernel flags every query for
which fewer than K' rows beat it, and flagged queries take the second pass / the exact path.

Checked here: the oracle's lists bit for bit under both schedules (MEVI_IP_SPEC_TAU=0: the geometric schedule to the end), fewer
launches with predictions, the batch-size boundary (<= 1024 queries keep their schedule), row orders that break the premise,
run-structured rows (D > 1), and -- without a GPU -- the plan itself through mevi_ip_topk_plan, the function the pass calls.
"""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 64


# ---- the plan (CPU) ----------------------------------------------------------------------------------------------------------
def _geom_cap(kp):
    S = 1
    while S < kp:
        S *= 2
    S = min(max(4 * S, 2048), 16384)
    return S - kp


def _plan(L, nq, nd, kp, cap, D):
    n = L.mevi_ip_topk_plan(nq, nd, kp, cap, D, 0, None, None, None)
    assert n >= 0
    rows, rank, keys = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float64)
    assert L.mevi_ip_topk_plan(nq, nd, kp, cap, D, n, rows.ctypes.data_as(ctypes.c_void_p), rank.ctypes.data_as(ctypes.c_void_p),
                               keys.ctypes.data_as(ctypes.c_void_p)) == n
    return rows[:n], rank[:n], keys[:n]


def _parent_plan(nq, nd, k, cap, one_shot):
    """The schedule before predicted thresholds: the first chunk fills the candidate area, every further one is growth x the rows
    seen (growth from the cost model of its time), and searches of <= 1024 queries take all remaining rows in ONE sampled launch
    once enough rows are in."""
    growth = max(cap / (3.0 * k), 1.0)
    keys, t_launch = nq * k * 60e-9 * 1e3, 0.2
    best, best_cost = growth, (keys * growth + t_launch) / math.log(1.0 + growth)
    cand = 1.0
    while cand < growth:
        c = (keys * cand + t_launch) / math.log(1.0 + cand)
        if c < best_cost * 0.99:
            best, best_cost = cand, c
        cand += 0.25
    growth = best
    cap_docs = cap // 256 * 256
    s_c, n_sample = 0.0, 0
    if one_shot and 32 <= k <= 4096:
        r = min(max(k // 2, 16), 96) * 1.0
        c = min(3.0 if r >= 96.0 else 8.0, cap / (k * (1.0 + 8.0 / math.sqrt(r))))
        if c >= 1.5 and (1.0 - 1.0 / c) * math.sqrt(r) >= 4.5:
            s_c, n_sample = c, math.ceil(r * nd / (c * k))
    out, seen, sampled = [], 0, False
    while seen < nd:
        chunk = cap_docs
        if seen >= k:
            chunk = max(chunk, int(seen * growth) // 256 * 256)
        chunk = min(chunk, nd - seen)
        rank = 0
        if s_c > 0.0 and not sampled and seen >= n_sample and seen >= k and chunk < nd - seen:
            r = math.ceil(s_c * k * seen / nd)
            if 16 <= r <= k:
                sampled, chunk, rank = True, nd - seen, r
        out.append((chunk, rank))
        seen += chunk
    return out


def _z_below(nq, launches):
    """The z of the failure budget nq x launches x Phi(-z) <= 1e-3, rounded DOWN (the library may only be stricter)."""
    budget, lo, hi = 1e-3 / (nq * launches), 0.0, 12.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if 0.5 * math.erfc(mid / math.sqrt(2.0)) <= budget:
            hi = mid
        else:
            lo = mid
    return lo


PLAN_GRID = [(nq, nd, kp, D) for nq in (1, 64, 1024, 1025, 1100, 6980, 50000) for nd in (0, 5000, 120000, 400000, 8841823, 50_000_000)
             for kp in (64, 192, 1280, 4096) for D in (1.0, 1.5, 3.0, 8.0, 30.0, 64.0, 200.0)]


def test_plan_covers_the_corpus_and_every_predicted_launch_keeps_its_margins():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    L = hip.lib()
    n_predicted = 0
    for nq, nd, kp, D in PLAN_GRID:
        cap = _geom_cap(kp)
        rows, rank, keys = _plan(L, nq, nd, kp, cap, D)
        what = (nq, nd, kp, D)
        # tile aligned chunks that cover [0, nd) exactly once
        assert int(rows.sum()) == nd and (rows > 0).all(), what
        assert (rows[:-1] % 256 == 0).all(), what
        pred = np.flatnonzero(rank > 0)
        if nq <= 1024:      # the schedule small batches have always had, whatever D
            assert [(int(a), int(b)) for a, b in zip(rows, rank)] == _parent_plan(nq, nd, kp, cap, True), what
            continue
        if D >= 64.0:       # a prefix predicts too little: today's schedule, launch for launch
            assert len(pred) == 0, what
            assert [(int(a), int(b)) for a, b in zip(rows, rank)] == _parent_plan(nq, nd, kp, cap, False), what
            continue
        if len(pred) == 0:
            continue
        z = _z_below(nq, len(pred))
        starts = np.concatenate([[0], np.cumsum(rows)[:-1]])
        assert len(rows) < len(_parent_plan(nq, nd, kp, cap, False)), what
        for i in pred:
            seen, chunk, r = int(starts[i]), int(rows[i]), int(rank[i])
            assert seen >= 50000, what
            c_s = keys[i] * (seen + chunk) / (kp * chunk)      # expected keys appended = c_s K' chunk / (seen + chunk)
            assert c_s >= 1.15 - 1e-9, what
            assert abs(r - math.ceil(c_s * kp * seen / (seen + chunk) - 1e-6)) == 0 and 16 <= r <= kp, (what, r, c_s)
            assert (1.0 - 1.0 / c_s) * math.sqrt(r / D) >= z, (what, r, c_s, z)
            assert c_s * kp * (1.0 + z * math.sqrt(D / r)) <= cap * (1.0 + 1e-12), (what, r, c_s, z)
            n_predicted += 1
    assert n_predicted > 100       # the grid does exercise the path


# ---- the searches (GPU) ------------------------------------------------------------------------------------------------------
def _child_search(q, d, k, env, tmp):
    """One indexed search in a child process (the switch is read once per process): ids, scores and the statistics."""
    code = ("import os, sys, ctypes, numpy as np, torch; sys.path.insert(0, %r); from mevi_amd import dense, hip; "
            "q = np.load(sys.argv[1]); d = np.load(sys.argv[2]); dev = torch.device('cuda:0'); "
            "s, i = dense.DenseIndex(torch.from_numpy(d).to(dev)).search(torch.from_numpy(q).to(dev), int(sys.argv[3])); torch.cuda.synchronize(); "
            "st = hip.IpTopkStats(); hip.lib().mevi_ip_topk_get_stats(st); "
            "np.save(sys.argv[4], i.cpu().numpy()); np.save(sys.argv[5], s.cpu().numpy()); "
            "print(int(st.n_chunks), int(st.n_failed_queries), int(st.n_second_pass_queries), int(st.n_predicted_launches), float(st.dispersion))" % ROOT)
    np.save(tmp + "/q.npy", q), np.save(tmp + "/d.npy", d)
    r = subprocess.run([sys.executable, "-c", code, tmp + "/q.npy", tmp + "/d.npy", str(k), tmp + "/i.npy", tmp + "/s.npy"],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    f = r.stdout.split()[-5:]
    return {"ids": np.load(tmp + "/i.npy"), "scores": np.load(tmp + "/s.npy"), "launches": int(f[0]), "failed": int(f[1]),
            "second_pass": int(f[2]), "predicted": int(f[3]), "D": float(f[4])}


def _same(run, es, ei):
    np.testing.assert_array_equal(run["ids"], ei)
    np.testing.assert_array_equal(run["scores"].view(np.uint32), es.view(np.uint32))


_IID = {}


def _iid(nq, nd, k):
    """i.i.d. rows and the oracle's lists, computed once per shape and never changed."""
    from oracle import dense as odense

    if (nq, nd, k) not in _IID:
        rng = np.random.default_rng(nq + nd + k)
        q = rng.standard_normal((nq, DIM), dtype=np.float32)
        d = rng.standard_normal((nd, DIM), dtype=np.float32)
        es, ei = odense.ip_topk_exact(q, d, k)
        for a in (q, d, es, ei):
            a.setflags(write=False)
        _IID[(nq, nd, k)] = (q, d, es, ei)
    return _IID[(nq, nd, k)]


@pytest.mark.gpu
@pytest.mark.parametrize("nq,nd,k", [(1100, 400_000, 100), (1300, 600_000, 1000)])
def test_both_schedules_return_the_oracles_lists_and_predictions_save_launches(cuda, nq, nd, k, tmp_path):
    q, d, es, ei = _iid(nq, nd, k)
    on = _child_search(q, d, k, {}, str(tmp_path))
    off = _child_search(q, d, k, {"MEVI_IP_SPEC_TAU": "0"}, str(tmp_path))
    print("launches", on["launches"], off["launches"], "predicted", on["predicted"], "D", on["D"])
    for run in (on, off):
        _same(run, es, ei)
        assert run["failed"] == 0
    np.testing.assert_array_equal(on["ids"], off["ids"])
    np.testing.assert_array_equal(on["scores"].view(np.uint32), off["scores"].view(np.uint32))
    assert on["launches"] < off["launches"], (on["launches"], off["launches"])
    assert on["predicted"] >= 1 and off["predicted"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1024, 1025])
def test_batch_size_boundary(cuda, nq, tmp_path):
    """1024 queries keep their schedule (the sampled last launch) whatever the switch says; 1025 predict."""
    q, d, es, ei = _iid(1100, 400_000, 100)
    on = _child_search(q[:nq], d, 100, {}, str(tmp_path))
    off = _child_search(q[:nq], d, 100, {"MEVI_IP_SPEC_TAU": "0"}, str(tmp_path))
    print(nq, "launches", on["launches"], off["launches"])
    for run in (on, off):
        _same(run, es[:nq], ei[:nq])
    if nq == 1024:
        assert on["launches"] == off["launches"]
    else:
        assert on["launches"] < off["launches"]


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["best rows first", "worst rows first", "40 distinct rows"])
def test_row_orders_that_break_the_premise_still_return_the_oracles_lists(cuda, order):
    import torch

    from mevi_amd import dense
    from oracle import dense as odense

    q, d, _, _ = _iid(1100, 400_000, 100)
    if order == "40 distinct rows":
        d = d[:40][np.random.default_rng(5).integers(0, 40, d.shape[0])].copy()
    else:
        sc = d @ q[0]
        d = d[np.argsort(-sc if order == "best rows first" else sc, kind="stable")].copy()
    es, ei = odense.ip_topk_exact(q, d, 100)
    s, i = dense.DenseIndex(torch.from_numpy(d).to(cuda)).search(torch.from_numpy(q.copy()).to(cuda), 100)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(i.cpu().numpy(), ei)
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), es.view(np.uint32))


@pytest.mark.gpu
def test_run_structured_rows_report_their_dispersion(cuda, tmp_path):
    """Rows in clusters laid out in adjacent runs (geometric length, mean 8: tools/synth.py's clustered corpus): the keys a
    launch appends per query come in runs, the pass reports D > 1 and widens its margins, and no more queries are flagged than
    under the geometric schedule."""
    from oracle import dense as odense

    nq, nd, k, n_clusters = 1100, 400_000, 100, 500
    rng = np.random.default_rng(77)
    centres = 0.05 * rng.standard_normal((n_clusters, DIM), dtype=np.float32)
    w = 1.0 / (np.arange(n_clusters) + 10.0) ** 0.7
    new_run = rng.random(nd) < 1.0 / 8
    new_run[0] = True
    run_id = np.cumsum(new_run) - 1
    cl = rng.choice(n_clusters, size=int(run_id[-1]) + 1, p=w / w.sum())[run_id]
    d = (centres[cl] + 0.012 * rng.standard_normal((nd, DIM), dtype=np.float32) + 0.02).astype(np.float32)
    ids = (np.arange(nq) * (nd // nq) + 17) % nd
    q = (d[ids] + 0.006 * rng.standard_normal((nq, DIM), dtype=np.float32)).astype(np.float32)
    es, ei = odense.ip_topk_exact(q, d, k)
    on = _child_search(q, d, k, {}, str(tmp_path))
    off = _child_search(q, d, k, {"MEVI_IP_SPEC_TAU": "0"}, str(tmp_path))
    print("D", on["D"], "launches", on["launches"], off["launches"], "flagged", on["failed"] + on["second_pass"],
          off["failed"] + off["second_pass"])
    _same(on, es, ei)
    _same(off, es, ei)
    assert on["D"] > 1.0
    assert on["failed"] + on["second_pass"] <= off["failed"] + off["second_pass"]
