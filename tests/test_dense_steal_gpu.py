"""Stealing in the ticketed tile walk of the large-batch f16 filter (csrc/ip_topk.hip: ip_filter_h16_kernel): a
workgroup whose own label's counter has run past its range draws tiles from the other labels' counters.  Which workgroup computes
a tile cannot change its keys, so the lists must be the oracle's, bit for bit, under all three settings of MEVI_IP_STEAL:
unset (stealing), 0 (the walk without it) and force (no workgroup draws from its own label's counter: every ticketed tile is
stolen, which takes the steal path deterministically).  The switch is read once per process, so every setting runs in ONE child
process that searches all the cases below; the oracle's lists are computed once per corpus.

Also checked, through mevi_ip_topk_get_walk_counts: the tiles computed are exactly the launches' items (none lost, none twice),
and the stolen ones are none under 0, every ticketed item under force, and never more than those under the default.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (queries, rows, dim, k, query blocks per wave of the kernel the shape runs: query tiles of 32 NI)
CASES = {
    "ticketed": (300, 262144, 128, 10, 8),        # the ragged second query tile included; launches of more than 8 x 2P items
    "not_multiple_of_8": (300, 263449, 128, 10, 8),
    "short_ranges": (300, 3000, 128, 10, 8),      # launches of 14 and 10 items: ranges shorter than 2P, workgroups without an item
    "ni4": (100, 262144, 128, 10, 4),
    "q50_dim128": (50, 262144, 128, 10, 4),       # (a 128-k image has four units: the 64-query tile is not offered there)
    "ni2": (50, 262144, 192, 10, 2),
}
SETTINGS = {"default": None, "0": "0", "force": "force"}

_CHILD = r"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from mevi_amd import dense, hip
cases = json.loads(sys.argv[2]); tmp = sys.argv[3]
dev = torch.device('cuda:0')
hip.lib().mevi_ip_topk_set_profiling(1)
out = {}
for name, (nq, nd, dim, k, ni) in cases.items():
    d = np.load(os.path.join(tmp, 'd_%d.npy' % dim))[:nd]
    q = np.load(os.path.join(tmp, 'q_%d.npy' % dim))[:nq]
    index = dense.DenseIndex(torch.from_numpy(d).to(dev))
    sys.stderr.write('case %s\n' % name); sys.stderr.flush()
    s, i = index.search(torch.from_numpy(q).to(dev), k)
    torch.cuda.synchronize()
    st = hip.IpTopkStats(); hip.lib().mevi_ip_topk_get_stats(st)
    tiles, stolen = hip.ip_walk_counts()
    np.save(os.path.join(tmp, 'i_%s.npy' % name), i.cpu().numpy()); np.save(os.path.join(tmp, 's_%s.npy' % name), s.cpu().numpy())
    out[name] = dict(tiles=tiles, stolen=stolen, failed=int(st.n_failed_queries), second_pass=int(st.n_second_pass_queries),
                     launches=int(st.n_chunks))
    del index
out['cus'] = torch.cuda.get_device_properties(0).multi_processor_count
print(json.dumps(out))
"""


def _corpus(dim):
    rng = np.random.default_rng(1000 + dim)
    nd = max(c[1] for c in CASES.values() if c[2] == dim)
    nq = max(c[0] for c in CASES.values() if c[2] == dim)
    return rng.standard_normal((nq, dim), dtype=np.float32), rng.standard_normal((nd, dim), dtype=np.float32)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The two corpora (128 and 192 dims) on disk for the children, and the oracle's lists per (rows, dim): the cases with fewer
    queries are the first rows of the same query matrix."""
    from oracle import dense as odense

    tmp = str(tmp_path_factory.mktemp("steal"))
    ref = {}
    for dim in sorted({c[2] for c in CASES.values()}):
        q, d = _corpus(dim)
        np.save(os.path.join(tmp, "q_%d.npy" % dim), q), np.save(os.path.join(tmp, "d_%d.npy" % dim), d)
        for nd in sorted({c[1] for c in CASES.values() if c[2] == dim}):
            es, ei = odense.ip_topk_exact(q, d[:nd], 10)
            es.setflags(write=False), ei.setflags(write=False)
            ref[(nd, dim)] = (es, ei)
    return tmp, ref


_RUNS = {}


def _run(setting, tmp):
    """All cases under one setting of MEVI_IP_STEAL, in one child process (once per setting)."""
    if setting not in _RUNS:
        env = {k: v for k, v in os.environ.items() if k != "MEVI_IP_STEAL"}
        env["MEVI_IP_TOPK_TRACE"] = "1"
        if SETTINGS[setting] is not None:
            env["MEVI_IP_STEAL"] = SETTINGS[setting]
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(CASES), tmp], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads(r.stdout.strip().splitlines()[-1])
        # rows of every filter launch, per case, from the trace
        rows, cur = {}, None
        for line in r.stderr.splitlines():
            m = re.match(r"case (\w+)", line)
            if m:
                cur = m.group(1)
                rows[cur] = []
            m = re.match(r"ip_topk launch \d+: (\d+) rows", line)
            if m and cur:
                rows[cur].append(int(m.group(1)))
        for name in CASES:
            out[name]["rows"] = rows[name]
            out[name]["ids"] = np.load(os.path.join(tmp, "i_%s.npy" % name))
            out[name]["scores"] = np.load(os.path.join(tmp, "s_%s.npy" % name))
        _RUNS[setting] = out
    return _RUNS[setting]


def _launch_items(case, run, cus):
    """Per launch: (items, workgroups per label, ticketed items) -- the grid arithmetic of run_pass and walk_range."""
    nq, _, _, _, ni = CASES[case]
    n_qtiles = -(-nq // (32 * ni))
    out = []
    for rows in run["rows"]:
        n_items = -(-rows // 256) * n_qtiles
        P = min(-(-n_items // 8), cus // 8)
        lens = [(n_items >> 3) + (g < (n_items & 7)) for g in range(8)]
        out.append((n_items, P, sum(max(n - 2 * P, 0) for n in lens)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("case", list(CASES))
def test_lists_are_the_oracles_and_every_item_is_computed_once(cuda, data, case, setting):
    tmp, ref = data
    runs = _run(setting, tmp)
    run = runs[case]
    nq, nd, dim, k, _ = CASES[case]
    es, ei = ref[(nd, dim)]
    launches = _launch_items(case, run, runs["cus"])
    ticketed = sum(t for _, _, t in launches)
    print(case, setting, "launch rows", run["rows"], "items, P, ticketed", launches, "tiles", run["tiles"], "stolen", run["stolen"])
    assert run["failed"] == 0 and run["second_pass"] == 0 and len(run["rows"]) >= 1
    np.testing.assert_array_equal(run["ids"], ei[:nq])
    np.testing.assert_array_equal(run["scores"].view(np.uint32), es[:nq].view(np.uint32))
    assert run["tiles"] == sum(n for n, _, _ in launches)
    if setting == "0":
        assert run["stolen"] == 0
    elif setting == "force":
        assert run["stolen"] == ticketed
    else:
        assert 0 <= run["stolen"] <= ticketed
    # what the case is there for
    big = max(launches)
    if case == "short_ranges":
        assert ticketed == 0 and run["stolen"] == 0
        assert any(n < 8 * P for n, P, _ in launches)            # a workgroup without an item
    else:
        assert big[0] > 16 * big[1] and ticketed > 0             # more than 8 x 2P items: ticketed items exist
        if setting == "force":
            assert run["stolen"] > 0
    if case == "not_multiple_of_8":
        assert big[0] & 7 != 0
