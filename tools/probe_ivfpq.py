"""One IVF-PQ search regime at C2 size, repeated, for a kernel trace: which of the ADC search's kernels the time goes to.
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/probe_ivfpq.py [nlist] [nprobe] [nq] [reps] [--docs N]
(the build's kernels are in the trace too; the search's are ivf_scan_kernel / ivf_select_kernel of the coarse call and
adc_clean_kernel / adc_lut_kernel / ivfpq_scan_kernel and, again, ivf_select_kernel: select, clean and lut carry one name for every
family of list scan)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from mevi_amd import ivfpq  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    nlist, nprobe, nq, reps = (int(v) for v in (args + ["100", "4", str(bench.N_QUERIES), "3"][len(args):]))
    n_docs = int(sys.argv[sys.argv.index("--docs") + 1]) if "--docs" in sys.argv else bench.N_DOCS
    dev = torch.device("cuda:0")
    docs = bench.gen_shard(0, n_docs, dev, n_docs)
    q = bench.gen_queries(nq, dev, n_docs)
    index = ivfpq.IVFPQIndex(docs, nlist, 64, 8)
    for _ in range(reps):
        index.search_scan(q, bench.TOPK, nprobe)
    torch.cuda.synchronize()
    print(f"IVF{nlist},PQ64 nprobe {nprobe}, {nq} queries, {reps} searches")


if __name__ == "__main__":
    main()
