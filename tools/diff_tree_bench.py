#!/usr/bin/env python3
"""Cost of the per-row derivative calls: writes profiles/diff_tree_array_bench.txt.

    python tools/diff_tree_bench.py [--trees 2000] [--rows 131072] [--calls 15] [--out profiles/diff_tree_array_bench.txt]

Workload: trees of the C2 distribution (node_count ~ U{1..30}, + - * / cos exp log, 5 features) x 2^17 rows, both
element types; modes: variable=False, variable=True (nfeatures = 5) and diff (direction 1 + t mod 5).  Per mode:
two warm-up calls, then the median of `calls` timed calls with the spread (min .. max) — kernel time is the sum
of sr_last_grad_info's buckets (HIP events around the tangent launches; the context's "timing" on), wall time the
whole call (PRED pass, launches, copies to the caller's arrays).  Beside the kernel time: the bytes the kernels
must write, sum over launched trees of n_grad_t x n_rows x sizeof(T), and the share of the HBM peak that
implies.  The peak is the microarchitecture guide's 8 TB/s (MI355X: 8 HBM3E stacks); its measured achievable
figure for a streaming write kernel is lower, so the share understates how close to the roof the stores run.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "symbolicregression.jl_amd"))

import sr_amd  # noqa: E402
from sr_amd import Dataset, Options, eval_diff_tree_array_batch, eval_grad_tree_array_batch, flatten_trees  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=2000)
    ap.add_argument("--rows", type=int, default=1 << 17)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diff_tree_array_bench.txt"))
    args = ap.parse_args()
    nf = 5
    opts = Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "log"])
    trees = sr_amd.gen_random_population(args.trees, opts, nf, seed=0)
    ctx = sr_amd.get_context()
    ctx.set_tuning("timing", 1)
    lines = [f"# tools/diff_tree_bench.py: {args.trees} C2 trees x {args.rows} rows, nfeatures = {nf}; "
             f"2 warm-up calls, median (min .. max) of {args.calls} calls",
             "# kernel_ms: sum of sr_last_grad_info's buckets; bytes: sum n_grad_t x n_rows x sizeof(T) over the "
             "launched (complete) trees; share: bytes / kernel time / 8 TB/s (HBM peak, MI355X_MICROARCH.md)",
             "# dtype mode trees_launched kernel_ms(min..max) wall_ms(min..max) bytes_written GB/s share_of_peak"]
    for dtype in (np.float32, np.float64):
        rng = np.random.default_rng(2)
        X = rng.standard_normal((nf, args.rows)).astype(dtype)
        ds = Dataset(X)
        tb = flatten_trees(trees, dtype)
        directions = 1 + np.arange(tb.n_trees) % nf
        modes = (("variable=false", lambda: eval_grad_tree_array_batch(tb, ds, opts, variable=False)),
                 ("variable=true", lambda: eval_grad_tree_array_batch(tb, ds, opts, variable=True)),
                 ("diff", lambda: eval_diff_tree_array_batch(tb, ds, opts, directions)))
        for name, call in modes:
            kms, wms = [], []
            nbytes = launched = 0
            for i in range(2 + args.calls):
                t0 = time.perf_counter()
                _, grads, comp = call()
                wall = (time.perf_counter() - t0) * 1e3
                if i < 2:
                    continue
                wms.append(wall)
                kms.append(sum(b["kernel_ms"] for b in ctx.last_grad_info()))
                if name == "diff":
                    launched = int(comp.sum())  # (a tree found non-finite was launched too: a lower bound)
                    nbytes = launched * args.rows * np.dtype(dtype).itemsize
                else:
                    nbytes = sum(grads[t].size for t in np.flatnonzero(comp)) * np.dtype(dtype).itemsize
                    launched = int(sum(1 for t in np.flatnonzero(comp) if grads[t].size))
                del grads
            k, w = statistics.median(kms), statistics.median(wms)
            bw = nbytes / (k * 1e-3) if k > 0 else 0.0
            lines.append(f"{np.dtype(dtype).name} {name} {launched} {k:.3f}({min(kms):.3f}..{max(kms):.3f}) "
                         f"{w:.1f}({min(wms):.1f}..{max(wms):.1f}) {nbytes} {bw / 1e9:.1f} {bw / HBM_PEAK:.3f}")
            print(lines[-1], flush=True)
        ds.free_device()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
