"""One-process A/B of tuning knobs on the C2 step (bench.py's headline workload: 10k trees x 2^20 rows, f32).

    python tools/c2_knob_ab.py loss_compact=0 loss_compact=1 loss_compact=1,tail_chunk=5,first_chunk=8 ...

Every argument is one configuration (knob=value pairs joined by commas; the knobs it does not name are at the
library's defaults).  The configurations are alternated over --rounds rounds of --steps timed steps each; per
configuration and round the median step_ms, and once per configuration the (tree, row block) pairs the plan
took from the loss launch's candidates / left to the FOLD pass (sr_last_fold_cand) and the listed loss
launches' positions (sr_last_phase_ms out[16..18]), and per compacted FOLD launch (region 2 chunk, + 1 for
the LDS-stack launch) its live workgroups, listed entries, entries per workgroup g and longest row block's list
(out[19 + 4 region ..])."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "symbolicregression.jl_amd")]
import numpy as np

import sr_amd
from bench import C2_OPS, c2_data, single_gpu_call
from sr_amd import Dataset, Options, _lib, flatten_trees, gen_random_population

DEFAULTS = dict(loss_compact=1, loss_list_groups=0, tail_chunk=4, first_chunk=6, fold_compact=1, fold_cand_est=1, exact_early=1,
                code_cache=1, probe=2, fold_list_wgs=2048)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="+")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    configs = [dict((k, int(v)) for k, v in (kv.split("=") for kv in c.split(","))) for c in a.configs]
    ctx = sr_amd.get_context()
    opts = Options(**C2_OPS)
    tb = flatten_trees(gen_random_population(10_000, opts, 5, max_size=30, seed=1), np.float32)
    X, y = c2_data(1 << 20, 0)
    ds = Dataset(X, y)
    ds.device_handle(ctx)
    call, _ = single_gpu_call(ctx, tb, ds, opts)
    med = [[] for _ in configs]
    info = [None] * len(configs)
    for _ in range(a.rounds):
        for i, cfg in enumerate(configs):
            for k, v in {**DEFAULTS, **cfg}.items():
                ctx.set_tuning(k, v)
            for _ in range(a.warmup):
                call()
            ts = []
            for _ in range(a.steps):
                t = time.perf_counter()
                call()
                ts.append((time.perf_counter() - t) * 1e3)
            med[i].append(float(np.median(ts)))
            if info[i] is None:
                out = (ctypes.c_double * 51)()
                _lib.check(_lib.lib.sr_last_phase_ms(ctx.handle, out, 51))
                info[i] = dict(ctx.last_fold_cand(), listed_launches=int(out[16]), listed=int(out[17]),
                               excluded=int(out[18]), kernel_ms=round(ctx.last_kernel_ms()[0], 3),
                               fold_lists=[(r, int(out[19 + 4 * r]), int(out[20 + 4 * r]), int(out[21 + 4 * r]),
                                            int(out[22 + 4 * r])) for r in range(8) if out[21 + 4 * r] > 0])
    for k, v in DEFAULTS.items():
        ctx.set_tuning(k, v)
    for cfg, m, inf in zip(a.configs, med, info):
        print(f"{cfg:48s} step_ms medians per round: {' '.join(f'{v:.3f}' for v in m)}  {inf}", flush=True)


if __name__ == "__main__":
    main()
