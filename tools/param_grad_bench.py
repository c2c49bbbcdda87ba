"""Cost of the parametric gradient call (sr_eval_grad_batch_parametric) against the plain twins.

DESIGN.md §13's workload: 2,000 trees of the C2 distribution over 5 + 2 features with the last two
features' leaves turned into p1, p2, 2^17 rows, one shared matrix; the plain twins are the same trees on the
materialised 7-row X_ext, which computes no parameter tangents: the ratio is the price of the parameter
tangents plus the class binning.  The interpreter's work does not depend on the number of classes, the
binning's does, so the call is timed at 1, 8 and 64 classes, and under both binning schemes: the default
(per-lane class accumulators where slots x classes <= 16, else one masked wave sum per class present in a
64-row group and parameter tangent) and the wave sums everywhere (tuning "grad_lane_bins" 0).  Medians of 15 calls: wall, and the tangent kernels' time per bucket
(sr_last_grad_info).  Then one optimize_constants_batch of the 8-class population.
One JSON line per (dtype, classes).
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "symbolicregression.jl_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import sr_amd  # noqa: E402
from sr_amd import Dataset, Options, eval_grad_batch, optimize_constants_batch  # noqa: E402
from parametric_util import population, to_parametric, x_ext  # noqa: E402

N, NF, K, NT, CALLS = 1 << 17, 5, 2, 2000, 15
opts = Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "log"])
ctx = sr_amd.get_context()
ctx.set_tuning("timing", 1)


def timed(tb, ds, lane_bins=1):
    ctx.set_tuning("grad_lane_bins", lane_bins)
    eval_grad_batch(tb, ds, opts)
    wall, kern = [], []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        out = eval_grad_batch(tb, ds, opts)
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append([b["kernel_ms"] for b in ctx.last_grad_info()])
    info = ctx.last_grad_info()
    ctx.set_tuning("grad_lane_bins", 1)
    return out, float(np.median(wall)), np.median(np.array(kern), axis=0).tolist(), info


for dt in (np.float64, np.float32):
    rng = np.random.default_rng(1)
    X = rng.standard_normal((NF, N)).astype(dt)
    y = (2 * np.cos(X[3]) + X[0] ** 2 - 2).astype(dt)
    ext = population(NT, opts, NF, K, dt, seed=1, max_size=30)
    for C in (8, 1, 64):
        cls = rng.integers(1, C + 1, N).astype(np.int32)
        P = rng.standard_normal((K, C)).astype(dt)
        par = to_parametric(ext, NF, P)
        pds = Dataset(X, y, extra={"class": cls}, n_classes=C)
        tds = Dataset(x_ext(X, P, cls), y)
        (lp, gp, cp), wall_p, kern_p, info_p = timed(par, pds)
        # the same call with the per-lane class accumulators off: the masked wave sums everywhere
        (_, gw, _), wall_w, kern_w, info_w = timed(par, pds, lane_bins=0)
        (lt, gt, ct), wall_t, kern_t, info_t = timed(ext, tds)
        gc = par.split_scalars(gp)[0]
        # (bit-equal at sizes where both calls split the rows into the same row blocks — the tests' sizes; here
        #  the two calls' buckets differ in size, and with them the row blocks: compared to rounding only)
        bit_equal = bool(np.array_equal(cp, ct) and np.array_equal(gc.view(np.uint8), gt.view(np.uint8)))
        schemes_close = bool(np.allclose(gp, gw, rtol=1e-4 if dt == np.float32 else 1e-9, atol=1e-12, equal_nan=True))
        close = bool(np.array_equal(cp, ct) and np.allclose(gc, gt, rtol=1e-4 if dt == np.float32 else 1e-9, atol=1e-12,
                                                            equal_nan=True))
        rec = {"dtype": np.dtype(dt).name, "classes": C, "trees": NT, "rows": N, "complete": int(cp.sum()),
               "parameter_leaves": int(par.is_parameter.sum()), "nodes": int(par.n_nodes),
               "constants_agree_with_twin": close, "constants_bit_equal_to_twin": bit_equal,
               "lane_slots_per_bucket": [min(k, K) if dt == np.float32 and min(k, K) * C <= 16 else 0 for k in (1, 2, 4, 8, 16)],
               "schemes_agree": schemes_close,
               "parametric_wave_sums_only": {"wall_ms": wall_w, "kernel_ms": kern_w, "kernel_ms_sum": float(sum(kern_w))},
               "parametric": {"wall_ms": wall_p, "kernel_ms": kern_p, "kernel_ms_sum": float(sum(kern_p)),
                              "items": [b["items"] for b in info_p], "rows_per_lane": [b["rows_per_lane"] for b in info_p]},
               "twin": {"wall_ms": wall_t, "kernel_ms": kern_t, "kernel_ms_sum": float(sum(kern_t)),
                        "items": [b["items"] for b in info_t], "rows_per_lane": [b["rows_per_lane"] for b in info_t]}}
        if C == 8:
            t0 = time.perf_counter()
            _, _, improved, evals = optimize_constants_batch(par, pds, opts, np.random.default_rng(0))
            rec["optimiser"] = {"wall_s": time.perf_counter() - t0, "improved": int(improved.sum()),
                                "f_calls": float(evals.sum())}
        print(json.dumps(rec), flush=True)
        pds.free_device()
        tds.free_device()
