"""Cost of an interpreted elementwise loss (sr_register_loss_expr) against the catalog loss it restates.

DESIGN.md §14's workload: 2,000 trees of the C2 distribution (5 features, up to 30 nodes) x 2^17 rows, both
element types; `square(p - t)` against L2DistLoss() and the logit restatement against LogitDistLoss(), the
catalog calls at "ref_fold" 0 (the f64 sums an expression-loss call returns too: the same launch sequence
but for the kernels).  Medians of 15 calls: wall and the loss launches' device time (sr_last_kernel_ms) of
eval_loss_batch, wall and the tangent kernels' time per bucket (sr_last_grad_info) of eval_grad_batch.
The catalog call's loss launch runs the register-stack build (16 / 8 rows per lane), which the expression
set does not have; so the catalog loss call is timed a second time with the classic kernel forced
("rows_per_lane" 8 / 4: the expression builds' own shape) — that ratio is the interpreter's price alone.
One JSON line per (dtype, loss).
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "symbolicregression.jl_amd")]
import numpy as np  # noqa: E402

import sr_amd  # noqa: E402
from sr_amd import Dataset, Options, eval_grad_batch, eval_loss_batch, flatten_trees, gen_random_population  # noqa: E402

N, NF, NT, CALLS = 1 << 17, 5, 2000, 15
OPS = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "log"])
PAIRS = [("L2DistLoss()", "loss(p, t) = square(p - t)"),
         ("LogitDistLoss()", "loss(p, t) = -log(4.0) - (p - t) + 2.0*log(1.0 + exp(p - t))")]
ctx = sr_amd.get_context()
ctx.set_tuning("timing", 1)
ctx.set_tuning("ref_fold", 0)


def timed_loss(tb, ds, opts, rows=0):
    ctx.set_tuning("rows_per_lane", rows)
    try:
        eval_loss_batch(tb, ds, opts)
        wall, kern = [], []
        for _ in range(CALLS):
            t0 = time.perf_counter()
            eval_loss_batch(tb, ds, opts)
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(ctx.last_kernel_ms()[0])
        return {"loss_wall_ms": float(np.median(wall)), "loss_kernel_ms": float(np.median(kern)),
                "rows_per_lane": ctx.last_rows_per_lane()}
    finally:
        ctx.set_tuning("rows_per_lane", 0)


def timed(tb, ds, opts):
    eval_loss_batch(tb, ds, opts)
    wall, kern = [], []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        out = eval_loss_batch(tb, ds, opts)
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(ctx.last_kernel_ms()[0])
    eval_grad_batch(tb, ds, opts)
    gwall, gkern = [], []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        eval_grad_batch(tb, ds, opts)
        gwall.append((time.perf_counter() - t0) * 1e3)
        gkern.append([b["kernel_ms"] for b in ctx.last_grad_info()])
    info = ctx.last_grad_info()
    gk = np.median(np.array(gkern), axis=0)
    return out, {"loss_wall_ms": float(np.median(wall)), "loss_kernel_ms": float(np.median(kern)),
                 "rows_per_lane": ctx.last_rows_per_lane(), "grad_wall_ms": float(np.median(gwall)),
                 "grad_kernel_ms": gk.tolist(), "grad_kernel_ms_sum": float(gk.sum()),
                 "grad_rows_per_lane": [b["rows_per_lane"] for b in info]}


for dt in (np.float32, np.float64):
    rng = np.random.default_rng(1)
    X = rng.standard_normal((NF, N)).astype(dt)
    y = (2 * np.cos(X[3]) + X[0] ** 2 - 2).astype(dt)
    ds = Dataset(X, y)
    for cat, expr in PAIRS:
        oc, oe = Options(elementwise_loss=cat, **OPS), Options(elementwise_loss=expr, **OPS)
        tb = flatten_trees(gen_random_population(NT, oc, NF, max_size=30, dtype=dt, seed=1), dt)
        (lc, cc), rc = timed(tb, ds, oc)
        (le, ce), re_ = timed(tb, ds, oe)
        rk = timed_loss(tb, ds, oc, rows=8 if dt == np.float32 else 4)
        fin = cc & np.isfinite(lc) & np.isfinite(le)
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.abs(le[fin].astype(np.float64) - lc[fin]) / np.maximum(np.abs(lc[fin].astype(np.float64)), 1e-300)
        print(json.dumps({"dtype": np.dtype(dt).name, "catalog": cat, "expression": expr, "trees": NT, "rows": N,
                          "complete": int(cc.sum()), "flags_equal": bool(np.array_equal(cc, ce)),
                          "median_rel_diff": float(np.median(rel)), "catalog_call": rc, "expression_call": re_,
                          "catalog_call_classic_kernel": rk,
                          "ratio_loss_kernel_vs_classic": re_["loss_kernel_ms"] / rk["loss_kernel_ms"],
                          "ratio_loss_kernel": re_["loss_kernel_ms"] / rc["loss_kernel_ms"],
                          "ratio_loss_wall": re_["loss_wall_ms"] / rc["loss_wall_ms"],
                          "ratio_grad_kernel": re_["grad_kernel_ms_sum"] / rc["grad_kernel_ms_sum"],
                          "ratio_grad_wall": re_["grad_wall_ms"] / rc["grad_wall_ms"]}), flush=True)
    ds.free_device()
