"""Cost of the template path: wall time of eval_loss_batch on 2,000 TemplateExpression
candidates x 2^17 rows against the same call on the pre-composed batch, median of 15 calls, and the host
composition's share.  Structure: two sub-expressions and one repeated call, sub-trees from the C2 distribution
(node_count ~ U{1..30}).

    python tools/template_bench.py [--trees 2000] [--rows 131072] [--calls 15]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "symbolicregression.jl_amd")]

import sr_amd  # noqa: E402
from sr_amd import (Dataset, Options, TemplateExpression, TemplateStructure, compose, eval_loss_batch,  # noqa: E402
                    flatten_trees)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=2000)
    ap.add_argument("--rows", type=int, default=1 << 17)
    ap.add_argument("--calls", type=int, default=15)
    a = ap.parse_args()
    opts = Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "log"])
    rng = np.random.default_rng(0)
    X = rng.standard_normal((5, a.rows)).astype(np.float32)
    y = (2 * np.cos(X[3]) + X[0] ** 2 - 2).astype(np.float32)
    ds = Dataset(X, y)
    st = TemplateStructure(("f", "g"), "f(x1, x2, x3) * g(x4, x5) + f(x3, x4, x5)")
    pop = [TemplateExpression({"f": sr_amd.gen_random_tree_fixed_size(int(rng.integers(1, 31)), opts, 3, np.float32, rng),
                               "g": sr_amd.gen_random_tree_fixed_size(int(rng.integers(1, 31)), opts, 2, np.float32, rng)},
                              structure=st) for _ in range(a.trees)]

    def timed(fn):
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    uo = Options(operators=st.union_operators(opts.operators))
    composed = [compose(ex, opts) for ex in pop]
    tb = flatten_trees([c.tree for c in composed] + [g for c in composed for g in c.guards], np.float32)
    eval_loss_batch(pop, ds, opts), eval_loss_batch(tb, ds, uo)  # warm-up
    t_tmpl = timed(lambda: eval_loss_batch(pop, ds, opts))
    t_pre = timed(lambda: eval_loss_batch(tb, ds, uo))
    t_comp = timed(lambda: [compose(ex, opts) for ex in pop])
    t_flat = timed(lambda: flatten_trees([c.tree for c in composed] + [g for c in composed for g in c.guards], np.float32))
    l1, c1 = eval_loss_batch(pop, ds, opts)
    print(f"template_bench: {a.trees} templates x {a.rows} rows, Float32, median of {a.calls} calls; composed batch "
          f"{tb.n_trees} trees ({tb.n_trees - a.trees} guards), {tb.n_nodes} nodes; {int(c1.sum())} complete")
    print(f"  eval_loss_batch(templates)        {t_tmpl:9.2f} ms")
    print(f"  eval_loss_batch(pre-composed)     {t_pre:9.2f} ms")
    print(f"  compose() of the population       {t_comp:9.2f} ms  ({100 * t_comp / t_tmpl:.1f} % of the template call)")
    print(f"  flatten_trees of the composed     {t_flat:9.2f} ms  ({100 * t_flat / t_tmpl:.1f} % of the template call)")
    print(f"  host share of the template call (compose + flatten + glue): {100 * (t_tmpl - t_pre) / t_tmpl:.1f} %")


if __name__ == "__main__":
    main()
