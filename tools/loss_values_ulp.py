"""Measures the inexact-class losses' error against tests/golden/loss_values.json and writes the table
profiles/loss_values_ulp.txt that tests/loss_values_util.py's BARS quote.

    python tools/loss_values_ulp.py [--out profiles/loss_values_ulp.txt]

Per loss and dtype: the largest |got - fixture| in ulp_T(scale) over the loss's parameters and inexact-class
points, value and derivative separately, for the host (sr_host_elem_loss and the oracle's values) and, when a GPU is visible, the device
(every tier, unweighted and weighted, through loss_values_util.device_elements).  The bar is twice the maximum
rounded up to a whole unit (profiles/op_values_ulp.txt's rule).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "symbolicregression.jl_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import loss_values_util as U  # noqa: E402
import sr_amd  # noqa: E402


def measure(where):
    """{(bar name, dtype): [value max, derivative max, (spec, pred, target) of each]}"""
    out = {}
    for dtype_name in U.DTYPES:
        for spec in U.specs(dtype_name):
            pts = U.Points(dtype_name, spec)
            if pts.cls_name != "inexact":
                continue
            runs = []
            if where == "host":
                with np.errstate(all="ignore"):
                    v, d = U.host_elements(pts)
                runs.append((v, d))
                runs += [(U.oracle_values(pts, accum), d) for accum in ("ref", "f64")]  # (the oracle has no derivative)
            else:
                for tier in ("BASIC", "FULL"):
                    for weighted in (False, True):
                        runs.append(U.device_elements(pts, tier, weighted)[:2])
            m = out.setdefault((pts.bar_name, dtype_name), [0.0, 0.0, None, None])
            sel = pts.cls == U.INEXACT
            for v, d in runs:
                for i, err in enumerate(U.errors(pts, v, d)):
                    err = np.where(sel, err, 0.0)
                    k = int(np.argmax(err))
                    if err[k] > m[i]:
                        m[i], m[2 + i] = float(err[k]), (spec, float(pts.pred[k]), float(pts.target[k]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_values_ulp.txt"))
    args = ap.parse_args()
    lines = ["# max |got - fixture| in ulp_T(scale) over tests/golden/loss_values.json's inexact-class points, per loss (all its",
             "# parameters); value / derivative; bar = ceil(2 max).  host: sr_host_elem_loss and the oracle; device: MI355X (gfx950), every",
             "# tier, unweighted and weighted one-row views.  The worst point follows each pair.",
             "# where   loss       dtype      value   bar  derivative   bar   worst value point / worst derivative point"]
    for where in ["host"] + (["device"] if sr_amd.device_available() else []):
        for (name, dtype_name), (mv, md, wv, wd) in sorted(measure(where).items()):
            lines.append(f"  {where:<7} {name:<10} {dtype_name:<8} {mv:8.4f} {U.bar_of(mv):5d} {md:11.4f} {U.bar_of(md):5d}   {wv} / {wd}")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
