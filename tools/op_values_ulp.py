"""Measure, on the GPU, max |device - (hi + lo)| in ulps of T per inexact operator and dtype over the values of
tests/golden/op_values.json (tests/test_gpu_op_values.py: measure), and print the table kept as
profiles/op_values_ulp.txt and next to the bars in that test.

    python tools/op_values_ulp.py > profiles/op_values_ulp.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "symbolicregression.jl_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import test_gpu_op_values as t  # noqa: E402
from op_values_util import entry  # noqa: E402


def main():
    ver = "unknown"
    for p in ("/opt/rocm/.info/version", "/opt/rocm/.info/version-dev"):
        if os.path.exists(p):
            with open(p) as f:
                ver = f.read().strip()
            break
    print(f"# max |device - (hi + lo)| in ulps of T over tests/golden/op_values.json's values, MI355X (gfx950), ROCm {ver}")
    print(f"# {'operator':<12} {'float32':>10} {'float64':>10}")
    for degree, name in t.OPS:
        if not entry("float32", name, degree)["exact"]:
            m = [t.measure(dn, name, degree) for dn in ("float32", "float64")]
            print(f"  {name:<12} {m[0]:>10.4f} {m[1]:>10.4f}", flush=True)


if __name__ == "__main__":
    main()
