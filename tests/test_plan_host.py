"""CPU: the batch engine's launch plan (csrc/sr_plan.h) — grids, chunk bounds, a chunk's launch order, code
layout, view segments and the in-order fold's path decision are integer arithmetic on host arrays, checked
by a stand-alone program without a GPU.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sanitized_plan_program_runs_clean():
    """tools/plan_check.cpp (its own main, no HIP) built with -fsanitize=address,undefined."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "symbolicregression.jl_amd"), "plan-check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "plan_check: ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
