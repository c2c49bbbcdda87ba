"""CPU: the tuning-knob table (csrc/sr_knobs.h) — every knob's default, what sr_set_tuning stores or refuses
for it, the names sr_set_tuning and the environment accept, and the environment's rule (the same range,
clamped) — checked by a stand-alone program without a GPU.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sanitized_knob_program_runs_clean():
    """tools/knob_check.cpp (its own main, no HIP) built with -fsanitize=address,undefined."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "symbolicregression.jl_amd"), "knob-check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "knob_check: ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
