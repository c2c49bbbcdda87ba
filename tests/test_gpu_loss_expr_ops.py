"""GPU: every operator of the catalog INSIDE a loss program, per value (csrc/sr_loss_expr.h: sr_lx_unary_rows /
sr_lx_binary_rows, the hand-written switch lists that exist only in the device build and whose ``default:`` returns
NaN — the host interpreter calls sr_unary directly and cannot show a missing or mis-indexed case).

Per operator the body is ``u(p)``, or ``b(p, t)`` and ``b(t, p)``; the points are tests/golden/op_values.json's
(mpmath at 60 digits; the special cases of the reference's definitions), through loss_expr_points.device_elements —
one one-row view per point, so each device value is one element's bits — in both dtypes and both tiers (the four
gathered expression-loss tile builds).

Every `values` point and every special point with finite arguments is used.  Left out are only the binary specials
with a non-finite argument (a dataset holds finite numbers): 2 of ^, max, min, > < >= <=, logical_or and
logical_and each, 18 per dtype; the test asserts exactly that set is skipped.

Bars: special points bit-exact (the sign of a zero included); where the fixture says `incomplete` the tree x1 is
complete and the loss non-finite; value points bit-equal for the exact class, else within test_gpu_op_values.BARS
(the loss program calls the same sr_unary / sr_binary as the tree interpreter).
"""
import numpy as np
import pytest

import loss_expr_points as lp
from op_values_util import BINARY, DTYPES, UNARY, bits, entry, rows, ulp_error
from test_gpu_op_values import BARS

pytestmark = pytest.mark.gpu

CASES = [(1, n, "p") for n in UNARY] + [(2, n, f) for n in BINARY for f in ("pt", "tp")]
IDS = [f"{'u' if d == 1 else 'b'}:{n}:{f}" for d, n, f in CASES]
# binary specials with a non-finite argument, per dtype
SKIPPED = {"^": 2, "max": 2, "min": 2, ">": 2, "<": 2, ">=": 2, "<=": 2, "logical_or": 2, "logical_and": 2}


def body_of(degree, name, form):
    if degree == 1:
        return f"{name}(p)"
    a, b = ("p", "t") if form == "pt" else ("t", "p")
    return f"{a} {name} {b}" if name in lp.INFIX else f"{name}({a}, {b})"


def used_points(dtype_name, name, degree):
    """(args, hi, lo, incomplete, special) of the points with finite arguments, and how many were left out."""
    args, hi, lo, inc = rows(dtype_name, name, degree)
    nv = len(entry(dtype_name, name, degree)["values"])
    fin = np.isfinite(args).all(axis=1)
    assert fin[:nv].all(), name  # every `values` point is used
    special = np.arange(len(args)) >= nv
    return args[fin], hi[fin], lo[fin], inc[fin], special[fin], int((~fin).sum())


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("tier", lp.TIERS)
@pytest.mark.parametrize("degree,name,form", CASES, ids=IDS)
def test_operator_inside_a_loss_program(degree, name, form, tier, dtype_name):
    T = DTYPES[dtype_name]
    exact = entry(dtype_name, name, degree)["exact"]
    bar = None if exact else BARS[name][0 if T == np.float32 else 1]
    args, hi, lo, inc, special, _ = used_points(dtype_name, name, degree)
    x = args[:, 0]
    y = args[:, 1] if degree == 2 else np.zeros(len(x), dtype=T)
    p, t = (x, y) if form != "tp" else (y, x)
    val, _, comp = lp.device_elements(body_of(degree, name, form), p, t, np.ones(len(x), dtype=T), T, tier, deriv=False)
    assert comp.all(), (name, args[~comp])  # the tree is x1: the loss decides nothing about completeness
    bad = inc & np.isfinite(val)
    assert not bad.any(), (name, "incomplete points must give a non-finite loss", args[bad], val[bad])
    want = hi.astype(T)
    bitwise = ~inc & (special | exact)
    bad = bitwise & (bits(val) != bits(want))
    assert not bad.any(), (name, dtype_name, tier, "bit-exact points", args[bad], val[bad], want[bad])
    rest = ~inc & ~bitwise
    if rest.any():
        err = ulp_error(T, val[rest], hi[rest], lo[rest])
        print(f"{name} {form} {dtype_name} {tier}: {int(rest.sum())} values, max ulp error {err.max():.4f} (bar {bar})")
        assert err.max() <= bar, (name, dtype_name, tier, args[rest][int(err.argmax())], float(err.max()))
        z = rest & (hi == 0)
        assert np.array_equal(np.signbit(val[z]), np.signbit(hi[z])), (name, args[z], val[z])


def test_exactly_the_non_finite_binary_specials_are_left_out():
    for dtype_name in DTYPES:
        skipped = {}
        for degree, name, form in CASES:
            if form != "tp":
                n = used_points(dtype_name, name, degree)[5]
                if n:
                    skipped[name] = n
        assert skipped == SKIPPED and sum(skipped.values()) == 18, (dtype_name, skipped)


def test_every_operator_of_the_catalog_has_a_body():
    assert len(UNARY) == 33 and len(BINARY) == 16 and len(CASES) == 33 + 2 * 16
    for degree, name, form in CASES:
        e = lp.parse(body_of(degree, name, form))
        assert e[1] == name and lp.plan(e)["ins"][-1][0] == ("UNARY" if degree == 1 else "LL")
