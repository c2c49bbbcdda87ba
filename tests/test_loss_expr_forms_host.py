"""CPU: every instruction form of the expression-loss program (csrc/sr_loss_expr.h) through the library's host
interpreter, bit for bit against an exact reference.

loss_expr_points.py holds a fixed table of bodies over the operators whose results are exact in T (+ - *, / by a
power of two or by w, neg abs square relu max min > < >= <= cond) and 60 seeded random ones, 32 points (multiples of
1/8, w in {0.5, 1, 2, 4}) at least 1/16 from every kink, and a recursive evaluator over fractions.Fraction whose
derivative is the exact central difference (degree in p at most 2: no derivative rule on the reference's side).
Every value, intermediate and derivative is exact in Float32 (asserted by the reference), so
``LossExpression.host_eval(..., deriv=True)`` must return the reference's bits in both dtypes — the sign of a zero
value included; a zero derivative by value (the central difference has no signed zero).

What the table covers is asserted from a restatement of the header's documented live-value rule
(loss_expr_points.plan).  test_gpu_loss_expr_forms.py runs the same table on the device.
"""
import numpy as np
import pytest

import loss_expr_points as lp
from op_values_util import bits
from sr_amd import LossExpression

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def refs():
    pts = lp.points()
    return {body: lp.reference(body, pts) for body in lp.table()}


def assert_elements(body, dtype, val, der, ref_val, ref_der):
    """Values bit for bit; derivatives bit for bit but for the sign of a zero."""
    want = ref_val.astype(dtype)
    bad = bits(np.asarray(val, dtype=dtype)) != bits(want)
    assert not bad.any(), (body, dtype.__name__, "value", np.nonzero(bad)[0], np.asarray(val)[bad], want[bad])
    if der is not None:
        wd = ref_der.astype(dtype)
        bad = ~((np.asarray(der) == wd) & ((wd == 0) | (bits(np.asarray(der, dtype=dtype)) == bits(wd))))
        assert not bad.any(), (body, dtype.__name__, "derivative", np.nonzero(bad)[0], np.asarray(der)[bad], wd[bad])


def test_the_points_and_the_table_meet_their_constraints():
    pts = lp.points()
    assert len(pts) == 32 and len(set(pts)) == 32
    for p, t, w in pts:
        assert (p * 8).denominator == 1 and (t * 8).denominator == 1 and abs(p) <= 4 and abs(t) <= 4
        assert float(w) in (0.5, 1.0, 2.0, 4.0)
    assert {float(w) for _, _, w in pts} == {0.5, 1.0, 2.0, 4.0}
    tab = lp.table()
    assert len(set(tab)) == len(tab)
    for body in tab:  # (no case dropped: every body of the table, the fixed ones too, is inside the constraints)
        e = lp.parse(body)
        assert lp.constants_ok(e) and lp.divisors_ok(e) and lp.mul_depth(e) <= 3 and lp.degree(e) <= 2, body
        assert lp.admissible(body, pts), body
        assert lp.parse(lp.render(e)) == e, body
        LossExpression(lp.spec(body))  # parses


def test_sixty_random_bodies_deterministically():
    a = lp.random_bodies()
    assert len(a) == 60 and len(set(a)) == 60
    lp.random_bodies.cache_clear()
    assert lp.random_bodies() == a
    plans = [lp.plan(b) for b in a]
    assert {pl["live"] for pl in plans} >= {1, 2, 3}
    assert sum(lp.uses_w(lp.parse(b)) for b in a) >= 10


def test_the_fixed_table_covers_every_form():
    plans = {b: lp.plan(b) for b in lp.FIXED}
    ins = [(b, i) for b, pl in plans.items() for i in pl["ins"]]
    kinds = {i[0] for _, i in ins}
    assert kinds == {"PUSH", "UNARY", "SS", "SW", "SL", "LS", "LL"}
    for kind in ("SS", "SW", "SL", "LS", "LL"):  # every binary kind with - and with /
        assert {"-", "/"} <= {i[1] for _, i in ins if i[0] == kind}, kind
    # SW with a non-commutative operator, in the issue's example body
    assert ("SW", "-", 1, 1, None, None) in plans["abs(p) - (abs(p - t) * abs(p + t))"]["ins"]
    # exactly 1, 2, 3 and 4 live values; the deeper ones with - at every level
    for n in (1, 2, 3, 4):
        pl = plans[lp._live(n)]
        assert pl["live"] == n and {i[1] for i in pl["ins"] if i[0] in ("SS", "SW")} <= {"-"}
        assert sum(i[0] == "SS" for i in pl["ins"]) == 2 ** (n - 1) - 1
    assert {pl["live"] for pl in plans.values()} == {1, 2, 3, 4}
    deep_sw = [b for b, pl in plans.items() if pl["live"] == 4 and any(i[0] == "SW" and i[1] == "-" for i in pl["ins"])]
    assert len(deep_sw) >= 2
    # all four DX / DY combinations for SS, SW and LL; both for SL, LS and UNARY
    for kind in ("SS", "SW", "LL"):
        assert {(i[2], i[3]) for _, i in ins if i[0] == kind} == {(0, 0), (0, 1), (1, 0), (1, 1)}, kind
    assert {i[2] for _, i in ins if i[0] == "SL"} == {0, 1} and {i[3] for _, i in ins if i[0] == "LS"} == {0, 1}
    assert {i[2] for _, i in ins if i[0] == "UNARY"} == {0, 1}
    # the weight and a constant as each leaf source
    assert {"w", "c", "p", "t"} <= {i[4] for _, i in ins if i[4]} and {"w", "c"} <= {i[5] for _, i in ins if i[5]}
    # a folded constant subtree; the 31-node chain
    assert sum(pl["folded"] > 0 for pl in plans.values()) >= 3
    chain = lp.chain31()
    assert lp.count_nodes(lp.parse(chain)) == 31 and plans[chain]["live"] == 1 and len(plans[chain]["ins"]) == 15
    assert LossExpression(lp.spec(chain)).batch().n_nodes == 31


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_interpreter_equals_the_exact_reference(dtype, refs):
    pts = lp.points()
    p, t, w = lp.arrays(pts, dtype)
    n = 0
    for body in lp.table():
        val, der = lp.host_elements(body, p, t, w, dtype)
        assert_elements(body, dtype, val, der, *refs[body])
        only = lp.LossExpression(lp.spec(body)).host_eval(*((p, t, w) if lp.uses_w(lp.parse(body)) else (p, t)))
        assert np.array_equal(bits(only), bits(val)), body  # the value pass and the derivative pass: the same bits
        n += 1
    assert n == len(lp.FIXED) + 60


# t ^ p at t = 0: sr_binary_partials gives pa = +Inf, pb = 0 there.  DX is clear (the base does not depend on the
# prediction), so the Inf must never meet the base's zero tangent: value 0, derivative exactly 0, not NaN.
POW_CASES = [("t ^ p", False), ("(w * 0.0) ^ p", True)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("body,weighted", POW_CASES)
def test_zero_base_power_has_a_zero_derivative(body, weighted, dtype):
    assert lp.uses_w(lp.parse(body)) == weighted
    pw = [i for i in lp.plan(body)["ins"] if i[1] == "^"]
    assert [(i[2], i[3]) for i in pw] == [(0, 1)]
    p, t, w = np.array([0.5], dtype=dtype), np.array([0.0], dtype=dtype), np.array([2.0], dtype=dtype)
    val, der = lp.host_elements(body, p, t, w, dtype)
    assert val[0] == 0 and not np.signbit(val[0]) and der[0] == 0, (body, val, der)
