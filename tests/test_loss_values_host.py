"""CPU: the loss-value fixture (tests/golden/loss_values.json: the 19 catalog losses with their parameters, value
and d loss / d prediction per point, mpmath at 60 digits from the published LossFunctions.jl definitions, on and
around every kink) against itself, against sr_host_elem_loss (csrc/sr_ops.h's sr_elem_loss / sr_elem_loss_deriv on
the host) and against the oracle's restatement (oracle/de_eval_impl.h::elem_loss), and parse_loss /
sr_register_loss on the specs and on parameters outside a loss's domain.

Bars.  The exact class (+ - * / and comparisons only) is bit-equal to the fixture, value and derivative, a zero's
sign apart.  The inexact class is within loss_values_util.BARS["host"] units of ulp_T(scale), scale being the
fixture's largest operand of an addition or result; the bars are twice the maxima measured here
(profiles/loss_values_ulp.txt).  An overflow point is +-Inf.
"""
import ctypes

import mpmath as mp
import numpy as np
import pytest

import loss_values_util as U
from sr_amd import Options, _lib
from sr_amd.options import parse_loss

CASES = [(d, s) for d in U.DTYPES for s in U.specs(d)]
IDS = [f"{d}:{s}" for d, s in CASES]
KINK_MARGIN = 2.0 ** -4


def test_the_fixture_is_what_its_maker_writes():
    """Regenerated and compared as text; the maker itself asserts that an exact-class value at a dyadic point is
    both the step-by-step T result and the correctly rounded 60-digit value."""
    assert U.maker().dumps(U.maker().build()) == U.fixture_text()


def test_the_fixture_holds_the_catalog():
    for dtype_name in U.DTYPES:
        fx = U.fixture()[dtype_name]
        assert sorted(fx) == sorted(U.specs(dtype_name))
        for spec, (kind, cls, param) in U.specs(dtype_name).items():
            assert fx[spec]["class"] == cls and 40 <= len(fx[spec]["points"]) <= 130, spec
            assert parse_loss(spec) == (kind, param), spec
    kinds = {k for k, _, _ in U.CATALOG.values()}
    assert kinds == set(range(19))


@pytest.mark.parametrize("dtype_name,spec", CASES, ids=IDS)
def test_exact_class_is_the_formula_step_by_step_in_T(dtype_name, spec):
    """Every exact-class expectation is the published formula evaluated step by step in T by numpy; at a dyadic
    point that is also the 60-digit value rounded once."""
    pts = U.Points(dtype_name, spec)
    if pts.cls_name != "exact":
        return
    m, T = U.maker(), pts.T
    name, P = m.CATALOG[spec]
    seen = 0
    for k in range(pts.n):
        with np.errstate(all="ignore"):
            v, g, _, _ = m.evaluate(name, None if P is None else T(P), pts.pred[k], pts.target[k], T, m._NP)
        assert U.bits(np.array([v, g], dtype=T)).tolist() == U.bits(np.array([pts.value[k], pts.deriv[k]], dtype=T)).tolist()
        if pts.dyadic[k] and pts.cls[k] == U.EXACT:
            mv, mg, _, _ = m.evaluate(name, None if P is None else mp.mpf(P), mp.mpf(float(pts.pred[k])), mp.mpf(float(pts.target[k])), mp.mpf, m._MP)
            assert m.round_to(mp.mpf(mv), T) == pts.value[k] and m.round_to(mp.mpf(mg), T) == pts.deriv[k], (spec, k)
            seen += 1
    assert seen >= 30, (spec, seen)


def _x(pts, k):
    """The variable the kinks are stated in: d = pred - target, or a = target * pred."""
    p, t = float(pts.pred[k]), float(pts.target[k])
    return t * p if pts.margin else p - t


def _kinks(pts):
    return [s * k for k in pts.kinks for s in (1, -1)] + [0.0]


@pytest.mark.parametrize("dtype_name,spec", CASES, ids=IDS)
def test_derivative_is_the_central_difference_of_the_value(dtype_name, spec):
    """No derivative formula on this side: (L(p + h) - L(p - h)) / 2h in mpmath at 60 digits, h = 2^-60, at every
    point farther than 2^-4 from a kink (d = 0 and a = 0 count as kinks).  The difference's own error is h^2 L'''/6,
    below 1e-30 here.  Tolerance: an inexact-class derivative is the rounded 60-digit value, half an ulp_T(scale);
    an exact-class one is the step-by-step T result, whose steps (pred - target or target * pred, one subtraction,
    one product) each round at most half an ulp of an operand no larger than max(|pred|, |target|, |derivative|, 1)
    times the constant factor 2 or 4 of the formula: 4 ulp_T of that magnitude."""
    pts = U.Points(dtype_name, spec)
    m, T = U.maker(), pts.T
    name, P = {**m.CATALOG, **m.F32_ONLY}[spec]
    Pm = None if P is None else mp.mpf(P)
    h = mp.mpf(2) ** -60
    checked = 0
    for k in range(pts.n):
        if pts.cls[k] == U.OVERFLOW or min(abs(_x(pts, k) - kk) for kk in _kinks(pts)) <= KINK_MARGIN:
            continue
        p, t = mp.mpf(float(pts.pred[k])), mp.mpf(float(pts.target[k]))
        fd = (m.evaluate(name, Pm, p + h, t, mp.mpf, m._MP)[0] - m.evaluate(name, Pm, p - h, t, mp.mpf, m._MP)[0]) / (2 * h)
        if pts.cls[k] == U.INEXACT:
            tol = 0.5 * float(U.ulp_of(pts.scale_d[k], T))
        else:
            tol = 4 * float(U.ulp_of(max(abs(float(pts.pred[k])), abs(float(pts.target[k])), abs(float(pts.deriv[k])), 1.0), T))
        assert abs(float(fd - mp.mpf(float(pts.deriv[k])))) <= tol * (1 + 1e-9), (spec, float(p), float(t), float(fd), pts.deriv[k])
        checked += 1
    assert checked >= 15, (spec, checked)


def _value_at(spec, dtype_name, pred, target):
    m = U.maker()
    name, P = {**m.CATALOG, **m.F32_ONLY}[spec]
    return m.evaluate(name, None if P is None else mp.mpf(P), mp.mpf(pred), mp.mpf(target), mp.mpf, m._MP)[0]


CONTINUOUS = [s for s in U.CATALOG if U.CATALOG[s][0] not in (9,)]  # (ZeroOne jumps at a = 0)


@pytest.mark.parametrize("spec", CONTINUOUS)
def test_value_is_continuous_across_each_kink(spec):
    """The fixture's own values one float on either side of a kink differ from the value on it by no more than
    the slope bound 4 (|target| <= 2.5 for a margin loss included: 10) times the step, plus an ulp of each."""
    for dtype_name, T in U.DTYPES.items():
        pts = U.Points(dtype_name, spec)
        val = pts.value.astype(np.float64)
        met = 0
        for kk in _kinks(pts):
            on = [k for k in range(pts.n) if _x(pts, k) == kk and pts.cls[k] != U.OVERFLOW]
            for k in on:
                near = [j for j in range(pts.n) if pts.target[j] == pts.target[k] and j != k and pts.cls[j] != U.OVERFLOW and
                        0 < abs(float(pts.pred[j]) - float(pts.pred[k])) <= 4 * float(np.spacing(np.abs(pts.pred[k])))]
                for j in near:
                    step = abs(float(pts.pred[j]) - float(pts.pred[k]))
                    slack = float(np.spacing(T(max(abs(val[k]), abs(val[j]))))) + float(U.ulp_of(max(pts.scale_v[k], pts.scale_v[j]), T))
                    assert abs(val[j] - val[k]) <= 10 * step * max(1.0, abs(float(pts.target[k])) ** 2) + 2 * slack, (spec, kk, pts.pred[k], pts.pred[j], val[k], val[j])
                    met += 1
        assert met >= (4 if pts.kinks else 0), (spec, met)


def _by_point(pts):
    return {(int(U.bits(pts.pred)[k]), int(U.bits(pts.target)[k])): k for k in range(pts.n)}


@pytest.mark.parametrize("dtype_name", list(U.DTYPES))
def test_identities_between_losses(dtype_name):
    """Where no formula is involved: L2Hinge = L1Hinge^2, L2EpsIns = L1EpsIns^2, Huber = L2 / 2 inside delta,
    Logit even in d, LP{2} = L2 and LP{1} = L1 — on the points the two entries share, the square taken in T."""
    T = U.DTYPES[dtype_name]
    P = lambda s: U.Points(dtype_name, s)  # noqa: E731

    def shared(a, b):
        ia, ib = _by_point(a), _by_point(b)
        keys = [k for k in ia if k in ib]
        return np.array([ia[k] for k in keys]), np.array([ib[k] for k in keys])

    for two, one in (("L2HingeLoss()", "L1HingeLoss()"), ("L2EpsilonInsLoss(0.25)", "L1EpsilonInsLoss(0.25)"),
                     ("L2EpsilonInsLoss(2.0)", "L1EpsilonInsLoss(2.0)")):
        a, b = P(two), P(one)
        ia, ib = shared(a, b)
        assert len(ia) == a.n == b.n
        assert np.array_equal(a.value[ia], (b.value[ib] * b.value[ib]).astype(T)), two
    for spec, delta in (("HuberLoss()", 1.0), ("HuberLoss(0.5)", 0.5)):
        a, b = P(spec), P("L2DistLoss()")
        ia, ib = shared(a, b)
        inside = np.abs(a.pred[ia] - a.target[ia]) <= delta
        assert inside.sum() >= 20
        assert np.array_equal(a.value[ia][inside], (b.value[ib][inside] / T(2)).astype(T)), spec
    lg = P("LogitDistLoss()")
    idx = _by_point(lg)
    zero = [k for k in range(lg.n) if lg.target[k] == 0 and lg.cls[k] == U.INEXACT]
    pairs = [(k, idx[(int(U.bits(np.array([-lg.pred[k]], dtype=T))[0]), int(U.bits(lg.target)[k]))]) for k in zero if lg.pred[k] > 0]
    pairs = [(k, j) for k, j in pairs if lg.cls[j] == U.INEXACT]
    assert len(pairs) >= 8
    assert all(lg.value[k] == lg.value[j] and lg.deriv[k] == -lg.deriv[j] for k, j in pairs)
    for lp, base in (("LPDistLoss{2}()", "L2DistLoss()"), ("LPDistLoss{1}()", "L1DistLoss()")):
        a, b = P(lp), P(base)
        ia, ib = shared(a, b)
        ok = (a.cls[ia] != U.OVERFLOW) & b.dyadic[ib]  # (a dyadic point: the exact class's value is the rounded one)
        assert ok.sum() >= 25
        assert np.array_equal(a.value[ia][ok], b.value[ib][ok]) and np.array_equal(a.deriv[ia][ok], b.deriv[ib][ok]), lp


@pytest.mark.parametrize("dtype_name,spec", CASES, ids=IDS)
def test_host_elem_loss_meets_the_fixture(dtype_name, spec):
    pts = U.Points(dtype_name, spec)
    with np.errstate(all="ignore"):
        v, d = U.host_elements(pts)
    U.assert_meets(pts, v, d, "host", (spec, dtype_name, "sr_host_elem_loss"))


@pytest.mark.parametrize("accum", ["ref", "f64"])
@pytest.mark.parametrize("dtype_name,spec", CASES, ids=IDS)
def test_oracle_meets_the_fixture(dtype_name, spec, accum):
    """One-row datasets (one per target), constant trees (one per prediction), both accumulation modes: the loss
    is the element's value."""
    pts = U.Points(dtype_name, spec)
    got = U.oracle_values(pts, accum)
    U.assert_meets(pts, got, pts.deriv, "host", (spec, dtype_name, "oracle", accum))  # (the oracle has no derivative)


def test_host_elem_loss_refuses_bad_arguments():
    z = np.zeros(1, dtype=np.float32)
    p = z.ctypes.data_as(ctypes.c_void_p)
    assert _lib.lib.sr_host_elem_loss(_lib.SR_DTYPE_F32, 19, 0.0, 1, p, p, p, p) == _lib.SR_ERR_INVALID_ARG
    assert _lib.lib.sr_host_elem_loss(_lib.SR_DTYPE_F32, -1, 0.0, 1, p, p, p, p) == _lib.SR_ERR_INVALID_ARG
    assert _lib.lib.sr_host_elem_loss(7, 0, 0.0, 1, p, p, p, p) == _lib.SR_ERR_INVALID_ARG
    assert _lib.lib.sr_host_elem_loss(_lib.SR_DTYPE_F32, 0, 0.0, 1, None, p, p, p) == _lib.SR_ERR_INVALID_ARG
    assert _lib.lib.sr_host_elem_loss(_lib.SR_DTYPE_F32, 0, 0.0, 0, None, None, None, None) == _lib.SR_OK


# ------------------------------------------------------------------------------------------------- parse_loss
def test_parse_loss_forms():
    assert parse_loss("LPDistLoss{3}()") == parse_loss("LPDistLoss(3)") == (2, 3.0)
    assert parse_loss("HuberLoss()") == (4, 1.0)
    assert parse_loss("QuantileLoss(-0.5)") == (8, -0.5) and parse_loss("QuantileLoss(0)") == (8, 0.0)  # tau: no bound
    for spec in ("LPDistLoss()", "L1EpsilonInsLoss()", "L2EpsilonInsLoss()", "PeriodicLoss()", "QuantileLoss()",
                 "SmoothedL1HingeLoss()", "DWDMarginLoss()"):
        with pytest.raises(ValueError, match="needs its parameter"):
            parse_loss(spec)
    for spec in ("L2DistLoss(1.0)", "L1DistLoss(2)", "LogitDistLoss(1)", "ZeroOneLoss(0.5)", "ExpLoss(1)", "L2HingeLoss{2}()"):
        with pytest.raises(ValueError, match="takes no parameter"):
            parse_loss(spec)


POSITIVE = ["HuberLoss", "L1EpsilonInsLoss", "L2EpsilonInsLoss", "PeriodicLoss", "SmoothedL1HingeLoss", "DWDMarginLoss", "LPDistLoss"]


@pytest.mark.parametrize("name", POSITIVE)
def test_parse_loss_refuses_a_parameter_outside_the_domain(name):
    for bad in ("0", "0.0", "-0.0", "-1.5", "nan", "inf"):
        with pytest.raises(ValueError, match="must be positive"):
            parse_loss(f"{name}({bad})")
        with pytest.raises(ValueError):
            Options(elementwise_loss=f"{name}({bad})", binary_operators=["+"], unary_operators=[])
    assert parse_loss(f"{name}(0.125)")[1] == 0.125


def test_bars_quote_the_measured_table():
    """loss_values_util.BARS is profiles/loss_values_ulp.txt's bar columns, each ceil(2 x the measured maximum)."""
    import os

    seen = 0
    with open(os.path.join(U.HERE, "..", "profiles", "loss_values_ulp.txt")) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            where, name, dtype_name, mv, bv, md, bd = line.split()[:7]
            assert (int(bv), int(bd)) == (U.bar_of(float(mv)), U.bar_of(float(md))), line
            assert U.BARS[where][dtype_name][name] == (int(bv), int(bd)), line
            assert float(mv) <= 4 and float(md) <= 4, line  # (above 4 units: a finding, not a bar)
            seen += 1
    assert seen == sum(len(d) for w in U.BARS.values() for d in w.values()) == 26
