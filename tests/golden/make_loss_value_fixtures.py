"""Writes tests/golden/loss_values.json: the elementwise-loss catalog of csrc/sr_ops.h (sr_elem_loss,
sr_elem_loss_deriv) per point — value and d loss / d prediction, Float32 and Float64, on and around every kink.

    python tests/golden/make_loss_value_fixtures.py        (needs mpmath and numpy; no GPU)

Nothing here is imported from the library or the oracle.  LossFunctions.jl is not vendored under the reference, so
parity beyond L1 / L2 (which the reference's own test/unit/misc/test_losses.jl pins) rests on the definitions
LossFunctions.jl 0.11 publishes (src/losses/distance.jl, src/losses/margin.jl), restated here with
d = prediction - target and a = target * prediction:

    L2DistLoss            abs2(d)                                   deriv 2d
    L1DistLoss            abs(d)                                    deriv sign(d)
    LPDistLoss{P}         abs(d)^P                                  deriv d == 0 ? 0 : P d abs(d)^(P-2)
    LogitDistLoss         -log(4) - d + 2 log(1 + exp(d))           deriv tanh(d/2)
    HuberLoss(δ)          |d| <= δ ? 0.5 abs2(d) : δ|d| - 0.5 δ^2   deriv |d| <= δ ? d : δ sign(d)
    L1EpsilonInsLoss(ε)   max(0, |d| - ε)                           deriv |d| <= ε ? 0 : sign(d)
    L2EpsilonInsLoss(ε)   abs2(max(0, |d| - ε))                     deriv |d| <= ε ? 0 : 2 sign(d) (|d| - ε)
    PeriodicLoss(c)       1 - cos(d k), k = 2π/c                    deriv k sin(d k)
    QuantileLoss(τ)       d ((d > 0) - τ)                           deriv (d > 0) - τ
    ZeroOneLoss           sign(a) < 0 ? 1 : 0                       deriv 0
    PerceptronLoss        max(0, -a)                                deriv a >= 0 ? 0 : -1
    L1HingeLoss           max(0, 1 - a)                             deriv a >= 1 ? 0 : -1
    L2HingeLoss           a >= 1 ? 0 : abs2(1 - a)                  deriv a >= 1 ? 0 : 2 (a - 1)
    SmoothedL1HingeLoss(γ) a >= 1-γ ? 0.5/γ abs2(max(0, 1-a)) : 1 - γ/2 - a
                                                                    deriv a >= 1-γ ? (a >= 1 ? 0 : (a-1)/γ) : -1
    ModifiedHuberLoss     a >= -1 ? abs2(max(0, 1 - a)) : -4a       deriv a >= -1 ? (a > 1 ? 0 : 2a - 2) : -4
    L2MarginLoss          abs2(1 - a)                               deriv 2 (a - 1)
    ExpLoss               exp(-a)                                   deriv -exp(-a)
    SigmoidLoss           1 - tanh(a)                               deriv -abs2(sech(a))
    DWDMarginLoss(q)      a <= q/(q+1) ? 1 - a : (q^q/(q+1)^(q+1)) / a^q
                                                                    deriv a <= q/(q+1) ? -1 : -(q/(q+1))^(q+1) / a^(q+1)

The margin losses' derivative with respect to the prediction is target * deriv(a).  Every formula is written once
(`evaluate`) and run twice: over mpmath numbers at 60 digits (the value), and over numpy scalars of T, step by step
(what the published formula gives in T: the expectation of the exact class, and the overflow points).

{"float32" | "float64": {spec: {"class": "exact" | "inexact", "kinks": [..], "points": [
    [pred bits, target bits, value bits, derivative bits, value scale, derivative scale, class, dyadic], ...]}}}

  * bits: the unsigned integer holding the T value's bit pattern;
  * value / derivative: an exact-class loss: the step-by-step T result; an inexact-class loss: the 60-digit value
    correctly rounded to T; an overflow point: the step-by-step T result (+-Inf; the mathematical value is finite);
  * scale: the largest magnitude among the operands of the formula's additions and its result (log 4, d and
    2 log(1 + e^d) for Logit; 1 and d 2π/c for Periodic): errors are counted in ulp_T(scale); 0 for the exact class;
  * class: 0 exact, 1 inexact, 2 overflow (value or derivative of the step-by-step T formula is +-Inf);
  * dyadic: 1 where the nominal d (or a) is dyadic: there the exact class's step-by-step result is also the
    correctly rounded 60-digit value (asserted here and in the host test).

A kink's float neighbours are the two values of T on either side of the PREDICTION that puts d (or a) on the kink;
with target 0 (+-1 for a margin loss) these are d's (a's) own neighbours.  DWDMarginLoss's kink q/(q+1) is the
quotient rounded to T, not a dyadic number for q = 2 and 0.5; its two branches meet there.
"""
import json
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
HERE = os.path.dirname(os.path.abspath(__file__))
EXACT, INEXACT, OVERFLOW = 0, 1, 2

# spec -> (name, parameter or None, "dist" | "margin", exact class?)
CATALOG = {
    "L2DistLoss()": ("L2", None), "L1DistLoss()": ("L1", None),
    "LPDistLoss{3}()": ("LP", 3.0), "LPDistLoss(1.5)": ("LP", 1.5), "LPDistLoss{2}()": ("LP", 2.0), "LPDistLoss{1}()": ("LP", 1.0),
    "LogitDistLoss()": ("Logit", None), "HuberLoss()": ("Huber", 1.0), "HuberLoss(0.5)": ("Huber", 0.5),
    "L1EpsilonInsLoss(0.25)": ("L1Eps", 0.25), "L1EpsilonInsLoss(2.0)": ("L1Eps", 2.0),
    "L2EpsilonInsLoss(0.25)": ("L2Eps", 0.25), "L2EpsilonInsLoss(2.0)": ("L2Eps", 2.0),
    "PeriodicLoss(4.0)": ("Periodic", 4.0), "PeriodicLoss(0.5)": ("Periodic", 0.5),
    "QuantileLoss(0.25)": ("Quantile", 0.25), "QuantileLoss(0.75)": ("Quantile", 0.75),
    "ZeroOneLoss()": ("ZeroOne", None), "PerceptronLoss()": ("Perceptron", None), "L1HingeLoss()": ("L1Hinge", None),
    "L2HingeLoss()": ("L2Hinge", None), "SmoothedL1HingeLoss(0.5)": ("Smoothed", 0.5), "SmoothedL1HingeLoss(2.0)": ("Smoothed", 2.0),
    "ModifiedHuberLoss()": ("ModHuber", None), "L2MarginLoss()": ("L2Margin", None), "ExpLoss()": ("Exp", None),
    "SigmoidLoss()": ("Sigmoid", None), "DWDMarginLoss(1)": ("DWD", 1.0), "DWDMarginLoss(2)": ("DWD", 2.0),
    "DWDMarginLoss(0.5)": ("DWD", 0.5),
}
# Float32 only, held to the inexact bar: LossFunctions keeps the parameter in Float64, the device rounds it to T
F32_ONLY = {"HuberLoss(0.3)": ("Huber", 0.3)}
MARGIN = ("ZeroOne", "Perceptron", "L1Hinge", "L2Hinge", "Smoothed", "ModHuber", "L2Margin", "Exp", "Sigmoid", "DWD")
INEXACT_NAMES = ("LP", "Logit", "Periodic", "Exp", "Sigmoid", "DWD")


class _MP:
    exp, log, cos, sin, tanh = mp.exp, mp.log, mp.cos, mp.sin, mp.tanh
    pow = staticmethod(lambda x, y: mp.power(x, y))
    pi = mp.pi


class _NP:
    exp, log, cos, sin, tanh, pow = np.exp, np.log, np.cos, np.sin, np.tanh, np.power
    pi = np.pi


def evaluate(name, P, pred, target, T, F):
    """(value, d value / d pred, value scale, derivative scale) of the published formula; T converts a constant,
    F holds the functions.  Every operation is one of T's own, in the published order."""
    d = pred - target
    a = target * pred
    ad = abs(d)
    zero, one, two, half = T(0), T(1), T(2), T(0.5)
    sgn = one if d > 0 else (-one if d < 0 else zero)
    mag = lambda *v: max(abs(float(x)) for x in v)  # noqa: E731
    if name == "L2":
        return d * d, two * d, 0, 0
    if name == "L1":
        return ad, sgn, 0, 0
    if name == "LP":
        v = F.pow(ad, P)
        g = zero if d == 0 else P * d * F.pow(ad, P - two)
        return v, g, mag(v), mag(g)
    if name == "Logit":
        er = F.exp(d)
        s = two * F.log(one + er)
        c = F.log(T(4))
        v = -c - d + s
        g = F.tanh(d / two)
        return v, g, mag(c, d, s, v), mag(g)
    if name == "Huber":
        if ad <= P:
            v = half * (d * d)
            return v, d, mag(v), mag(d)
        v = P * ad - half * (P * P)
        return v, P * sgn, mag(P * ad, v), mag(P)
    if name == "L1Eps":
        e = ad - P
        return (e if e > 0 else zero), (zero if ad <= P else sgn), 0, 0
    if name == "L2Eps":
        e = ad - P
        e = e if e > 0 else zero
        return e * e, (zero if ad <= P else two * sgn * (ad - P)), 0, 0
    if name == "Periodic":
        k = two * T(F.pi) / P
        x = d * k
        v = one - F.cos(x)
        g = k * F.sin(x)
        return v, g, mag(one, x, v), mag(k * x, k, g)
    if name == "Quantile":
        q = (one if d > 0 else zero) - P
        return d * q, q, 0, 0
    # margin losses: d/dpred = target * deriv(a)
    if name == "ZeroOne":
        return (one if a < 0 else zero), zero * target, 0, 0
    if name == "Perceptron":
        return (-a if -a > 0 else zero), (zero if a >= 0 else -one) * target, 0, 0
    if name == "L1Hinge":
        e = one - a
        return (e if e > 0 else zero), (zero if a >= 1 else -one) * target, 0, 0
    if name == "L2Hinge":
        e = one - a
        return (zero if a >= 1 else e * e), (zero if a >= 1 else two * (a - one)) * target, 0, 0
    if name == "Smoothed":
        if a >= one - P:
            e = one - a
            e = e if e > 0 else zero
            return half / P * (e * e), (zero if a >= 1 else (a - one) / P) * target, 0, 0
        return one - P / two - a, -one * target, 0, 0
    if name == "ModHuber":
        if a >= -1:
            e = one - a
            e = e if e > 0 else zero
            return e * e, (zero if a > 1 else two * a - two) * target, 0, 0
        return T(-4) * a, T(-4) * target, 0, 0
    if name == "L2Margin":
        e = one - a
        return e * e, two * (a - one) * target, 0, 0
    if name == "Exp":
        v = F.exp(-a)
        return v, -v * target, mag(v), mag(v * target)
    if name == "Sigmoid":
        t = F.tanh(a)
        v = one - t
        g = -(one - t * t) * target  # abs2(sech(a)) = 1 - tanh(a)^2
        return v, g, mag(one, v), mag(target, g)
    if name == "DWD":
        if a <= P / (P + one):
            return one - a, -one * target, mag(one, a, one - a), mag(target)
        c = F.pow(P, P) / F.pow(P + one, P + one)
        v = c / F.pow(a, P)
        g = -F.pow(P / (P + one), P + one) / F.pow(a, P + one) * target
        return v, g, mag(v), mag(g)
    raise ValueError(name)


def kinks(name, P, T):
    """The kinks in d (distance) or a (margin), as values of T."""
    if name in ("Huber", "L1Eps", "L2Eps"):
        return [T(P)]
    if name in ("L1Hinge", "L2Hinge"):
        return [T(1)]
    if name == "Smoothed":
        return [T(1), T(1) - T(P)]
    if name == "ModHuber":
        return [T(1), T(-1)]
    if name == "DWD":
        return [T(P) / (T(P) + T(1))]
    return []  # (d = 0 and a = 0 are points of every loss)


def _neighbours(x, T):
    up = np.nextafter(x, T(np.inf))
    dn = np.nextafter(x, T(-np.inf))
    return [np.nextafter(dn, T(-np.inf)), dn, up, np.nextafter(up, T(np.inf))]


def points(name, P, T):
    """[(pred, target, dyadic)] as values of T, distinct by bit pattern."""
    f32 = T == np.float32
    ks = [float(k) for k in kinks(name, P, T)]
    out, seen = [], set()

    def add(pred, t, dy):
        key = (float(pred).hex(), float(t).hex())
        if key not in seen and np.isfinite(pred):
            seen.add(key)
            out.append((T(pred), T(t), dy))

    if name not in MARGIN:
        dy = [0.0, 2.0 ** -20, 0.5, 1.0, 3.0, 20.0] + [abs(k) for k in ks]
        non = [0.3, 0.7]
        if name == "Logit":
            dy += [80.0, 100.0]
        one_sided = [1000.0, 12345.678] if name == "Periodic" else []
        if name in ("LP", "L2") and f32:
            one_sided.append(1e20)
        for t in (0.0, 1.0, -2.5):
            for d in dy:
                for s in (1, -1):
                    add(T(t) + T(s * d), t, 1)
            for d in non:
                for s in (1, -1):
                    add(T(t) + T(s * d), t, 0)
            for d in one_sided:
                add(T(t) + T(d), t, 0)
            for k in ks:
                for s in (1, -1):
                    for nb in _neighbours(T(t) + T(s * k), T):
                        add(nb, t, int(t == 0))  # (pred - target rounds beside another target)
    else:
        dy = [2.0 ** -20, 0.25, 3.0, 20.0] + [abs(k) for k in ks]
        for t in (1.0, -1.0, 0.5, -2.0):
            add(T(0.0), t, 1), add(T(-0.0), t, 1)  # a = 0 from both signs
            for a in dy:
                for s in (1, -1):
                    add(T(s * a) / T(t), t, 1)
            for a in (0.3, -0.7):
                add(T(a) / T(t), t, 0)
            if name == "Exp":
                add(T(100.0) / T(t), t, 1), add(T(-100.0) / T(t), t, 1)
            for k in ks:
                for s in (1, -1):
                    for nb in _neighbours(T(s * k) / T(t), T):
                        add(nb, t, 0)  # (1 - a may round)
    return out


def bits(x, T):
    return int(np.array([x], dtype=T).view(np.uint32 if T == np.float32 else np.uint64)[0])


def round_to(v, T):
    """The mpmath number correctly rounded to T (ties to even; the subnormal range and overflow included)."""
    f = np.finfo(T)
    if v == 0:
        return T(0)
    if abs(v) < mp.mpf(float(f.tiny)):
        q = mp.mpf(float(f.smallest_subnormal))
        return T(float(mp.nint(v / q) * q))
    with mp.workprec(f.nmant + 1):
        r = +v
    if abs(r) > mp.mpf(float(f.max)):
        return T(np.inf) if r > 0 else T(-np.inf)
    return T(float(r))


def entry(name, P, T, rounded_parameter=False):
    """`rounded_parameter`: P is no value of T.  The 60-digit value keeps it in Float64, as LossFunctions does; the
    entry is of the inexact class."""
    exact = name not in INEXACT_NAMES and not rounded_parameter
    rows = []
    for pred, t, dy in points(name, P, T):
        mv, mg, sv, sg = evaluate(name, None if P is None else mp.mpf(P), mp.mpf(float(pred)), mp.mpf(float(t)), mp.mpf, _MP)
        with np.errstate(all="ignore"):
            nv, ng, _, _ = evaluate(name, None if P is None else T(P), pred, t, T, _NP)
        nv, ng = T(nv), T(ng)
        assert not (np.isnan(nv) or np.isnan(ng)), (name, P, pred, t)
        cv, cg = round_to(mp.mpf(mv), T), round_to(mp.mpf(mg), T)
        if np.isinf(nv) or np.isinf(ng):
            # the formula overflows in T step by step; the mathematical value is finite (asserted)
            assert mp.isfinite(mv) and mp.isfinite(mg), (name, pred, t)
            cls = OVERFLOW
            val, der = nv, (ng if np.isinf(ng) or exact else cg)
        elif exact:
            cls = EXACT
            val, der = nv, ng
            if dy:  # a dyadic point: no step of the formula rounds more than the value itself does
                assert (val == cv and der == cg), (name, P, float(pred), float(t), val, cv, der, cg)
        else:
            cls = INEXACT
            val, der = cv, cg
            assert np.isfinite(val) and np.isfinite(der), (name, pred, t)
        if not exact and (cls == INEXACT):
            slack = float(np.finfo(T).smallest_subnormal)  # (a subnormal result may round up past its own magnitude)
            assert sv >= abs(float(val)) * (1 - 1e-6) - slack and sg >= abs(float(der)) * (1 - 1e-6) - slack, (name, pred, t, sv, sg)
        if exact:
            sv = sg = 0
        rows.append([bits(pred, T), bits(t, T), bits(val, T), bits(der, T), float(sv), float(sg), cls, dy if exact else 0])
    return {"class": "exact" if exact else "inexact", "kinks": [float(k) for k in kinks(name, P, T)], "points": rows}


def build():
    out = {}
    for tname, T in (("float32", np.float32), ("float64", np.float64)):
        specs = dict(CATALOG)
        if T == np.float32:
            specs.update(F32_ONLY)
        out[tname] = {}
        for spec, (name, P) in specs.items():
            out[tname][spec] = entry(name, P, T, rounded_parameter=spec in F32_ONLY)
    return out


def dumps(out):
    return json.dumps(out, separators=(",", ":")) + "\n"


def main():
    path = os.path.join(HERE, "loss_values.json")
    with open(path, "w") as fh:
        fh.write(dumps(build()))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
