"""Writes tests/golden/op_values.json: per operator of csrc/sr_ops.h (33 unary, 16 binary) and element type,
points with their 60-digit value (mpmath) and the special cases of the reference's definitions.

    python tests/golden/make_op_value_fixtures.py        (needs mpmath and numpy; no GPU)

{"float32" | "float64": {"unary" | "binary": {name: {
    "exact":   true for the operators whose result is an IEEE operation in T (bit-equal), else false,
    "values":  [[x, (y,) hi, lo], ...] at most 64 in-domain points with a finite result: hi + lo is the value to
               60 digits (hi the nearest Float64; an exact-class operator: hi is the result in T, lo 0),
    "special": [[x, (y,) expected, citation], ...] every number a string float() reads ("-0.0", "nan", "inf");
               expected: the exact result in T, sign of zero included, or "incomplete" (the result is NaN or
               +-Inf, which is_valid_array refuses whatever the tree around it) }}}}

The special cases restate, and cite, the reference: src/Operators.jl 14-17 (gamma), 35-49 (safe_pow), 50-76 (the
safe_ functions), 81-82 (square, cube), 98-124 (comparisons, cond, relu, logical_*), and Julia Base's mod, max,
min, round, sign for floats.  Inputs are finite except where the result is NaN whatever the evaluation order
(max / min of a NaN) and the comparisons' NaN rows, whose value is 0.0.
"""
import json
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
HERE = os.path.dirname(os.path.abspath(__file__))
OPS = "src/Operators.jl"


UNARY_FN = {
    "exp": mp.exp, "cos": mp.cos, "sin": mp.sin, "tan": mp.tan, "log": mp.log, "log2": lambda x: mp.log(x, 2),
    "log10": mp.log10, "log1p": mp.log1p, "tanh": mp.tanh, "sinh": mp.sinh, "cosh": mp.cosh, "atan": mp.atan,
    "asin": mp.asin, "acos": mp.acos, "acosh": mp.acosh, "atanh": mp.atanh, "asinh": mp.asinh, "erf": mp.erf,
    "erfc": mp.erfc, "gamma": mp.gamma, "exp2": lambda x: mp.power(2, x), "expm1": mp.expm1,
}
BINARY_FN = {"^": mp.power, "atan2": mp.atan2}


def _mod(x, y):
    """Base.mod(x::T, y::T) for floats: r = rem(x, y); r == 0 -> copysign(r, y); signs differ -> r + y."""
    with np.errstate(all="ignore"):
        r = np.fmod(x, y)
        if r == 0:
            return np.copysign(r, y)
        return r + y if (r > 0) != (y > 0) else r


def _exact_unary(T):
    z = T(0)
    return {
        "neg": lambda x: -x, "square": lambda x: x * x, "cube": lambda x: (x * x) * x, "abs": lambda x: np.abs(x),
        "sign": lambda x: np.sign(x) if x != 0 else x, "relu": lambda x: x if x > 0 else np.copysign(z, x),
        "inv": lambda x: T(1) / x, "round": lambda x: np.rint(x), "floor": lambda x: np.floor(x),
        "ceil": lambda x: np.ceil(x), "sqrt": lambda x: np.sqrt(x),
    }


def _exact_binary(T):
    z, one = T(0), T(1)
    return {
        "+": lambda x, y: x + y, "-": lambda x, y: x - y, "*": lambda x, y: x * y, "/": lambda x, y: x / y,
        "max": lambda x, y: y if (y > x or (np.signbit(x) and not np.signbit(y) and x == y)) else x,
        "min": lambda x, y: y if (y < x or (np.signbit(y) and not np.signbit(x) and x == y)) else x,
        "mod": _mod, ">": lambda x, y: one if x > y else z, "<": lambda x, y: one if x < y else z,
        ">=": lambda x, y: one if x >= y else z, "<=": lambda x, y: one if x <= y else z,
        "cond": lambda x, y: y if x > 0 else np.copysign(z, y),
        "logical_or": lambda x, y: one if (x > 0 or y > 0) else z,
        "logical_and": lambda x, y: one if (x > 0 and y > 0) else z,
    }


def _hl(v):
    hi = float(v)
    return hi, float(v - mp.mpf(hi))


def unary_points(name, T):
    """In-domain points of a unary operator, as values of T."""
    f = np.finfo(T)
    f32 = T == np.float32
    up = lambda x: np.nextafter(T(x), T(np.inf))    # noqa: E731
    dn = lambda x: np.nextafter(T(x), T(-np.inf))   # noqa: E731
    tiny = [T(2.0 ** -k) for k in (10, 20, 30, 60, 100)] + [f.tiny]
    sym = lambda v: list(v) + [-T(x) for x in v]    # noqa: E731
    mid = [0.1, 0.5, 0.9, 1.0, 1.5, 2.0, 3.0, 7.5, 10.0, 20.0]
    log_ovf = np.log(float(f.max))                  # 88.72 / 709.78
    P = {
        "exp": sym(tiny[:4] + mid) + [dn(log_ovf), -log_ovf, T(-log_ovf - 10)],
        "exp2": sym(tiny[:4] + mid) + [dn(127.99 if f32 else 1023.99), T(-140 if f32 else -1060), 0.5, -0.5],
        "expm1": sym(tiny + mid) + [dn(log_ovf), -40.0],
        "cos": sym(tiny[:3] + mid + [np.pi / 2, np.pi, 3 * np.pi / 2, 100.0, 1e5, 3e6, 1e10, 1e30]),
        "sin": sym(tiny[:3] + mid + [np.pi / 2, np.pi, 3 * np.pi / 2, 100.0, 1e5, 3e6, 1e10, 1e30]),
        "tan": sym(tiny[:3] + mid + [np.pi / 2, up(np.pi / 2), dn(np.pi / 2), 3 * np.pi / 2, 5 * np.pi / 2, 101 * np.pi / 2, 1e5, 1e10]),
        "log": [f.tiny, f.smallest_subnormal, f.max, dn(1), up(1), 1 + 2.0 ** -10, 1 - 2.0 ** -10, np.e] + mid + tiny[:4] + [1e10, 1e30],
        "log2": [f.tiny, f.smallest_subnormal, f.max, dn(1), up(1), 1 + 2.0 ** -10, 1 - 2.0 ** -10, 8.0, 2.0 ** -30] + mid + [1e10, 1e30],
        "log10": [f.tiny, f.smallest_subnormal, f.max, dn(1), up(1), 1 + 2.0 ** -10, 1 - 2.0 ** -10, 1000.0, 1e-5] + mid + [1e10, 1e30],
        "log1p": sym(tiny) + [up(-1), -0.5, -0.9, -0.999] + mid + [1e10, f.max],
        "tanh": sym(tiny + mid + [8.0, 9.5, 19.0, 40.0]),
        "sinh": sym(tiny + mid + [dn(log_ovf), log_ovf - 1]),
        "cosh": sym(tiny[:2] + mid + [dn(log_ovf), log_ovf - 1]),
        "atan": sym(tiny + mid + [1e5, 1e20, f.max]),
        "asin": sym(tiny + [0.1, 0.5, 0.9, 0.99, 0.9999, dn(1), 1.0]),
        "acos": sym(tiny[:3] + [0.1, 0.5, 0.9, 0.99, 0.9999, dn(1)]) + [-1.0],
        "acosh": [up(1), 1 + 2.0 ** -10, 1 + 2.0 ** -20, 1.5, 2.0, 10.0, 1e5, 1e20, f.max],
        "atanh": sym(tiny + [0.1, 0.5, 0.9, 0.99, 0.9999, dn(1)]),
        "asinh": sym(tiny + mid + [1e5, 1e20, f.max]),
        "erf": sym(tiny + mid[:8] + [3.5, 4.0, 6.0]),
        "erfc": sym(tiny[:3] + mid[:8]) + [4.0, 6.0, 9.0, 10.0] + ([] if f32 else [20.0, 26.0, 26.5, 26.6, 27.0]),
        "gamma": [tiny[0], tiny[2], 0.5, 1.0, 1.5, 2.0, 3.0, 5.0, 10.5, 20.0, 30.0, 34.5 if f32 else 170.5, 35.0 if f32 else 171.0,
                  -0.5, -1.5, -2.5, -10.5, dn(-1), up(-1), dn(-2), up(-3), -tiny[0], -20.5],
        # the exact class
        "neg": sym([0.0] + tiny + mid + [f.max]), "abs": sym([0.0] + tiny + mid + [f.max]),
        "square": sym(tiny[:4] + mid + [1e10, 1 + 2.0 ** -12, 1 / 3]), "cube": sym(tiny[:3] + mid + [1e10, 1 + 2.0 ** -8, 1 / 3]),
        "sign": sym(tiny + mid + [f.max]), "relu": sym(tiny + mid + [f.max]),
        "inv": sym(tiny[:4] + mid + [1e10, 1 / 3, f.max / 4]),
        "round": sym([0.25, 0.5, 0.75, 1.5, 2.5, 3.5, 1e5 + 0.5, 2.0 ** (23 if f32 else 52) - 0.5, 2.0 ** (23 if f32 else 52) + 1, 1e30]),
        "floor": sym([0.25, 0.5, 0.75, 1.5, 2.5, 3.0, 1e5 + 0.5, 2.0 ** (23 if f32 else 52) - 0.5, 1e30]),
        "ceil": sym([0.25, 0.5, 0.75, 1.5, 2.5, 3.0, 1e5 + 0.5, 2.0 ** (23 if f32 else 52) - 0.5, 1e30])[:-1],
        "sqrt": [0.0, f.smallest_subnormal, f.tiny, f.max, 2.0, 3.0, 1 / 3, 1e10, 1e-10] + mid + tiny,
    }
    with np.errstate(all="ignore"):
        return [T(x) for x in P[name]]


def binary_points(name, T):
    f = np.finfo(T)
    f32 = T == np.float32
    mags = [0.5, 1.0, 1.5, 3.0, 1 / 3, 1e-3, 1e3, 1e10, 1e-10]
    cross = [(s * a, t * b) for a in mags[:6] for b in mags[:6] for s in (1, -1) for t in (1, -1)][:48]
    if name == "atan2":  # every quadrant and every axis
        pts = cross[:40] + [(0.0, 1.0), (0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (-0.0, 1.0), (-0.0, -1.0), (1.0, -0.0), (-1.0, -0.0),
                            (1e-30, 1e30), (1e30, 1e-30), (-1e30, -1e-30), (1e-20, -1e20)]
    elif name == "^":  # positive bases; negative bases with integer exponents; roots; large results
        pts = [(a, b) for a in (0.5, 1.5, 3.0, 1 / 3, 10.0, 1e-3) for b in (0.5, -0.5, 1.5, 3.0, -2.0, 1 / 3)] + \
              [(-2.0, 3.0), (-2.0, -2.0), (-1.5, 5.0), (-3.0, 4.0), (-1 / 3, 3.0), (-10.0, -3.0), (-1.5, 21.0), (-1.5, 20.0),
               (2.0, 100.0 if f32 else 1000.0), (2.0, -140.0 if f32 else -1060.0), (1 + 2.0 ** -10, 1000.0), (1e10, 3.0 if f32 else 30.0),
               (0.0, 0.5), (0.0, 3.0), (10.0, -30.0)]
    elif name == "mod":
        pts = cross[:40] + [(5.0, 3.0), (-5.0, 3.0), (5.0, -3.0), (-5.0, -3.0), (1e10, 3.0), (-1e10, 3.0), (0.5, 1e10), (-0.5, 1e10),
                            (7.5, 2.5), (1e3, 1 / 3)]
    else:
        pts = cross + [(1.0, 1.0), (-1.0, -1.0), (0.0, 1.0), (1.0, 0.0), (0.0, 0.0), (1e10, 1e-10), (-1e10, 1e10), (float(f.max) / 4, 2.0),
                       (float(f.tiny), 0.5), (1 / 3, 3.0)]
        if name == "/":
            pts = [p for p in pts if p[1] != 0]
    return [(T(a), T(b)) for a, b in pts][:64]


def _s(v):
    return repr(float(v))


def unary_special(name, T):
    """[x, expected, citation] in T: exact results (sign of zero included) and incomplete points."""
    f = np.finfo(T)
    up = lambda x: np.nextafter(T(x), T(np.inf))    # noqa: E731
    dn = lambda x: np.nextafter(T(x), T(-np.inf))   # noqa: E731
    big_int = 2.0 ** (23 if T == np.float32 else 52) + 1
    INC = "incomplete"
    S = {
        "gamma": [(0.0, INC, f"{OPS}:14-17 gamma(0) = Inf -> NaN"), (-0.0, INC, f"{OPS}:14-17 gamma(-0) = -Inf -> NaN"),
                  (-1.0, INC, f"{OPS}:14-17 a pole"), (-3.0, INC, f"{OPS}:14-17 a pole"),
                  (36.0 if T == np.float32 else 172.0, INC, f"{OPS}:14-17 overflow: Inf -> NaN"), (1.0, 1.0, "gamma(1) = 1"),
                  (5.0, 24.0, "gamma(5) = 4!")],
        "round": [(0.5, 0.0, "Base.round: RoundNearest, ties to even"), (1.5, 2.0, "ties to even"), (2.5, 2.0, "ties to even"),
                  (-0.5, -0.0, "round(-0.5) = -0.0"), (-1.5, -2.0, "ties to even"), (big_int, big_int, "every value this large is an integer"),
                  (0.0, 0.0, "round(0.0)"), (-0.0, -0.0, "round(-0.0)")],
        "floor": [(-0.5, -1.0, "Base.floor"), (0.5, 0.0, "Base.floor"), (-0.0, -0.0, "floor(-0.0) = -0.0"), (big_int, big_int, "an integer")],
        "ceil": [(-0.5, -0.0, "Base.ceil: ceil(-0.5) = -0.0"), (0.5, 1.0, "Base.ceil"), (-0.0, -0.0, "ceil(-0.0)"), (big_int, big_int, "an integer")],
        "relu": [(-3.0, -0.0, f"{OPS}:115 (x > 0) * x: false * x = copysign(0, x)"), (3.0, 3.0, f"{OPS}:115"), (0.0, 0.0, f"{OPS}:115"),
                 (-0.0, -0.0, f"{OPS}:115")],
        "sign": [(0.0, 0.0, "Base.sign(0.0) = 0.0"), (-0.0, -0.0, "Base.sign(-0.0) = -0.0"), (-3.0, -1.0, "Base.sign"), (f.tiny, 1.0, "Base.sign")],
        "abs": [(-0.0, 0.0, "abs(-0.0) = 0.0"), (0.0, 0.0, "abs(0.0)"), (-f.max, f.max, "abs")],
        "neg": [(0.0, -0.0, "-(0.0) = -0.0"), (-0.0, 0.0, "-(-0.0) = 0.0")],
        "square": [(-0.0, 0.0, f"{OPS}:81 x * x"), (f.tiny, 0.0, "underflow to 0.0"), (f.max, INC, "overflow")],
        "cube": [(-0.0, -0.0, f"{OPS}:82 x ^ 3"), (-f.tiny, -0.0, "underflow to -0.0"), (f.max, INC, "overflow")],
        "sqrt": [(-0.0, -0.0, f"{OPS}:74-76 safe_sqrt: -0.0 >= 0, sqrt(-0.0) = -0.0"), (0.0, 0.0, "sqrt(0.0)"), (4.0, 2.0, "sqrt(4)"),
                 (-f.smallest_subnormal, INC, f"{OPS}:74-76 x < 0 -> NaN"), (-1.0, INC, f"{OPS}:74-76 x < 0 -> NaN")],
        "inv": [(0.0, INC, "1 / 0.0 = Inf"), (-0.0, INC, "1 / -0.0 = -Inf"), (4.0, 0.25, "1 / 4"), (-0.5, -2.0, "1 / -0.5")],
        "log": [(0.0, INC, f"{OPS}:50-52 safe_log: x <= 0 -> NaN"), (-0.0, INC, f"{OPS}:50-52"), (-1.0, INC, f"{OPS}:50-52"), (1.0, 0.0, "log(1) = 0.0")],
        "log2": [(0.0, INC, f"{OPS}:53-55 safe_log2: x <= 0 -> NaN"), (-1.0, INC, f"{OPS}:53-55"), (1.0, 0.0, "log2(1)"), (8.0, 3.0, "log2(8) = 3"),
                 (2.0 ** -100, -100.0, "log2 of a power of two")],
        "log10": [(0.0, INC, f"{OPS}:56-58 safe_log10: x <= 0 -> NaN"), (-1.0, INC, f"{OPS}:56-58"), (1.0, 0.0, "log10(1)"), (1000.0, 3.0, "log10(1000) = 3")],
        "log1p": [(-1.0, INC, f"{OPS}:59-61 safe_log1p: log1p(-1) = -Inf"), (dn(-1), INC, f"{OPS}:59-61 x < -1 -> NaN"), (-2.0, INC, f"{OPS}:59-61"),
                  (0.0, 0.0, "log1p(0.0)"), (-0.0, -0.0, "log1p(-0.0) = -0.0")],
        "asin": [(up(1), INC, f"{OPS}:62-64 safe_asin: |x| > 1 -> NaN"), (dn(-1), INC, f"{OPS}:62-64"), (0.0, 0.0, "asin(0.0)"), (-0.0, -0.0, "asin(-0.0)")],
        "acos": [(up(1), INC, f"{OPS}:65-67 safe_acos: |x| > 1 -> NaN"), (dn(-1), INC, f"{OPS}:65-67"), (1.0, 0.0, "acos(1) = 0.0: the closed end")],
        "acosh": [(1.0, 0.0, f"{OPS}:68-70 safe_acosh: x >= 1, acosh(1) = 0.0: the closed end"), (dn(1), INC, f"{OPS}:68-70 x < 1 -> NaN"),
                  (0.0, INC, f"{OPS}:68-70"), (-2.0, INC, f"{OPS}:68-70")],
        "atanh": [(1.0, INC, f"{OPS}:71-73 safe_atanh: atanh(1) = Inf"), (-1.0, INC, f"{OPS}:71-73 atanh(-1) = -Inf"), (up(1), INC, f"{OPS}:71-73 |x| > 1 -> NaN"),
                  (dn(-1), INC, f"{OPS}:71-73"), (0.0, 0.0, "atanh(0.0)"), (-0.0, -0.0, "atanh(-0.0)")],
        "exp": [(0.0, 1.0, "exp(0)"), (-0.0, 1.0, "exp(-0.0)"), (89.0 if T == np.float32 else 710.0, INC, "overflow"),
                (-104.0 if T == np.float32 else -746.0, 0.0, "underflow to 0.0")],
        "exp2": [(0.0, 1.0, "exp2(0)"), (10.0, 1024.0, "exp2(10)"), (-1.0, 0.5, "exp2(-1)"), (128.0 if T == np.float32 else 1024.0, INC, "overflow"),
                 (-126.0 if T == np.float32 else -1022.0, f.tiny, "exp2 of the smallest normal exponent")],
        "expm1": [(0.0, 0.0, "expm1(0.0)"), (-0.0, -0.0, "expm1(-0.0) = -0.0"), (89.0 if T == np.float32 else 710.0, INC, "overflow")],
        "cos": [(0.0, 1.0, "cos(0)"), (-0.0, 1.0, "cos(-0.0)")], "sin": [(0.0, 0.0, "sin(0.0)"), (-0.0, -0.0, "sin(-0.0) = -0.0")],
        "tan": [(0.0, 0.0, "tan(0.0)"), (-0.0, -0.0, "tan(-0.0) = -0.0")],
        "tanh": [(0.0, 0.0, "tanh(0.0)"), (-0.0, -0.0, "tanh(-0.0)"), (40.0, 1.0, "saturated"), (-40.0, -1.0, "saturated")],
        "sinh": [(0.0, 0.0, "sinh(0.0)"), (-0.0, -0.0, "sinh(-0.0)"), (90.0 if T == np.float32 else 711.0, INC, "overflow")],
        "cosh": [(0.0, 1.0, "cosh(0)"), (-90.0 if T == np.float32 else -711.0, INC, "overflow")],
        "atan": [(0.0, 0.0, "atan(0.0)"), (-0.0, -0.0, "atan(-0.0)")], "asinh": [(0.0, 0.0, "asinh(0.0)"), (-0.0, -0.0, "asinh(-0.0)")],
        "erf": [(0.0, 0.0, "erf(0.0)"), (-0.0, -0.0, "erf(-0.0)"), (10.0, 1.0, "saturated"), (-10.0, -1.0, "saturated")],
        "erfc": [(0.0, 1.0, "erfc(0)"), (-10.0, 2.0, "saturated"), (30.0, 0.0, "underflow to 0.0")],
    }
    with np.errstate(all="ignore"):
        return [[_s(T(x)), e if e == INC else _s(T(e)), c] for x, e, c in S[name]]


def binary_special(name, T):
    f = np.finfo(T)
    INC, nan, inf = "incomplete", float("nan"), float("inf")
    big_even = 2.0 ** (24 if T == np.float32 else 53)
    big_odd = 2.0 ** (23 if T == np.float32 else 52) + 1
    pw = f"{OPS}:35-49 safe_pow"
    cmpc = f"{OPS}:98-109 (x op y) * one"
    S = {
        "^": [(0.0, -1.0, INC, pw + ": integer y < 0 and x == 0 -> NaN"), (0.0, -2.0, INC, pw + ": integer y < 0 and x == 0"),
              (-2.0, 0.5, INC, pw + ": non-integer y > 0 and x < 0 -> NaN"), (-2.0, -0.5, INC, pw + ": non-integer y < 0 and x <= 0 -> NaN"),
              (0.0, -0.5, INC, pw + ": non-integer y < 0 and x <= 0"), (-0.0, -0.5, INC, pw + ": -0.0 <= 0"),
              (2.0, 3.0, 8.0, pw + ": x ^ y"), (-2.0, 3.0, -8.0, pw + ": integer y, negative base"), (-2.0, -2.0, 0.25, pw + ": integer y < 0, x != 0"),
              (0.0, 0.0, 1.0, pw + ": 0 ^ 0 = 1"), (-0.0, 0.0, 1.0, pw + ": 0 ^ 0 = 1"), (0.0, 0.5, 0.0, pw + ": non-integer y > 0, x = 0"),
              (-0.0, 3.0, -0.0, pw + ": (-0.0) ^ 3 = -0.0"), (-0.0, 2.0, 0.0, pw + ": (-0.0) ^ 2 = 0.0"),
              (-1.0, big_even, 1.0, pw + ": an exponent so large that every value of T is an even integer"), (-1.0, big_odd, -1.0, pw + ": (-1) ^ odd"),
              (-1.0, 3.0, -1.0, pw + ": (-1) ^ odd"), (2.0, inf, INC, pw + ": y = Inf is no integer; 2 ^ Inf = Inf"),
              (-2.0, inf, INC, pw + ": y = Inf is no integer, y > 0 and x < 0 -> NaN"), (4.0, 0.5, 2.0, pw + ": 4 ^ 0.5"),
              (10.0, 39.0 if T == np.float32 else 309.0, INC, "overflow")],
        "mod": [(5.0, 3.0, 2.0, "Base.mod"), (-5.0, 3.0, 1.0, "Base.mod: the result has the sign of y"), (5.0, -3.0, -1.0, "Base.mod"), (-5.0, -3.0, -2.0, "Base.mod"),
                (6.0, 3.0, 0.0, "Base.mod: an exact multiple, the zero has the sign of y"), (6.0, -3.0, -0.0, "Base.mod: copysign(r, y)"),
                (-6.0, 3.0, 0.0, "Base.mod: copysign(r, y)"), (-6.0, -3.0, -0.0, "Base.mod: copysign(r, y)"), (0.0, -3.0, -0.0, "Base.mod: copysign(r, y)"),
                (5.0, 0.0, INC, "Base.mod: rem(x, 0) = NaN"), (5.5, 2.0, 1.5, "Base.mod"), (-5.5, 2.0, 0.5, "Base.mod")],
        "max": [(0.0, -0.0, 0.0, "Base.max: -0.0 < 0.0"), (-0.0, 0.0, 0.0, "Base.max: -0.0 < 0.0"), (nan, 1.0, INC, "Base.max: NaN propagates"),
                (1.0, nan, INC, "Base.max: NaN propagates"), (1.0, 2.0, 2.0, "Base.max"), (-1.0, -2.0, -1.0, "Base.max"), (-0.0, -0.0, -0.0, "Base.max")],
        "min": [(0.0, -0.0, -0.0, "Base.min: -0.0 < 0.0"), (-0.0, 0.0, -0.0, "Base.min: -0.0 < 0.0"), (nan, 1.0, INC, "Base.min: NaN propagates"),
                (1.0, nan, INC, "Base.min: NaN propagates"), (1.0, 2.0, 1.0, "Base.min"), (-1.0, -2.0, -2.0, "Base.min"), (0.0, 0.0, 0.0, "Base.min")],
        ">": [(1.0, 1.0, 0.0, cmpc), (2.0, 1.0, 1.0, cmpc), (1.0, 2.0, 0.0, cmpc), (0.0, -0.0, 0.0, cmpc + ": 0.0 == -0.0"), (nan, 1.0, 0.0, cmpc + ": NaN compares false"),
              (1.0, nan, 0.0, cmpc + ": NaN compares false")],
        "<": [(1.0, 1.0, 0.0, cmpc), (2.0, 1.0, 0.0, cmpc), (1.0, 2.0, 1.0, cmpc), (-0.0, 0.0, 0.0, cmpc + ": 0.0 == -0.0"), (nan, 1.0, 0.0, cmpc + ": NaN compares false"),
              (1.0, nan, 0.0, cmpc + ": NaN compares false")],
        ">=": [(1.0, 1.0, 1.0, cmpc), (2.0, 1.0, 1.0, cmpc), (1.0, 2.0, 0.0, cmpc), (-0.0, 0.0, 1.0, cmpc + ": 0.0 == -0.0"), (nan, 1.0, 0.0, cmpc + ": NaN compares false"),
               (1.0, nan, 0.0, cmpc + ": NaN compares false")],
        "<=": [(1.0, 1.0, 1.0, cmpc), (2.0, 1.0, 0.0, cmpc), (1.0, 2.0, 1.0, cmpc), (0.0, -0.0, 1.0, cmpc + ": 0.0 == -0.0"), (nan, 1.0, 0.0, cmpc + ": NaN compares false"),
               (1.0, nan, 0.0, cmpc + ": NaN compares false")],
        "cond": [(-1.0, 5.0, 0.0, f"{OPS}:110-112 (x > 0) * y: false * y = copysign(0, y)"), (-1.0, -5.0, -0.0, f"{OPS}:110-112 copysign(0, y)"),
                 (1.0, 5.0, 5.0, f"{OPS}:110-112"), (0.0, 5.0, 0.0, f"{OPS}:110-112: 0 > 0 is false"), (1.0, -0.0, -0.0, f"{OPS}:110-112")],
        "logical_or": [(1.0, 1.0, 1.0, f"{OPS}:118-120"), (0.0, 0.0, 0.0, f"{OPS}:118-120"), (1.0, -1.0, 1.0, f"{OPS}:118-120"), (-1.0, -1.0, 0.0, f"{OPS}:118-120"),
                       (nan, 1.0, 1.0, f"{OPS}:118-120: NaN > 0 is false"), (nan, 0.0, 0.0, f"{OPS}:118-120: NaN > 0 is false")],
        "logical_and": [(1.0, 1.0, 1.0, f"{OPS}:121-123"), (1.0, 0.0, 0.0, f"{OPS}:121-123"), (0.0, 1.0, 0.0, f"{OPS}:121-123"), (-1.0, -1.0, 0.0, f"{OPS}:121-123"),
                        (nan, 1.0, 0.0, f"{OPS}:121-123: NaN > 0 is false"), (1.0, nan, 0.0, f"{OPS}:121-123: NaN > 0 is false")],
        "atan2": [(0.0, 1.0, 0.0, "atan(0.0, 1)"), (-0.0, 1.0, -0.0, "atan(-0.0, 1) = -0.0"), (0.0, 0.0, 0.0, "atan(0.0, 0.0) = 0.0"), (-0.0, 0.0, -0.0, "atan(-0.0, 0.0)")],
        "+": [(0.0, -0.0, 0.0, "IEEE"), (-0.0, -0.0, -0.0, "IEEE"), (1.0, -1.0, 0.0, "IEEE"), (f.max, f.max, INC, "overflow")],
        "-": [(0.0, 0.0, 0.0, "IEEE"), (-0.0, 0.0, -0.0, "IEEE"), (1.0, 1.0, 0.0, "IEEE"), (f.max, -f.max, INC, "overflow")],
        "*": [(0.0, -1.0, -0.0, "IEEE"), (-0.0, -1.0, 0.0, "IEEE"), (f.tiny, f.tiny, 0.0, "underflow"), (f.max, 2.0, INC, "overflow")],
        "/": [(0.0, -1.0, -0.0, "IEEE"), (1.0, 0.0, INC, "1 / 0 = Inf"), (0.0, 0.0, INC, "0 / 0 = NaN"), (-1.0, 0.0, INC, "-1 / 0 = -Inf"), (6.0, 3.0, 2.0, "IEEE")],
    }
    with np.errstate(all="ignore"):
        return [[_s(T(x)), _s(T(y)), e if e == INC else _s(T(e)), c] for x, y, e, c in S[name]]


def main():
    out = {}
    for tname, T in (("float32", np.float32), ("float64", np.float64)):
        eu, eb = _exact_unary(T), _exact_binary(T)
        un, bi = {}, {}
        for name in list(UNARY_FN) + list(eu):
            vals, seen = [], set()
            for x in unary_points(name, T):
                if float(x).hex() in seen or not np.isfinite(x):  # (by bit pattern: -0.0 is its own point)
                    continue
                seen.add(float(x).hex())
                with np.errstate(all="ignore"):
                    if name in eu:
                        hi, lo = float(eu[name](x)), 0.0
                    else:
                        hi, lo = _hl(UNARY_FN[name](mp.mpf(float(x))))
                if np.isfinite(T(hi)) and abs(hi) <= float(np.finfo(T).max):
                    vals.append([float(x), hi, lo])
            assert 8 <= len(vals) <= 64, (name, len(vals))
            un[name] = {"exact": name in eu, "values": vals, "special": unary_special(name, T)}
        for name in list(BINARY_FN) + list(eb):
            vals, seen = [], set()
            for x, y in binary_points(name, T):
                if (float(x).hex(), float(y).hex()) in seen:
                    continue
                seen.add((float(x).hex(), float(y).hex()))
                with np.errstate(all="ignore"):
                    if name in eb:
                        hi, lo = float(eb[name](x, y)), 0.0
                    elif name == "atan2":  # (mpmath has no signed zero: atan(-0.0, y) = -atan(0.0, y))
                        hi, lo = _hl(mp.atan2(mp.mpf(float(x)), mp.mpf(float(y))))
                        if x == 0 and np.signbit(x):
                            hi, lo = -hi, -lo
                    else:
                        hi, lo = _hl(mp.power(mp.mpf(float(x)), mp.mpf(float(y))))
                if np.isfinite(T(hi)) and abs(hi) <= float(np.finfo(T).max):
                    vals.append([float(x), float(y), hi, lo])
            assert 8 <= len(vals) <= 64, (name, len(vals))
            bi[name] = {"exact": name in eb, "values": vals, "special": binary_special(name, T)}
        assert len(un) == 33 and len(bi) == 16, (len(un), len(bi))
        out[tname] = {"unary": un, "binary": bi}
    path = os.path.join(HERE, "op_values.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
