"""TEST HELPER: the operator-value fixture (tests/golden/op_values.json, make_op_value_fixtures.py) and the trees
that put one operator in each of its compiled forms."""
import functools
import json
import os

import numpy as np

from sr_amd import Node, Options

HERE = os.path.dirname(os.path.abspath(__file__))
UNARY = ("neg square cube exp cos sin tan log log2 log10 log1p sqrt abs sign tanh sinh cosh atan asin acos acosh atanh "
         "asinh relu inv erf erfc gamma round floor ceil exp2 expm1").split()
BINARY = "+ - * / ^ max min mod > < >= <= cond logical_or logical_and atan2".split()
DTYPES = {"float32": np.float32, "float64": np.float64}
INCOMPLETE = "incomplete"


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(HERE, "golden", "op_values.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def options():
    """The whole catalog in one operator set (the FULL tier): operator k of UNARY / BINARY has index k + 1."""
    return Options(binary_operators=BINARY, unary_operators=UNARY)


def entry(dtype_name, name, degree):
    return fixture()[dtype_name]["unary" if degree == 1 else "binary"][name]


def points(dtype_name, name, degree):
    """(values, special) of one operator: values [[x, (y,) hi, lo]] as floats; special [(x, (y,) expected or None for
    incomplete, citation)] as values of T."""
    T = DTYPES[dtype_name]
    e = entry(dtype_name, name, degree)
    special = []
    for row in e["special"]:
        args = tuple(T(float(s)) for s in row[:degree])
        special.append(args + (None if row[degree] == INCOMPLETE else T(float(row[degree])), row[degree + 1]))
    return e["values"], special


def rows(dtype_name, name, degree):
    """Every point of one operator, values then special: (args [n, degree] in T, hi, lo, expected-incomplete mask)."""
    T = DTYPES[dtype_name]
    values, special = points(dtype_name, name, degree)
    args = [v[:degree] for v in values] + [s[:degree] for s in special]
    hi = [v[degree] for v in values] + [np.nan if s[degree] is None else float(s[degree]) for s in special]
    lo = [v[degree + 1] for v in values] + [0.0] * len(special)
    inc = [False] * len(values) + [s[degree] is None for s in special]
    return np.array(args, dtype=T).reshape(len(args), degree), np.array(hi), np.array(lo), np.array(inc)


def special_mask(dtype_name, name, degree):
    """rows()' points that are special cases (they follow the values)."""
    e = entry(dtype_name, name, degree)
    return np.arange(len(e["values"]) + len(e["special"])) >= len(e["values"])


def bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def ulp_error(T, got, hi, lo):
    """|got - (hi + lo)| in ulps of T at the value (the smaller spacing at a power of two; subnormal spacing at
    least)."""
    got, hi, lo = (np.asarray(a, dtype=np.float64) for a in (got, hi, lo))
    a = np.abs(hi).astype(T)
    with np.errstate(all="ignore"):
        ulp = np.minimum(np.spacing(a), np.spacing(np.nextafter(a, T(0)))).astype(np.float64)
    ulp = np.maximum(ulp, float(np.finfo(T).smallest_subnormal))
    return np.abs((got - hi) - lo) / ulp


# ------------------------------------------------------------------------------------------------- trees
def X(k):
    return Node(feature=k)


def C(v):
    return Node(val=float(v))


def un(name, child):
    return Node(op=UNARY.index(name) + 1, l=child)


def bi(name, a, b):
    return Node(op=BINARY.index(name) + 1, l=a, r=b)


def _x1x3():
    return bi("*", X(1), X(3))


def unary_forms(name):
    """{form: tree} over the features x1 (the point), x3 = 1, x4 = -x1; every tree is op(x1)."""
    return {
        "leaf": un(name, X(1)),                                               # POST on the leaf's load
        "post_inf": un(name, _x1x3()),                                        # POST_INF on a pair (DE's fused deg1_l2_ll0_lr0)
        "own": un(name, bi("*", bi("*", _x1x3(), X(3)), C(1.0))),            # SR_OP_UNARY0 + op
        "own_inf": un(name, un("neg", X(4))),                                 # SR_OP_UNARY_INF0 + op (DE's fused deg1_l1_ll0)
    }


def binary_forms(name):
    """Forms of op(x1, x2) that hold no constant (x3 = 1)."""
    a, b = _x1x3, lambda: bi("*", X(2), X(3))
    return {"FF": bi(name, X(1), X(2)), "S": bi(name, a(), b()), "FR": bi(name, a(), X(2)), "FL": bi(name, X(1), b()),
            "S_other": bi(name, a(), bi("*", b(), bi("*", X(3), X(3))))}


def binary_const_forms(name, x, y):
    """Forms of op(x, y) with one operand a constant: the other comes from the row (x1 = x, x2 = y)."""
    return {"FC": bi(name, X(1), C(y)), "CF": bi(name, C(x), X(2)), "CR": bi(name, _x1x3(), C(y)),
            "CL": bi(name, C(x), bi("*", X(2), X(3)))}


def binary_param_forms(name):
    """Forms with a parameter operand (p1: leaf x5 before parametric_util.to_parametric over 4 features): PR
    op(x1 * x3, p1) with p1 = y, PL op(p1, x2 * x3) with p1 = x."""
    return {"PR": bi(name, _x1x3(), X(5)), "PL": bi(name, X(5), bi("*", X(2), X(3)))}
