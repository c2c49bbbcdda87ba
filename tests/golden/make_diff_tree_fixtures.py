"""Generate tests/golden/diff_tree_array.json — per-row derivatives of the reference derivative test's equations.

TEST INFRASTRUCTURE (fixture generator; runs in the build container, needs mpmath).

The reference tests eval_diff_tree_array / eval_grad_tree_array on three equations
(test/integration/ad/zygote/test_derivatives.jl:12-27) and, for the constants, on `3.2 * x1` and equation5
(:92-123).  Here they are restated over the operator catalog: pow_abs2(a, b) is abs(a) ^ b, custom_cos(a) is
square(cos(a)); the constants are the reference's.  This file holds NO derivative rule: it imports the VALUE
semantics of make_grad_rule_fixtures.py and differentiates every row numerically at 60 digits,

    d = (f(v + h) - f(v - h)) / 2h,   h = 1e-18 max(1, |v|)          (truncation error ~ 1e-36)

per feature x_f (every occurrence of the feature stepped together) and per constant (pre-order).

X: nfeatures = 3, N = 100, multiples of 2^-12 in [2^-4, 5) from a fixed numpy seed — exact in Float32, so
both element types see the same numbers.

Run:  python tests/golden/make_diff_tree_fixtures.py   (deterministic; rewrites the JSON)
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_grad_rule_fixtures import Tree, mpf, mpmath  # noqa: E402  (value semantics; sets mp.dps = 60)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "diff_tree_array.json")
SCALE = 4096
NFEATURES, N = 3, 100
F32 = lambda v: float(np.float32(v))  # noqa: E731  (the reference's Float32 literals)

UNARY = ["abs", "square", "cos", "exp", "sin"]
BINARY = ["+", "*", "-", "/", "^"]
POW = "(abs({0}) ^ {1})"
CC = "square(cos({0}))"

EQUATION1 = "x1 + x2 + x3 + 3.2"
EQUATION2 = POW.format("x1", "x2") + " + x3 + " + CC.format("1.0 + x3") + " + 3.0 / x1"
EQUATION3 = (
    "((x2 + x2) * ((-0.5982493 / " + POW.format("x1", "x2") + ") / -0.54734415)) + ("
    "sin(" + CC.format(
        "sin(1.2926733 - 1.6606787) / sin(((0.14577048 * x1) + ((0.111149654 + x1) - -0.8298334)) - -1.2071426)")
    + " * (" + CC.format("x3 - 2.3201916") + " + ((x1 - (x1 * x2)) / x2))"
    ") / (0.14854191 - ((" + CC.format("x2") + " * -1.6047639) - 0.023943262)))")
EQUATION4 = "%r * x1" % F32(3.2)
EQUATION5 = POW.format("x1", "x2") + " + x3 + " + CC.format("%r + x3" % F32(2.1)) + " + %r / x1" % F32(-3.2)

CASES = [("equation1", EQUATION1, True), ("equation2", EQUATION2, True), ("equation3", EQUATION3, True),
         ("equation4", EQUATION4, False), ("equation5", EQUATION5, False)]


def pole_sensitivity(x1):
    """equation3 holds custom_cos(A / sin(z)) with z = 0.14577048 x1 + ((0.111149654 + x1) + 0.8298334) + 1.2071426,
    and sin(z) has zeros inside the range of x1.  A Float32 evaluation carries z to about eps_32 |z|; this is
    how far (in radians) that moves the cosine's argument u = A / sin(z):  |du/dz| eps_32 |z|."""
    A = np.sin(1.2926733 - 1.6606787)
    z = 0.14577048 * x1 + ((0.111149654 + x1) + 0.8298334) + 1.2071426
    return np.abs(A * np.cos(z) / np.sin(z) ** 2) * np.abs(z) * 2.0 ** -23


def make_x():
    """Multiples of 2^-12 in [2^-4, 5).  A row where Float32's rounding of z alone would move the argument of
    equation3's cosine by more than 2^-7 rad is ill-conditioned in Float32 whatever evaluates it (the test's
    criterion, rtol = 0.1 on the 2-norm, is then decided by that one row's noise); its x1 is drawn again.  The rule looks at the
    inputs only."""
    rng = np.random.default_rng(20261021)
    X = rng.integers(SCALE // 16, 5 * SCALE, (NFEATURES, N)).astype(np.int64)
    for i in range(N):
        while pole_sensitivity(X[0, i] / SCALE) > 2.0 ** -7:
            X[0, i] = rng.integers(SCALE // 16, 5 * SCALE)
    return X


def derivatives(expr, Xq):
    tree = Tree(expr)
    data = dict(X=[[mpf(int(k)) / SCALE for k in row] for row in Xq], cls=[1] * N)
    consts = [mpf(c) for c in tree.constants]
    vals = tree.eval_all(data, consts, None)

    def central(leaves, base):
        """leaves: the stepped leaf nodes; base: their rows."""
        out = []
        hs = [mpf("1e-18") * max(1, abs(v)) for v in base]
        up = tree.with_leaf(vals, {i: [v + h for v, h in zip(base, hs)] for i in leaves})
        dn = tree.with_leaf(vals, {i: [v - h for v, h in zip(base, hs)] for i in leaves})
        for a, b, h in zip(up, dn, hs):
            out.append(float((a - b) / (2 * h)))
        return out

    d_feat = []
    for f in range(NFEATURES):
        leaves = [i for i, nd in enumerate(tree.nodes) if nd[0] == "x" and nd[1] == f]
        d_feat.append(central(leaves, data["X"][f]) if leaves else [0.0] * N)
    d_const = [central([node], [consts[k]] * N) for k, node in enumerate(tree.const_nodes)]
    return [float(v) for v in vals[0]], d_feat, d_const, tree.constants


def main():
    Xq = make_x()
    out = {"generator": "tests/golden/make_diff_tree_fixtures.py (mpmath %s, %d digits)" % (mpmath.__version__, mpmath.mp.dps),
           "note": "value[N]; d_feature[nfeatures][N]; d_constant[n_constants][N] (pre-order): central differences "
                   "of the value semantics, per row",
           "unary_operators": UNARY, "binary_operators": BINARY, "scale": SCALE, "X": Xq.tolist(), "cases": []}
    for name, expr, variable in CASES:
        value, d_feat, d_const, constants = derivatives(expr, Xq)
        out["cases"].append(dict(name=name, expr=expr, variable=variable, constants=constants, value=value,
                                 d_feature=d_feat, d_constant=d_const))
        print(name, expr, file=sys.stderr)
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, len(out["cases"]), "cases,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
