"""Generate tests/golden/loss_expr_rules.json — high-precision gradients THROUGH expression-loss programs.

TEST INFRASTRUCTURE (fixture generator; runs in the build container, needs mpmath).

An expression loss (csrc/sr_loss_expr.h) differentiates its body by forward mode with the rules of csrc/sr_ops.h
(sr_unary_deriv / sr_binary_partials) inside an interpreter of its own; the gradient kernels multiply the result
into the tree's tangents.  This file pins that path per rule, with make_grad_rule_fixtures.py's method and code: its
mpmath value semantics (`unary`, `binary`), its `Tree`, its kink margin (`Kink`), its datasets (read from
grad_rules.json through `mp_data`, not copied) and its stepping of constants off the kinks (`solve`, whose reference
function is replaced by the one below).  Here too NO derivative rule: the loss body is evaluated with `Tree`
(x1 = p, x2 = t, x3 = w) in place of `row_losses`, and the whole loss is differentiated numerically at 60 digits.

Cases: the tree is {0} * x1 + {1} * x2 + {2} on the dataset "normal"; the loss is sum(L) / n, or sum(L) / sum(w)
when the body names w (the weight is the expression's third argument and is not multiplied in again).
  * one body per unary operator with a rule, its argument chosen by domain; a piecewise-constant operator is
    multiplied by (p - t) so that the loss still depends on the prediction;
  * three bodies per binary operator — the first operand, the second, or both depending on the prediction — the
    operands wrapped into the operator's domain and w the independent operand (the three-argument form).
Stored per case, as in grad_rules.json: loss, grad, zero, u32 / u64 (eps_T sum |row terms| / denom), and the loss's
own unit lu32 / lu64 = eps_T sum |L_i| / denom.

Run:  python tests/golden/make_loss_expr_fixtures.py   (deterministic; rewrites the JSON; grad_rules.json untouched)
"""
import json
import os
import re
import sys

import mpmath

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_grad_rule_fixtures as mg  # noqa: E402
from make_grad_rule_fixtures import BINARY, EPS, PIECEWISE_CONSTANT, UNARY, Kink, Tree, call, mp_data, mpf  # noqa: E402,F401

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "loss_expr_rules.json")
GROUP = "lossx"
TREE = "{0} * x1 + {1} * x2 + {2}"
CONSTS = (1.25, -0.5, 0.5)
POSITIVE = "(square(p - t) + 1.25)"      # >= 1.25: log log2 log10 log1p sqrt inv acosh, divisors, bases
UNIT = "(0.5 * tanh(p - t))"             # inside (-0.5, 0.5): tan asin acos atanh
POSITIVE_ARG = ("log", "log2", "log10", "log1p", "sqrt", "inv", "acosh")
UNIT_ARG = ("tan", "asin", "acos", "atanh")
UNARY_STEPS = ("sign", "round", "floor", "ceil")
D1, D2 = "(p - t)", "(0.5 * p + t)"      # two operands that depend on the prediction
POSITIVE2 = "(square(0.5 * p + t) + 1.25)"


def body_tree(body):
    """The loss body as a `Tree` over x1 = p, x2 = t, x3 = w."""
    return Tree(re.sub(r"\b([ptw])\b", lambda m: "x%d" % ("ptw".index(m.group(1)) + 1), body))


def names_w(body):
    return re.search(r"\bw\b", body) is not None


def bodies():
    """[(case name, body)]: 32 unary and 48 binary bodies."""
    out = []
    for u in UNARY:
        arg = POSITIVE if u in POSITIVE_ARG else (UNIT if u in UNIT_ARG else D1)
        body = f"{u}({arg})"
        out.append((f"unary/{u}", f"{body} * {D1}" if u in UNARY_STEPS else body))
    for op, enum in BINARY.items():
        if op == "/":
            forms = [(D1, "w"), ("w", POSITIVE), (D1, POSITIVE2)]
        elif op == "^":
            forms = [(POSITIVE, "w"), ("w", D1), (POSITIVE, "(0.5 * tanh(0.5 * p + t))")]
        elif op == "mod":
            forms = [(D1, "w"), ("w", POSITIVE), (D1, POSITIVE2)]
        elif op == "atan2":
            forms = [(D1, "w"), ("w", D1), (D1, POSITIVE2)]
        else:
            forms = [(D1, "w"), ("w", D1), (D1, D2)]
        for tag, (a, b) in zip(("first", "second", "both"), forms):
            body = call(op, a, b)
            # (cond(a, w) = (a > 0) * w is piecewise constant in its first operand too)
            flat = op in PIECEWISE_CONSTANT or (op == "cond" and tag == "first")
            out.append((f"binary/{enum.lower()}/{tag}", f"{body} * {D1}" if flat else body))
    return out


def reference(expr, body, data, weighted, P):
    """make_grad_rule_fixtures.reference with the loss body in place of the catalog loss: loss, gradient and units
    of one case (mpf rows); raises Kink near a branch point of the tree or of the body."""
    assert P is None
    tree, loss_tree = Tree(expr), body_tree(body)
    consts = [mpf(c) for c in tree.constants]
    lconsts = [mpf(c) for c in loss_tree.constants]
    y, w = data["y"], data["w"]
    denom = mpmath.fsum(w) if weighted else mpf(len(y))

    def row_losses(pred):
        return loss_tree.eval_all(dict(X=[pred, y, w], cls=data["cls"]), lconsts, None)[0]

    vals = tree.eval_all(data, consts, None)
    li = row_losses(vals[0])
    loss = mpmath.fsum(li) / denom
    lunit = mpmath.fsum(abs(v) for v in li) / denom
    grads = []
    for k, node in enumerate(tree.const_nodes):
        h = mpf("1e-18") * max(1, abs(consts[k]))
        lp = row_losses(tree.with_leaf(vals, {node: [consts[k] + h] * len(y)}))
        lm = row_losses(tree.with_leaf(vals, {node: [consts[k] - h] * len(y)}))
        terms = [(a - b) / (2 * h) for a, b in zip(lp, lm)]
        grads.append((mpmath.fsum(terms) / denom, mpmath.fsum(abs(t) for t in terms) / denom))
    return dict(loss=float(loss), lu32=float(lunit * EPS["float32"]), lu64=float(lunit * EPS["float64"]),
                grad=[float(g) for g, _ in grads], zero=[int(s == 0) for _, s in grads],
                u32=[float(s * EPS["float32"]) for _, s in grads], u64=[float(s * EPS["float64"]) for _, s in grads])


def main():
    with open(os.path.join(HERE, "grad_rules.json")) as f:
        datasets = json.load(f)["datasets"]
    # `solve` steps a case's constants by 1/256 while a row sits within the margin of a kink; it calls the module's
    # `reference(expr, case["loss"], data, weighted, P)`: ours, with the body as the loss
    mg.GROUPS[GROUP] = ([], ["+", "*"], 0)
    mg.reference = reference
    out = {"generator": "tests/golden/make_loss_expr_fixtures.py (mpmath %s, %d digits)" % (mpmath.__version__, mg.mp.dps),
           "note": "loss = sum(L) / n, or / sum(w) when the body names w; grad: d loss / d constant of the tree in "
                   "pre-order; u32 / u64: eps_T sum|row terms| / denom; lu32 / lu64: eps_T sum|L_i| / denom; zero: "
                   "every row term is exactly 0; the dataset is grad_rules.json's",
           "dataset": "normal", "operators": dict(unary=[], binary=["+", "*"]), "cases": []}
    for name, body in bodies():
        weighted = names_w(body)
        case = dict(name=name, group=GROUP, dataset="normal", template=TREE, consts=list(CONSTS), loss=body,
                    weighted=weighted, rows=None)
        expr, ref = mg.solve(case, datasets)
        spec = ("loss(p, t, w) = " if weighted else "loss(p, t) = ") + body
        out["cases"].append(dict(name=name, body=body, loss_spec=spec, expr=expr, weighted=weighted,
                                 constants=Tree(expr).constants, **ref))
        print(name, body, expr, file=sys.stderr)
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, len(out["cases"]), "cases,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
