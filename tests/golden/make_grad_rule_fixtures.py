"""Generate tests/golden/grad_rules.json — high-precision loss gradients pinning every derivative rule.

TEST INFRASTRUCTURE (fixture generator; runs in the build container, needs mpmath).

The forward-mode gradient kernels (csrc/sr_grad_body.h) take their rules from csrc/sr_ops.h:
sr_unary_deriv, sr_binary_partials, sr_elem_loss_deriv.  This file holds NO derivative rule.  It restates
the VALUE semantics of sr_unary / sr_binary / sr_elem_loss in mpmath (safe operators, Julia mod, cond, relu,
round-half-even) and differentiates the whole loss numerically at 60 digits:

    g = (L(c + h) - L(c - h)) / 2h,   h = 1e-18 max(1, |c|)          (truncation error ~ 1e-36)

per scalar c, in eval_grad_batch's layout: the constants in pre-order, then the K x C parameter matrix
column-major.  Next to each entry it stores an error unit

    u_T = eps_T * sum_rows |w_i (L_i(c + h) - L_i(c - h)) / 2h| / denom

(the same central difference, its row terms summed by absolute value): a gradient computed in T cannot be
expected closer than a few u_T, however the rows cancel.  Entries whose every row term is exactly 0 are
marked `zero`: the device must return exactly 0 there.

Inputs stay off the kinks: no row of any case lies within 1e-3 of a point where an operator or loss changes
branch (asserted; a case that would hit one has its constants stepped by 1/256 until it does not — the
constants the JSON records are the stepped ones).  All data and constants are multiples of 2^-12 below 2^12:
exact in Float32, so the Float32 and Float64 runs see the same numbers.

Run:  python tests/golden/make_grad_rule_fixtures.py   (deterministic; rewrites the JSON)
"""
import ast
import json
import os
import sys

import mpmath
import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "grad_rules.json")
mp = mpmath.mp
mp.dps = 60
mpf = mpmath.mpf
SCALE = 4096
N_ROWS = 200
MARGIN = mpf("1e-3")
EPS = {"float32": float(np.finfo(np.float32).eps), "float64": float(np.finfo(np.float64).eps)}

# operator name -> SrUnaryOp / SrBinaryOp enumerator (csrc/sr_ops.h), for the `hits` a case records
UNARY = ["neg", "square", "cube", "exp", "cos", "sin", "tan", "log", "log2", "log10", "log1p", "sqrt", "abs", "sign",
         "tanh", "sinh", "cosh", "atan", "asin", "acos", "acosh", "atanh", "asinh", "relu", "inv", "erf", "erfc",
         "round", "floor", "ceil", "exp2", "expm1"]
BINARY = {"+": "ADD", "-": "SUB", "*": "MUL", "/": "DIV", "^": "POW", "max": "MAX", "min": "MIN", "mod": "MOD",
          "greater": "GREATER", "less": "LESS", "greater_equal": "GREATER_EQUAL", "less_equal": "LESS_EQUAL",
          "cond": "COND", "logical_or": "LOGICAL_OR", "logical_and": "LOGICAL_AND", "atan2": "ATAN2"}
PIECEWISE_CONSTANT = ("greater", "less", "greater_equal", "less_equal", "logical_or", "logical_and")
_PY_BIN = {ast.Add: "+", ast.Sub: "-", ast.Mult: "*", ast.Div: "/", ast.Pow: "^"}


class Kink(Exception):
    pass


def _off(dist, what):
    if abs(dist) < MARGIN:
        raise Kink(what)


# ------------------------------------------------------------------ value semantics (sr_unary / sr_binary)
def unary(name, x):
    if name == "neg":
        return -x
    if name == "square":
        return x * x
    if name == "cube":
        return x * x * x
    if name in ("exp", "cos", "sin", "tan", "tanh", "sinh", "cosh", "atan", "asinh", "erf", "erfc", "expm1"):
        return getattr(mpmath, name)(x)
    if name in ("log", "log2", "log10"):
        assert x > 0
        return mpmath.log(x) / {"log": 1, "log2": mpmath.log(2), "log10": mpmath.log(10)}[name]
    if name == "log1p":
        assert x > -1
        return mpmath.log1p(x)
    if name == "sqrt":
        assert x > 0
        return mpmath.sqrt(x)
    if name == "abs":
        _off(x, "abs at 0")
        return abs(x)
    if name == "sign":
        _off(x, "sign at 0")
        return mpf(1 if x > 0 else -1)
    if name in ("asin", "acos", "atanh"):
        assert -1 < x < 1
        return getattr(mpmath, name)(x)
    if name == "acosh":
        assert x > 1
        return mpmath.acosh(x)
    if name == "relu":
        _off(x, "relu at 0")
        return x if x > 0 else mpf(0)
    if name == "inv":
        return 1 / x
    if name == "round":  # ties to even; no row is near a tie
        _off(x - mpmath.floor(x) - mpf("0.5"), "round at a tie")
        return mpmath.nint(x)
    if name in ("floor", "ceil"):
        _off(x - mpmath.nint(x), name + " at a step")
        return getattr(mpmath, name)(x)
    if name == "exp2":
        return mpmath.power(2, x)
    raise ValueError(name)


def binary(name, a, b):
    if name == "+":
        return a + b
    if name == "-":
        return a - b
    if name == "*":
        return a * b
    if name == "/":
        return a / b
    if name == "^":  # safe_pow's valid branches only
        isint = b == mpmath.nint(b)
        assert a > 0 or (isint and (a != 0 or b > 0)), ("safe_pow domain", a, b)
        return mpmath.power(a, b) if a != 0 else mpf(0)
    if name in ("max", "min"):
        _off(a - b, name + " tie")
        return (a if a > b else b) if name == "max" else (a if a < b else b)
    if name == "mod":  # Julia mod: x - y floor(x / y), the sign of y
        q = a / b
        _off((q - mpmath.nint(q)) * b, "mod wrap")
        return a - b * mpmath.floor(q)
    if name in ("greater", "less", "greater_equal", "less_equal"):
        _off(a - b, name + " threshold")
        return mpf(1 if ((a > b) == (name.startswith("greater"))) else 0)
    if name == "cond":
        _off(a, "cond threshold")
        return b if a > 0 else mpf(0)
    if name in ("logical_or", "logical_and"):
        _off(a, name + " threshold")
        _off(b, name + " threshold")
        return mpf(1 if ((a > 0 or b > 0) if name == "logical_or" else (a > 0 and b > 0)) else 0)
    if name == "atan2":
        return mpmath.atan2(a, b)
    raise ValueError(name)


# ------------------------------------------------------------------ elementwise losses (sr_elem_loss)
LOSS_KINDS = ["L2DistLoss", "L1DistLoss", "LPDistLoss", "LogitDistLoss", "HuberLoss", "L1EpsilonInsLoss",
              "L2EpsilonInsLoss", "PeriodicLoss", "QuantileLoss", "ZeroOneLoss", "PerceptronLoss", "L1HingeLoss",
              "L2HingeLoss", "SmoothedL1HingeLoss", "ModifiedHuberLoss", "L2MarginLoss", "ExpLoss", "SigmoidLoss",
              "DWDMarginLoss"]


def parse_loss(spec):
    name = spec.split("{")[0].split("(")[0]
    arg = spec[len(name):].strip("{}()")
    return name, (mpf(arg) if arg else mpf(1))  # (HuberLoss() is HuberLoss(1.0))


def is_margin(spec):
    return LOSS_KINDS.index(parse_loss(spec)[0]) >= 9


def elem_loss(name, p, pred, y):
    """(value, branch) of one row; the branch index counts rows per side for the piecewise losses."""
    d, a = pred - y, y * pred
    ad = abs(d)
    pos = lambda v: v if v > 0 else mpf(0)  # noqa: E731
    if name == "L2DistLoss":
        return d * d, 0
    if name == "L1DistLoss":
        _off(d, "L1 at 0")
        return ad, 0
    if name == "LPDistLoss":
        return mpmath.power(ad, p), 0
    if name == "LogitDistLoss":
        return -mpmath.log(4) - d + 2 * mpmath.log(1 + mpmath.exp(d)), 0
    if name == "HuberLoss":
        _off(ad - p, "Huber at delta")
        return (d * d / 2, 0) if ad <= p else (p * (ad - p / 2), 1)
    if name == "L1EpsilonInsLoss":
        _off(ad - p, "EpsilonIns at eps")
        return pos(ad - p), int(ad > p)
    if name == "L2EpsilonInsLoss":
        _off(ad - p, "EpsilonIns at eps")
        return pos(ad - p) ** 2, int(ad > p)
    if name == "PeriodicLoss":
        return 1 - mpmath.cos(d * 2 * mpmath.pi / p), 0
    if name == "QuantileLoss":
        _off(d, "Quantile at 0")
        return d * ((1 if d > 0 else 0) - p), int(d > 0)
    if name == "ZeroOneLoss":
        _off(a, "ZeroOne at 0")
        return mpf(1 if a < 0 else 0), int(a < 0)
    if name == "PerceptronLoss":
        _off(a, "Perceptron at 0")
        return pos(-a), int(a < 0)
    if name == "L1HingeLoss":
        _off(a - 1, "hinge at 1")
        return pos(1 - a), int(a < 1)
    if name == "L2HingeLoss":
        _off(a - 1, "hinge at 1")
        return pos(1 - a) ** 2, int(a < 1)
    if name == "SmoothedL1HingeLoss":
        _off(a - 1, "hinge at 1")
        _off(a - (1 - p), "smoothed hinge at 1 - gamma")
        if a >= 1 - p:
            return pos(1 - a) ** 2 / (2 * p), int(a < 1)
        return 1 - p / 2 - a, 2
    if name == "ModifiedHuberLoss":
        _off(a - 1, "hinge at 1")
        _off(a + 1, "modified Huber at -1")
        if a >= -1:
            return pos(1 - a) ** 2, int(a < 1)
        return -4 * a, 2
    if name == "L2MarginLoss":
        return (1 - a) ** 2, 0
    if name == "ExpLoss":
        return mpmath.exp(-a), 0
    if name == "SigmoidLoss":
        return 1 - mpmath.tanh(a), 0
    if name == "DWDMarginLoss":
        _off(a - p / (p + 1), "DWD at q / (q + 1)")
        if a <= p / (p + 1):
            return 1 - a, 0
        return (mpmath.power(p, p) / mpmath.power(p + 1, p + 1)) / mpmath.power(a, p), 1
    raise ValueError(name)


N_BRANCHES = {"HuberLoss": 2, "SmoothedL1HingeLoss": 3, "ModifiedHuberLoss": 3, "DWDMarginLoss": 2}


# ------------------------------------------------------------------ trees
class Tree:
    """Pre-order node list of an expression string in parse_expression's syntax: numeric literals are the
    constants, x<k> features, p<k> parameters.  Node: (kind, arg, kids) with kind in c x p u b."""

    def __init__(self, expr):
        self.nodes, self.parent = [], []
        self._add(ast.parse(expr.replace("^", "**"), mode="eval").body, -1)
        self.const_nodes = [i for i, n in enumerate(self.nodes) if n[0] == "c"]
        self.constants = [self.nodes[i][1] for i in self.const_nodes]

    def _add(self, e, parent):
        i = len(self.nodes)
        self.nodes.append(None)
        self.parent.append(parent)
        if isinstance(e, ast.Constant):
            self.nodes[i] = ("c", float(e.value), ())
        elif isinstance(e, ast.UnaryOp) and isinstance(e.op, ast.USub) and isinstance(e.operand, ast.Constant):
            self.nodes[i] = ("c", -float(e.operand.value), ())
        elif isinstance(e, ast.Name):
            assert e.id[0] in "xp" and e.id[1:].isdigit(), e.id
            self.nodes[i] = (e.id[0], int(e.id[1:]) - 1, ())
        elif isinstance(e, ast.BinOp):
            l = self._add(e.left, i)
            self.nodes[i] = ("b", _PY_BIN[type(e.op)], (l, self._add(e.right, i)))
        elif isinstance(e, ast.Call) and len(e.args) == 1:
            self.nodes[i] = ("u", e.func.id, (self._add(e.args[0], i),))
        elif isinstance(e, ast.Call) and len(e.args) == 2:
            l = self._add(e.args[0], i)
            self.nodes[i] = ("b", e.func.id, (l, self._add(e.args[1], i)))
        else:
            raise ValueError(ast.dump(e))
        return i

    def leaf(self, i, data, consts, P):
        kind, arg, _ = self.nodes[i]
        n = len(data["cls"])
        if kind == "c":
            return [consts[self.const_nodes.index(i)]] * n
        if kind == "x":
            return data["X"][arg]
        return [P[arg][c - 1] for c in data["cls"]]

    def node(self, i, vals):
        kind, arg, kids = self.nodes[i]
        if kind == "u":
            return [unary(arg, x) for x in vals[kids[0]]]
        return [binary(arg, a, b) for a, b in zip(vals[kids[0]], vals[kids[1]])]

    def eval_all(self, data, consts, P):
        vals = [None] * len(self.nodes)
        for i in reversed(range(len(self.nodes))):  # children follow their parent in pre-order
            vals[i] = self.leaf(i, data, consts, P) if not self.nodes[i][2] else self.node(i, vals)
        return vals

    def with_leaf(self, vals, leaves):
        """The root's rows with the given {leaf node: rows} replaced: only the leaves' ancestors are
        recomputed, every other subtree comes from `vals`."""
        new = dict(leaves)
        todo = sorted({a for i in leaves for a in self._ancestors(i)}, reverse=True)

        class V:
            def __getitem__(s, k):
                return new[k] if k in new else vals[k]

        for i in todo:
            new[i] = self.node(i, V())
        return new[0] if 0 in new else vals[0]

    def _ancestors(self, i):
        while self.parent[i] >= 0:
            i = self.parent[i]
            yield i


def row_losses(spec, pred, y):
    name, p = parse_loss(spec)
    out = [elem_loss(name, p, a, b) for a, b in zip(pred, y)]
    return [v for v, _ in out], [b for _, b in out]


def reference(expr, spec, data, weighted, P):
    """Loss, gradient and error units of one case on `data` (mpf rows); raises Kink near a branch point."""
    tree = Tree(expr)
    consts = [mpf(c) for c in tree.constants]
    Pm = None if P is None else [[mpf(v) for v in row] for row in P]
    y = data["ym"] if is_margin(spec) else data["y"]
    w = data["w"] if weighted else [mpf(1)] * len(y)
    denom = mpmath.fsum(w)
    vals = tree.eval_all(data, consts, Pm)
    li, branch = row_losses(spec, vals[0], y)
    name = parse_loss(spec)[0]
    for b in range(N_BRANCHES.get(name, 0)):
        assert branch.count(b) >= 20, (spec, "rows on branch", b, branch.count(b))
    loss = mpmath.fsum(wi * v for wi, v in zip(w, li)) / denom

    def diff(leaves_of):  # leaves_of(step) -> {leaf node: rows}; per-row central difference of w_i L_i
        c, h = leaves_of
        lp, _ = row_losses(spec, tree.with_leaf(vals, c(+h)), y)
        lm, _ = row_losses(spec, tree.with_leaf(vals, c(-h)), y)
        terms = [wi * (a - b) / (2 * h) for wi, a, b in zip(w, lp, lm)]
        return mpmath.fsum(terms) / denom, mpmath.fsum(abs(t) for t in terms) / denom

    grads = []
    for k, node in enumerate(tree.const_nodes):
        h = mpf("1e-18") * max(1, abs(consts[k]))
        grads.append(diff((lambda s, node=node, k=k: {node: [consts[k] + s] * len(y)}, h)))
    if Pm is not None:
        K, C = len(Pm), len(Pm[0])
        for c in range(C):  # column-major: entry k + K c
            for k in range(K):
                nodes = [i for i, nd in enumerate(tree.nodes) if nd[0] == "p" and nd[1] == k]
                h = mpf("1e-18") * max(1, abs(Pm[k][c]))

                def leaves(s, nodes=nodes, k=k, c=c):
                    rows = [Pm[k][cl - 1] + (s if cl - 1 == c else 0) for cl in data["cls"]]
                    return {i: rows for i in nodes}

                grads.append(diff((leaves, h)) if nodes else (mpf(0), mpf(0)))
    return dict(loss=float(loss), grad=[float(g) for g, _ in grads], zero=[int(s == 0) for _, s in grads],
                u32=[float(s * EPS["float32"]) for _, s in grads], u64=[float(s * EPS["float64"]) for _, s in grads])


# ------------------------------------------------------------------ datasets
def _q(a):
    return np.round(np.asarray(a) * SCALE).astype(np.int64)


def make_datasets():
    rng = np.random.default_rng(20261020)
    out = {}
    for name in ("normal", "unit", "pos", "powint"):
        if name == "normal":
            X = rng.standard_normal((3, N_ROWS))
        elif name == "unit":
            X = rng.uniform(-0.9, 0.9, (3, N_ROWS))
        elif name == "pos":
            X = rng.uniform(0.5, 3.0, (3, N_ROWS))
        else:  # x1: bases with exact zeros and both signs; x3: the integer exponents 2 and 3
            X = rng.uniform(-2.0, 2.0, (3, N_ROWS))
            X[0, ::8] = 0.0
            X[2] = 2 + (np.arange(N_ROWS) % 5 < 2)
        noise = rng.standard_normal(N_ROWS)
        y = 1.5 * X[0] - X[1] + 0.5 * X[2] + 0.25 + 0.3 * noise
        ym = np.where(X[0] - X[0].mean() + 1.2 * rng.standard_normal(N_ROWS) > 0, 1.0, -1.0)
        cls = rng.integers(1, 4, N_ROWS)
        cls[:3] = (1, 2, 3)
        out[name] = dict(scale=SCALE, X=_q(X).tolist(), y=_q(y).tolist(), ym=_q(ym).tolist(),
                         w=_q(rng.uniform(0.5, 2.0, N_ROWS)).tolist(), cls=cls.tolist())
    return out


def mp_data(ds, rows=None):
    sel = (lambda v: v) if rows is None else (lambda v: [v[r] for r in rows])
    m = lambda v: [mpf(int(k)) / ds["scale"] for k in sel(v)]  # noqa: E731
    return dict(X=[m(f) for f in ds["X"]], y=m(ds["y"]), ym=m(ds["ym"]), w=m(ds["w"]), cls=sel(ds["cls"]))


# ------------------------------------------------------------------ the case list
ALL_BINARY = list(BINARY)
GROUPS = {
    # name -> (unary operators, binary operators, parametric K)
    "unary": (UNARY, ["+", "*"], 0),
    "binary": (["cos"], ALL_BINARY, 0),
    "loss": ([], ["+", "*"], 0),
    "param": (["cos"], ALL_BINARY, 2),
}
P_MATRIX = [[1.5, 0.75, 1.25], [0.625, 2.0, 0.875]]
CATALOG = ["L2DistLoss()", "L1DistLoss()", "LPDistLoss{3}()", "LogitDistLoss()", "HuberLoss()", "HuberLoss(0.3)",
           "L1EpsilonInsLoss(0.2)", "L2EpsilonInsLoss(0.2)", "PeriodicLoss(4.0)", "QuantileLoss(0.3)",
           "ZeroOneLoss()", "PerceptronLoss()", "L1HingeLoss()", "L2HingeLoss()", "SmoothedL1HingeLoss(0.5)",
           "ModifiedHuberLoss()", "L2MarginLoss()", "ExpLoss()", "SigmoidLoss()", "DWDMarginLoss(2)"]
UNARY_DATA = {"unit": ("tan", "asin", "acos", "atanh"),
              "pos": ("log", "log2", "log10", "log1p", "sqrt", "inv", "acosh")}


def call(op, a, b):
    return f"({a} {op} {b})" if op in "+-*/^" else f"{op}({a}, {b})"


def variant(op, v):
    """The opcode variant the compiler emits: + and * commute, so only their R variants exist."""
    if op in "+*" and v[-1] == "L":
        v = v[:-1] + "R"
    return v


def case_list():
    cases = []

    def add(name, group, dataset, template, consts, hits, loss="L2DistLoss()", weighted=False, rows=None):
        cases.append(dict(name=name, group=group, dataset=dataset, template=template, consts=list(consts), hits=hits,
                          loss=loss, weighted=weighted, rows=rows))

    # --- unary: c3 * u(c1 * x1 + c2) on the dataset of u's domain
    for u in UNARY:
        ds = next((d for d, ops in UNARY_DATA.items() if u in ops), "normal")
        c2 = {"acosh": 1.0, "unit": 0.125}.get(u if u == "acosh" else ds, 0.25)
        add(f"unary/{u}", "unary", ds, "{2} * %s({0} * x1 + {1})" % u, (0.75, c2, 1.5), [f"U:{u.upper()}"])
    # --- binary: every operand position the gradient compiler emits
    g = "cos(x2 * {1})"
    A, B = "(cos(x1 * {0}) + cos(x2 * {1}))", "cos(x3 * {2})"
    for op, enum in BINARY.items():
        c1 = {"^": 1.5, "mod": 2.75, "/": 1.5, "atan2": 1.5}.get(op, 0.84375)
        forms = [("CL", call(op, "{0}", g), (c1, 0.25)), ("CR", call(op, g, "{0}"), ({"mod": 0.40625}.get(op, c1), 0.25)),
                 ("FL", call(op, "x1", g), (0.0, 0.25)), ("FR", call(op, g, "x1"), (0.0, 0.25)),
                 ("SL", call(op, A, B), (0.25, 0.3125, 0.375)), ("SR", call(op, B, A), (0.25, 0.3125, 0.375)),
                 ("FR", call(op, "{0}", "x1"), (1.25,)), ("CR", call(op, "x1", "{0}"), (1.25,)),
                 ("CR", call(op, "{0}", "{1}"), (1.25, 0.75))]
        for k, (v, tmpl, consts) in enumerate(forms):
            if "{0}" not in tmpl:  # (feature forms: g's constant is the only one)
                tmpl, consts = tmpl.replace("{1}", "{0}"), consts[1:]
            if op in PIECEWISE_CONSTANT:  # zero gradient for the operands: a further constant that has one
                tmpl, consts = "{%d} * " % len(consts) + tmpl, tuple(consts) + (1.5,)
            tag = ("CL CR FL FR SL SR leafCX leafXC leafCC".split())[k]
            add(f"binary/{enum.lower()}/{tag}", "binary", "pos", tmpl, consts, [f"B:{enum}:{variant(op, v)}"])
    # --- ^ edges: base exactly 0 with exponents 2 and 3, negative bases with an integer exponent (a feature)
    add("pow/zero_and_negative_base", "binary", "powint", "{1} * ((x1 * {0}) ^ x3)", (0.75, 1.5), ["B:POW:FR"])
    # --- tangent windows: 20 constants (a ^ and an atan2 constant operand at slots >= 16), 70 constants (cval1)
    term = lambda k: "{%d} * cos(x%d + {%d})" % (2 * k, 1 + k % 3, 2 * k + 1)  # noqa: E731
    cs = lambda n: [((7 * k) % 16 + 4) / 16 for k in range(n)]  # noqa: E731
    t20 = " + ".join(term(k) for k in range(8)) + " + (cos(x1 * {16}) ^ {17}) + atan2({18}, cos(x2 * {19}))"
    add("windows/20_constants", "binary", "pos", t20, cs(16) + [0.25, 1.5, 0.75, 0.25],
        ["B:POW:CR", "B:ATAN2:CL", "SLOT>=16"], weighted=True)
    t70 = " + ".join(term(k) for k in range(34)) + " + atan2({68} * cos(x1), {69})"
    add("windows/70_constants", "binary", "pos", t70, cs(70), ["B:ATAN2:CR", "SLOT>=64"], weighted=True)
    # --- the loss catalog on c1 * x1 + c2 * x2 + c3, unweighted and weighted
    for spec in CATALOG:
        for weighted in (False, True):
            add(f"loss/{spec}/{'weighted' if weighted else 'plain'}", "loss", "normal", "{0} * x1 + {1} * x2 + {2}",
                (1.25, -0.5, 0.5), [], loss=spec, weighted=weighted)
    # --- a weighted row view with repeats on the general path, L1HingeLoss
    rows = np.random.default_rng(7).integers(0, N_ROWS, 150).tolist()
    add("gather/general_l1hinge", "binary", "pos", "{0} * atan2(max(x1 ^ {1}, {2}), mod(x2, {3})) - {4}",
        (2.0, 1.5, 1.25, 0.75, 1.5), ["B:POW:CR", "B:MAX:CR", "B:MOD:CR", "B:ATAN2:SL"], loss="L1HingeLoss()",
        weighted=True, rows=rows)
    # --- parametric: a parameter as either operand of every binary operator
    gp = "cos(x2 * {0})"
    for op, enum in BINARY.items():
        forms = [("PL", call(op, "p1", gp), (0.25,), True), ("PR", call(op, gp, "p1"), (0.25,), True),
                 ("PR", call(op, "p1", "p2"), (), False)]
        for k, (v, tmpl, consts, _) in enumerate(forms):
            if op in PIECEWISE_CONSTANT or not consts:
                tmpl, consts = "{%d} * " % len(consts) + tmpl, tuple(consts) + (1.5,)
            add(f"param/{enum.lower()}/{('PL', 'PR', 'PP')[k]}", "param", "pos", tmpl, consts,
                [f"P:{enum}:{variant(op, v)}"] + (["LOADP"] if k == 2 else []))
    add("param/p2_only", "param", "pos", "{1} * atan2(p2, cos(x1 * {0}))", (0.25, 1.5), ["P:ATAN2:PL"])
    # (a parameter leaf opening the second operand of a stack binary: LOAD_PARAM_PUSH)
    add("param/stack_push", "param", "pos", "cos(x1 * {0}) - atan2(p2, p1)", (0.25,), ["P:ATAN2:PR", "LOADP_PUSH"])
    # (rows without class 3: that column of the gradient is exactly 0)
    ds = make_datasets()["pos"]
    add("param/class_absent", "param", "pos", "{1} * atan2(cos(x1 * {0}), p1) + p2", (0.25, 1.5),
        ["P:ATAN2:PR", "P:ADD:PR"], rows=[r for r in range(N_ROWS) if ds["cls"][r] != 3][::2])
    return cases


def solve(case, datasets):
    """The case's reference, its constants stepped by 1/256 while a row sits within MARGIN of a kink."""
    data = mp_data(datasets[case["dataset"]], case["rows"])
    P = P_MATRIX if GROUPS[case["group"]][2] else None
    base = case["consts"]
    trials = [list(base)] + [[c + (j / 256 if i == k else 0) for i, c in enumerate(base)]
                             for j in range(1, 33) for k in range(len(base))]
    for consts in trials:
        expr = case["template"].format(*[f"({c!r})" for c in consts])
        try:
            ref = reference(expr, case["loss"], data, case["weighted"], P)
        except Kink as e:
            last = e
            continue
        assert len(ref["grad"]) == len(consts) + (6 if P else 0) and all(float(np.float32(c)) == c for c in consts)
        return expr, ref
    raise SystemExit(f"{case['name']}: no constants off the kinks ({last})")


def main():
    datasets = make_datasets()
    out = {"generator": "tests/golden/make_grad_rule_fixtures.py (mpmath %s, %d digits)" % (mpmath.__version__, mp.dps),
           "note": "grad: d loss / d scalar (constants in pre-order, then P column-major); u32 / u64: the error "
                   "unit eps_T sum|row terms| / denom; zero: every row term is exactly 0",
           "datasets": datasets, "parameters": P_MATRIX,
           "groups": {k: dict(unary=v[0], binary=v[1], max_parameters=v[2]) for k, v in GROUPS.items()},
           "cases": []}
    for case in case_list():
        expr, ref = solve(case, datasets)
        entry = dict(name=case["name"], group=case["group"], dataset=case["dataset"], expr=expr, loss_spec=case["loss"],
                     weighted=case["weighted"], hits=case["hits"], constants=Tree(expr).constants, **ref)
        if case["rows"] is not None:
            entry["rows"] = case["rows"]
        out["cases"].append(entry)
        print(case["name"], expr, file=sys.stderr)
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, len(out["cases"]), "cases,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
