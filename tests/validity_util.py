"""TEST HELPER: the `complete` flag as two rules, the forms that exercise them and their data.

DynamicExpressions' evaluation handles every node's output in one of three ways: it is array-checked
(isfinite(sum(array))) by its parent or as the root; in the two fused degree-1 forms it is scalar-checked and
replaced by +Inf, which the next check sees; or it is a constant and is scalar-checked.  Hence

  rule A  a node whose value is non-finite on any row makes the tree incomplete, whatever a later operator
          makes of that value (`inv(exp(x))`, `tanh(..)`, `x > ..`, `cond`, `min`, `atan2(1, ..)`);
  rule B  an array of finite values whose sum overflows makes the tree incomplete if and only if the node is
          array-checked.

`analyse` restates the control flow that decides which nodes are array-checked and which substitute +Inf;
`evaluate` computes every node's array with plain numpy / math; `verdict` applies the two rules.  Nothing
here imports the oracle or the library's evaluator: the CPU tests compare the three.

Rule A forms are absorber(producer, other operand) under four wrappers.  A producer is benign on every row but
one; the control dataset lacks that row's value.  Forms are kept in groups, one batch and one dataset each:

  "E"  bad row: x1 = 1000 (exp(x1) = +Inf) and x3 = 0 (x2 / x3 = +Inf, -0.25 / x3 = -Inf)
  "L"  bad row: x1 = -1 (log(x1) = NaN)
  "K"  the producer is a constant subtree (exp(1000.0), log(-1.0)): incomplete on any data, by the constant alone

Benign rows: x1 in (1.1, 2.5), so that exp(x1) > 1 (acosh, log, sqrt hold) and log(x1) in (0, 1) (asin, acos,
atanh hold); x2 in (0.1, 0.4); x3 in (1, 2), so that x2 / x3 lies in (0, 1).  A (producer, absorber, position)
triple is left out only where the absorber is not finite on the producer's benign values; `excluded()` lists them
with the reason.
"""
import functools
import math
import re
from fractions import Fraction

import numpy as np

from sr_amd import Options, flatten_trees, parse_expression

UNARY = ("neg square cube exp cos sin tan log log2 log10 log1p sqrt abs sign tanh sinh cosh atan asin acos acosh atanh "
         "asinh relu inv erf erfc gamma round floor ceil exp2 expm1").split()
BINARY = "+ - * / ^ max min mod > < >= <= cond logical_or logical_and atan2".split()
BASIC_UNARY = "neg square cube exp cos sin log sqrt abs".split()
BASIC_BINARY = "+ - * /".split()
OPSETS = {"basic": dict(binary_operators=BASIC_BINARY, unary_operators=BASIC_UNARY),
          "full": dict(binary_operators=BINARY, unary_operators=UNARY),
          # the catalog less gamma, the one operator without a gradient rule (sr_unary_grad_supported)
          "grad": dict(binary_operators=BINARY, unary_operators=[u for u in UNARY if u != "gamma"])}
DTYPES = {"float32": np.float32, "float64": np.float64}
INFIX = ("+", "-", "*", "/", "^", ">", "<", ">=", "<=")
NF = 3

# operators that map some non-finite operand to a finite value (the other operand benign): the forms with power
UNARY_ABSORBING = {"exp", "sign", "tanh", "atan", "relu", "inv", "erf", "erfc", "exp2", "expm1"}
BINARY_ABSORBING = set(BINARY) - {"+", "-", "*"}
# why an absorber may be non-finite on a producer's benign values
DOMAIN = {"log": "x > 0", "log2": "x > 0", "log10": "x > 0", "log1p": "x > -1", "sqrt": "x >= 0", "acosh": "x >= 1",
          "asin": "|x| <= 1", "acos": "|x| <= 1", "atanh": "|x| < 1", "inv": "x != 0", "gamma": "x no pole", "/": "y != 0",
          "^": "x >= 0 or y an integer; no negative power of 0", "mod": "y != 0"}


@functools.lru_cache(maxsize=None)
def options(opset):
    return Options(**OPSETS[opset])


# ------------------------------------------------------------------------------------------- operators in numpy
def _map(f, x):
    return np.array([f(float(v)) for v in x], dtype=np.float64)


def _gamma(v):
    if math.isnan(v) or v == -math.inf:
        return math.nan
    try:
        g = math.gamma(v)
    except (ValueError, OverflowError):
        return math.nan
    return math.nan if math.isinf(g) else g


def np_unary(name, x, T):
    """The catalog's unary operator (the reference's safe_ forms: NaN outside the domain) on an array of T."""
    x = np.asarray(x, dtype=T)
    nan = T(np.nan)
    with np.errstate(all="ignore"):
        if name in ("log", "log2", "log10"):
            return np.where(x > 0, getattr(np, name)(np.where(x > 0, x, 1)), nan).astype(T)
        if name == "log1p":
            return np.where(x > -1, np.log1p(np.where(x > -1, x, 0)), nan).astype(T)
        if name == "sqrt":
            return np.where(x >= 0, np.sqrt(np.where(x >= 0, x, 0)), nan).astype(T)
        if name in ("asin", "acos", "atanh"):
            f = {"asin": np.arcsin, "acos": np.arccos, "atanh": np.arctanh}[name]
            ok = (x >= -1) & (x <= 1)
            return np.where(ok, f(np.where(ok, x, 0)), nan).astype(T)
        if name == "acosh":
            return np.where(x >= 1, np.arccosh(np.where(x >= 1, x, 1)), nan).astype(T)
        simple = {"neg": lambda: -x, "square": lambda: x * x, "cube": lambda: x * x * x, "exp": lambda: np.exp(x),
                  "cos": lambda: np.cos(x), "sin": lambda: np.sin(x), "tan": lambda: np.tan(x), "abs": lambda: np.abs(x),
                  "sign": lambda: np.sign(x), "tanh": lambda: np.tanh(x), "sinh": lambda: np.sinh(x),
                  "cosh": lambda: np.cosh(x), "atan": lambda: np.arctan(x), "asinh": lambda: np.arcsinh(x),
                  "relu": lambda: np.where(x > 0, x, np.copysign(T(0), x)), "inv": lambda: T(1) / x,
                  "round": lambda: np.rint(x), "floor": lambda: np.floor(x), "ceil": lambda: np.ceil(x),
                  "exp2": lambda: np.exp2(x), "expm1": lambda: np.expm1(x),
                  "erf": lambda: _map(math.erf, x), "erfc": lambda: _map(math.erfc, x), "gamma": lambda: _map(_gamma, x)}
        return np.asarray(simple[name]()).astype(T)


def _pow(x, y):
    if math.isnan(x) or math.isnan(y):
        return math.nan
    if math.isfinite(y) and y == math.trunc(y):  # (y - trunc(y) == 0: an infinite exponent is no integer)
        if y < 0 and x == 0:
            return math.nan
    else:
        if (y > 0 and x < 0) or (y < 0 and x <= 0):
            return math.nan
    try:
        return math.pow(x, y)
    except OverflowError:
        return math.inf
    except ValueError:
        return math.nan


def _mod(x, y):
    if math.isnan(x) or math.isnan(y) or math.isinf(x) or y == 0:
        return math.nan
    r = math.fmod(x, y)
    if r == 0:
        return math.copysign(r, y)
    return r + y if (r > 0) != (y > 0) else r


def np_binary(name, a, b, T):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=T), np.asarray(b, dtype=T))
    one, zero = T(1), T(0)
    with np.errstate(all="ignore"):
        if name in ("+", "-", "*", "/"):
            return {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide}[name](a, b).astype(T)
        if name == "^":
            return np.array([_pow(float(x), float(y)) for x, y in zip(a, b)], dtype=np.float64).astype(T)
        if name == "mod":
            return np.array([_mod(float(x), float(y)) for x, y in zip(a, b)], dtype=np.float64).astype(T)
        if name == "max":  # (a NaN operand is returned; the sign of zero plays no part here)
            return np.where(np.isnan(a), a, np.where(np.isnan(b), b, np.where(b > a, b, a))).astype(T)
        if name == "min":
            return np.where(np.isnan(a), a, np.where(np.isnan(b), b, np.where(b < a, b, a))).astype(T)
        if name in (">", "<", ">=", "<="):
            f = {">": np.greater, "<": np.less, ">=": np.greater_equal, "<=": np.less_equal}[name]
            return np.where(f(a, b), one, zero).astype(T)
        if name == "cond":
            return np.where(a > 0, b, np.copysign(zero, b)).astype(T)
        if name == "logical_or":
            return np.where((a > 0) | (b > 0), one, zero).astype(T)
        if name == "logical_and":
            return np.where((a > 0) & (b > 0), one, zero).astype(T)
        if name == "atan2":
            return np.arctan2(a, b).astype(T)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------- the two rules
def op_name(node, operators):
    from sr_amd.operators import print_name

    return print_name(operators.ops[node.degree][node.op - 1])


def _index(tree):
    order = tree.preorder()
    return order, {id(n): k for k, n in enumerate(order)}


def _is_const(n):
    if n.degree == 0:
        return bool(n.constant)
    return _is_const(n.l) and (n.degree == 1 or _is_const(n.r))


def analyse(tree):
    """DynamicExpressions' _eval_tree_array control flow as sets of pre-order node indices: `checked` (the arrays
    is_valid_array sees, root included), `infsub` (the outer nodes of deg1_l2_ll0_lr0 / deg1_l1_ll0: non-finite
    inner value -> +Inf), `folded` (roots of constant subtrees: dispatch_constant_tree) and `role` (per node, how
    its parent treats it)."""
    _, at = _index(tree)
    checked, infsub, folded, role = set(), set(), set(), {0: "root"}

    def leaf(n):
        return n.degree == 0

    def walk(n):
        if n.degree == 0:
            return
        if _is_const(n):  # the constant-tree fold comes first
            folded.add(at[id(n)])
            return
        if n.degree == 1:
            c = n.l
            if c.degree == 2 and leaf(c.l) and leaf(c.r):
                infsub.add(at[id(n)])
                role[at[id(c)]] = "deg1_l2_ll0_lr0.child"
                role[at[id(c.l)]], role[at[id(c.r)]] = "deg1_l2_ll0_lr0.ll", "deg1_l2_ll0_lr0.lr"
            elif c.degree == 1 and leaf(c.l):
                infsub.add(at[id(n)])
                role[at[id(c)]] = "deg1_l1_ll0.child"
                role[at[id(c.l)]] = "deg1_l1_ll0.ll"
            else:  # the child is evaluated and array-checked, a bare feature too
                walk(c)
                checked.add(at[id(c)])
                role[at[id(c)]] = "deg1.feature" if leaf(c) else ("deg1.const" if _is_const(c) else "deg1.child")
            return
        a, b = n.l, n.r
        if leaf(a) and leaf(b):
            role[at[id(a)]], role[at[id(b)]] = "deg2_l0_r0.left", "deg2_l0_r0.right"
        elif leaf(b):
            walk(a)
            checked.add(at[id(a)])
            role[at[id(a)]], role[at[id(b)]] = ("deg2_r0.const" if _is_const(a) else "deg2_r0.left"), "deg2_r0.right"
        elif leaf(a):
            walk(b)
            checked.add(at[id(b)])
            role[at[id(a)]], role[at[id(b)]] = "deg2_l0.left", ("deg2_l0.const" if _is_const(b) else "deg2_l0.right")
        else:
            for c, side in ((a, "left"), (b, "right")):
                walk(c)
                checked.add(at[id(c)])
                role[at[id(c)]] = "deg2.const" if _is_const(c) else "deg2." + side

    walk(tree)
    checked.add(0)  # the root is always checked
    return dict(checked=checked, infsub=infsub, folded=folded, role=role)


def evaluate(tree, X, T, operators):
    """{pre-order index: the node's array in T} for the nodes DynamicExpressions materialises (every node outside a
    folded constant subtree; a folded subtree's root holds its scalar), with the fused forms' +Inf substitution;
    and the list of scalars the constant fold went through."""
    _, at = _index(tree)
    a = analyse(tree)
    n = X.shape[1]
    vals, scalars = {}, []

    def scalar(m):
        if m.degree == 0:
            v = np.array([m.val], dtype=T)
        elif m.degree == 1:
            v = np_unary(op_name(m, operators), scalar(m.l), T)
        else:
            v = np_binary(op_name(m, operators), scalar(m.l), scalar(m.r), T)
        scalars.append(v[0])
        return v

    def rec(m):
        k = at[id(m)]
        if m.degree == 0:
            if m.constant:
                scalars.append(T(m.val))
            v = np.full(n, m.val, dtype=T) if m.constant else np.array(X[m.feature - 1], dtype=T)
        elif k in a["folded"]:
            v = np.full(n, scalar(m)[0], dtype=T)
        elif m.degree == 1:
            c = rec(m.l)
            v = np_unary(op_name(m, operators), c, T)
            if k in a["infsub"]:
                v = np.where(np.isfinite(c), v, T(np.inf)).astype(T)
        else:
            v = np_binary(op_name(m, operators), rec(m.l), rec(m.r), T)
        vals[k] = v
        return v

    rec(tree)
    return vals, scalars


def exact_sum(v):
    """(sum, sum of magnitudes) of a finite array as Fractions."""
    u, cnt = np.unique(np.asarray(v, dtype=np.float64), return_counts=True)
    s = sum((Fraction(float(x)) * int(c) for x, c in zip(u, cnt)), Fraction(0))
    m = sum((abs(Fraction(float(x))) * int(c) for x, c in zip(u, cnt)), Fraction(0))
    return s, m


def verdict(tree, X, T, operators):
    """(complete, by the constants alone) from the two rules.  Asserts that no summation order could change a
    checked array's verdict: its magnitudes sum to at most 0.8 floatmax, or it has one sign and sums to at least
    1.4 floatmax."""
    a = analyse(tree)
    vals, scalars = evaluate(tree, X, T, operators)
    order, _ = _index(tree)
    fmax = Fraction(float(np.finfo(T).max))
    static = not all(np.isfinite(s) for s in scalars)
    complete = not static
    for k, v in vals.items():  # rule A
        if not np.isfinite(v).all():
            complete = False
    if not complete:
        return False, static
    for k in sorted(a["checked"]):  # rule B
        s, m = exact_sum(vals[k])
        if m * 10 <= fmax * 8:
            continue
        assert abs(s) == m and m * 10 >= fmax * 14, ("a sum near floatmax", k, float(m / fmax))
        complete = False
        if _is_const(order[k]):
            static = True
    return complete, static and not complete


# ------------------------------------------------------------------------------------------- rule A: data
def rule_a_data(n, T, bad_row):
    """{"control", "E", "L"}: X [3, n] in T (module docstring); y is zeros."""
    j = np.arange(n, dtype=np.float64)
    frac = lambda a: (j * a) % 1.0  # noqa: E731
    X = np.stack([1.1 + 1.4 * frac(0.6180339887), 0.1 + 0.3 * frac(0.7548776662), 1.0 + frac(0.5698402910)]).astype(T)
    assert X[0].min() >= 1.1 and X[0].max() < 2.5 and X[1].min() >= 0.1 and X[1].max() < 0.4
    assert X[2].min() >= 1 and X[2].max() < 2
    out = {"control": X}
    e = X.copy()
    e[0, bad_row], e[2, bad_row] = T(1000.0), T(0.0)
    l = X.copy()
    l[0, bad_row] = T(-1.0)
    out["E"], out["L"] = e, l
    out["K"] = X  # (constant producers: no row matters)
    for v in out.values():
        v.setflags(write=False)
    return out


# producers: kind -> (group, expression, sign class of the non-finite value)
PRODUCERS = {
    "exp": ("E", "exp(x1)", "+inf"),
    "neg_exp": ("E", "neg(exp(x1))", "-inf"),
    "div": ("E", "(x2 / x3)", "+inf"),
    "div_neg": ("E", "(-0.25 / x3)", "-inf"),
    "inf_minus_inf": ("E", "(exp(x1) - exp(x1))", "nan"),
    "zero_times_inf": ("E", "(0.0 * exp(x1))", "nan"),
    "log": ("L", "log(x1)", "nan"),
    "log_above_1": ("L", "(log(x1) + 2.0)", "nan"),  # for acosh alone: its domain excludes log(x1) < 1
    # x3 as an operand beside a computed value (a parameter operand PR / PL in the parametric twin); a few absorbers
    "div_sub": ("E", "((x2 + 0.5) / x3)", "+inf"),
    "log_sub": ("E", "log((x3 - (x2 + 0.5)))", "nan"),
    # the non-finite value first appears as a post-binary constant's output (LOAD x3, POST abs, PBC 2.0 / tos)
    "const_over_abs": ("E", "(2.0 / abs(x3))", "+inf"),
    "const_inf": ("K", "exp(1000.0)", "+inf"),
    "const_nan": ("K", "log(-1.0)", "nan"),
}
POSITIONS = ("P,feature", "feature,P", "P,const", "const,P", "P,subtree", "subtree,P")
OTHER = {"feature": "x2", "const": "2.0", "subtree": "(x2 + 0.5)"}


def _deep():
    """{} * x2^15 as a balanced product of 16 operands: more than two operand-stack slots, so the tree runs on the
    LDS-stack kernels, never on the register-stack ones."""
    terms = ["{}"] + ["x2"] * 15
    while len(terms) > 1:
        terms = [f"({a} * {b})" for a, b in zip(terms[::2], terms[1::2])]
    return terms[0]


WRAPPERS = {"root": "{}", "plus_feature": "({} + x2)", "times_const": "({} * 0.5)", "cos": "cos({})", "deep": _deep()}


def _call(name, *args):
    if name in INFIX:
        return f"({args[0]} {name} {args[1]})"
    return f"{name}({', '.join(args)})"


def _needs(kind, opset):
    un, bi = OPSETS[opset]["unary_operators"], OPSETS[opset]["binary_operators"]
    need = {"exp": ["exp"], "neg_exp": ["neg", "exp"], "div": ["/"], "div_neg": ["/"], "inf_minus_inf": ["exp", "-"],
            "zero_times_inf": ["exp", "*"], "div_sub": ["/", "+"], "const_over_abs": ["/", "abs"],
            "log_sub": ["log", "-", "+"], "log": ["log"], "log_above_1": ["log", "+"], "const_inf": ["exp"],
            "const_nan": ["log"]}[kind]
    return all(o in un or o in bi for o in need)


def _benign(kind, T):
    """The producer's values on the control rows (a constant producer has none: it is never benign)."""
    X = rule_a_data(257, T, 0)["control"]
    x1, x2, x3 = X
    with np.errstate(all="ignore"):
        return {"exp": lambda: np.exp(x1), "neg_exp": lambda: -np.exp(x1), "div": lambda: x2 / x3,
                "div_neg": lambda: T(-0.25) / x3, "inf_minus_inf": lambda: np.exp(x1) - np.exp(x1),
                "zero_times_inf": lambda: T(0) * np.exp(x1), "log": lambda: np.log(x1),
                "log_above_1": lambda: np.log(x1) + T(2), "div_sub": lambda: (x2 + T(0.5)) / x3,
                "const_over_abs": lambda: T(2) / np.abs(x3),
                "log_sub": lambda: np.log(x3 - (x2 + T(0.5)))}[kind]().astype(T)


def _other_values(what, T):
    X = rule_a_data(257, T, 0)["control"]
    return {"feature": X[1], "const": np.full(257, T(2.0)), "subtree": (X[1] + T(0.5)).astype(T)}[what]


def _apply(absorber, position, p, T):
    """The absorber at producer values p, the other operand benign."""
    if position is None:
        return np_unary(absorber, p, T)
    first, second = position.split(",")
    o = _other_values(first if second == "P" else second, T)[:len(p)]
    return np_binary(absorber, p, o, T) if first == "P" else np_binary(absorber, o, p, T)


@functools.lru_cache(maxsize=None)
def _fits(kind, absorber, position):
    """The absorber is finite on the producer's benign values, in both precisions."""
    if PRODUCERS[kind][0] == "K":
        return True
    return all(np.isfinite(_apply(absorber, position, _benign(kind, T), T)).all() for T in DTYPES.values())


def absorbs(absorber, position, sign):
    """The evidence of absorption: the absorber at the producer's non-finite value, by numpy / math, is finite."""
    v = {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan}[sign]
    return all(np.isfinite(_apply(absorber, position, np.full(257, v, dtype=T), T)).all() for T in DTYPES.values())


class Form:
    __slots__ = ("expr", "group", "kind", "absorber", "position", "wrapper", "absorbing")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def __repr__(self):
        return f"Form({self.expr!r}, {self.group}, {self.kind}, {self.absorber}, {self.position}, {self.wrapper})"


@functools.lru_cache(maxsize=None)
def _rule_a(opset):
    un, bi = OPSETS[opset]["unary_operators"], OPSETS[opset]["binary_operators"]
    forms, left_out = [], []
    slots = [(a, None) for a in un] + [(a, pos) for a in bi for pos in POSITIONS]
    for absorber, pos in slots:
        for kind, (group, p, sign) in PRODUCERS.items():
            if not _needs(kind, opset):
                continue
            if kind == "log_above_1" and absorber != "acosh":
                continue
            if kind in ("div_sub", "log_sub", "const_over_abs") and absorber not in ("cos", "abs", "+", "/"):
                continue
            if group == "K" and pos not in (None, "P,feature", "feature,P"):
                continue  # (a constant producer beside a constant would fold the absorber too)
            if not _fits(kind, absorber, pos):
                left_out.append((kind, absorber, pos, f"{absorber} needs {DOMAIN[absorber]}: not so on the benign "
                                 f"values of {p}"))
                continue
            if pos is None:
                inner = _call(absorber, p)
            else:
                first, second = pos.split(",")
                inner = _call(absorber, p, OTHER[second]) if first == "P" else _call(absorber, OTHER[first], p)
            for wname, w in WRAPPERS.items():
                if group == "K" and wname != "plus_feature":
                    continue  # (one wrapper that keeps the tree from folding as a whole)
                forms.append(Form(expr=w.format(inner), group=group, kind=kind, absorber=absorber, position=pos,
                                  wrapper=wname, absorbing=absorbs(absorber, pos, sign)))
    _assert_coverage(opset, slots, forms)
    return tuple(forms), tuple(left_out)


def _assert_coverage(opset, slots, forms):
    """Every operator in every listed position, under every wrapper, with an infinite and with a NaN producer that
    depends on the data; and an absorbing form for every operator that has one."""
    for absorber, pos in slots:
        for wname in WRAPPERS:
            signs = {PRODUCERS[f.kind][2] for f in forms
                     if (f.absorber, f.position, f.wrapper) == (absorber, pos, wname) and f.group != "K"}
            assert signs & {"+inf", "-inf"} and "nan" in signs, (opset, absorber, pos, wname, signs)
    un, bi = OPSETS[opset]["unary_operators"], OPSETS[opset]["binary_operators"]
    have = {f.absorber for f in forms if f.absorbing}
    want = (UNARY_ABSORBING & set(un)) | (BINARY_ABSORBING & set(bi))
    assert have == want, (opset, sorted(have ^ want))
    for a in want & set(bi):  # a binary absorber: the producer on every side from which it can absorb
        sides = {f.position.split(",")[0] == "P" for f in forms if f.absorber == a and f.absorbing}
        can = {pos.split(",")[0] == "P" for pos in POSITIONS for sign in ("+inf", "-inf", "nan") if absorbs(a, pos, sign)}
        assert sides == can and sides, (opset, a, sides, can)


def rule_a_forms(opset, group=None):
    forms = _rule_a(opset)[0]
    return forms if group is None else tuple(f for f in forms if f.group == group)


def excluded(opset):
    """[(producer kind, absorber, position, reason)] left out of the rule A set."""
    return _rule_a(opset)[1]


GROUPS = ("E", "L", "K")


@functools.lru_cache(maxsize=None)
def rule_a_batch(opset, group, dtype_name, parametric=False):
    """The group's forms as one TreeBatch.  The parametric twin reads p1 for x1 and p2 for x3 (leaves x4 / x5 of a
    plain batch over 5 features, for parametric_util.to_parametric)."""
    opts = options(opset)
    exprs = [f.expr for f in rule_a_forms(opset, group)]
    if parametric:
        exprs = [e.replace("x1", "x4").replace("x3", "x5") for e in exprs]
    return flatten_trees([parse_expression(e, opts) for e in exprs], DTYPES[dtype_name])


def rule_a_params(group, T):
    """[2, 2] parameters (p1, p2) x (class 1 benign, class 2 bad) standing in for x1 and x3."""
    bad = {"E": (1000.0, 0.0), "L": (-1.0, 1.5), "K": (2.0, 1.5)}[group]
    return np.array([[2.0, bad[0]], [1.5, bad[1]]], dtype=T)


# ------------------------------------------------------------------------------------------- gradients of the controls
def _d_unary(name, x, y):
    """d op(x) / dx given y = op(x): the rules of forward-mode dual numbers (csrc/sr_ops.h: sr_unary_deriv)."""
    one = np.ones_like(x)
    with np.errstate(all="ignore"):
        return {"neg": lambda: -one, "square": lambda: 2 * x, "cube": lambda: 3 * x * x, "exp": lambda: y,
                "cos": lambda: -np.sin(x), "sin": lambda: np.cos(x), "tan": lambda: 1 + y * y, "log": lambda: 1 / x,
                "log2": lambda: 1 / (x * math.log(2)), "log10": lambda: 1 / (x * math.log(10)), "log1p": lambda: 1 / (1 + x),
                "sqrt": lambda: 0.5 / y, "abs": lambda: np.where(np.signbit(x), -one, one), "sign": lambda: 0 * one,
                "tanh": lambda: 1 - y * y, "sinh": lambda: np.cosh(x), "cosh": lambda: np.sinh(x),
                "atan": lambda: 1 / (1 + x * x), "asin": lambda: 1 / np.sqrt(1 - x * x),
                "acos": lambda: -1 / np.sqrt(1 - x * x), "acosh": lambda: 1 / np.sqrt(x * x - 1),
                "atanh": lambda: 1 / (1 - x * x), "asinh": lambda: 1 / np.sqrt(1 + x * x),
                "relu": lambda: np.where(x > 0, one, 0 * one), "inv": lambda: -(y * y),
                "erf": lambda: 2 / math.sqrt(math.pi) * np.exp(-(x * x)),
                "erfc": lambda: -2 / math.sqrt(math.pi) * np.exp(-(x * x)),
                "round": lambda: 0 * one, "floor": lambda: 0 * one, "ceil": lambda: 0 * one,
                "exp2": lambda: math.log(2) * y, "expm1": lambda: y + 1}[name]()


def _d_binary(name, a, b, r):
    """(d/da, d/db) of r = op(a, b) (sr_binary_partials): x^y has d/dy = r log x for x > 0, else 0."""
    one, zero = np.ones_like(r), np.zeros_like(r)
    with np.errstate(all="ignore"):
        if name == "+":
            return one, one
        if name == "-":
            return one, -one
        if name == "*":
            return b + zero, a + zero
        if name == "/":
            return 1 / b + zero, -r / b
        if name == "^":
            pa = np.where(a == 0, b * np.power(np.abs(a), b - 1), b * r / a)
            return pa, np.where(a > 0, r * np.log(np.where(a > 0, a, 1)), zero)
        if name == "max":
            return np.where(b > a, zero, one), np.where(b > a, one, zero)
        if name == "min":
            return np.where(b < a, zero, one), np.where(b < a, one, zero)
        if name == "mod":
            return one, -np.floor(a / b)
        if name == "cond":
            return zero, np.where(a > 0, one, zero)
        if name == "atan2":
            d = a * a + b * b
            return b / d, -a / d
    return zero, zero  # comparisons / logical operators: piecewise constant


def control_gradient_is_finite(tree, X, operators):
    """Forward-mode dual numbers in Float64 over the control rows: is every d prediction / d constant finite?  Not
    so where a partial derivative is infinite at the producer's benign value 0 (sqrt' at 0, y 0^(y - 1), 1 / 0 under
    mod): dual arithmetic then gives Inf, or NaN from 0 x Inf even for a constant elsewhere in the tree."""
    consts = [m for m in tree.preorder() if m.degree == 0 and m.constant]
    slot = {id(m): k for k, m in enumerate(consts)}
    n = X.shape[1]

    def rec(m):
        if m.degree == 0:
            t = np.zeros((len(consts), n))
            if m.constant:
                t[slot[id(m)]] = 1.0
                return np.full(n, float(m.val)), t
            return np.array(X[m.feature - 1], dtype=np.float64), t
        name = op_name(m, operators)
        with np.errstate(all="ignore"):
            if m.degree == 1:
                x, tx = rec(m.l)
                y = np_unary(name, x, np.float64)
                return y, _d_unary(name, x, y) * tx
            (a, ta), (b, tb) = rec(m.l), rec(m.r)
            r = np_binary(name, a, b, np.float64)
            pa, pb = _d_binary(name, a, b, r)
            return r, pa * ta + pb * tb

    v, t = rec(tree)
    assert np.isfinite(v).all()
    return bool(np.isfinite(t).all())


@functools.lru_cache(maxsize=None)
def singular_controls(opset, group):
    """Per form of the group: the control's gradient is not finite under dual arithmetic (a property of the form,
    not of a kernel), so "a finite gradient" cannot be asked of it."""
    opts = options(opset)
    if group == "K":  # (no control of this group is complete)
        return np.zeros(len(rule_a_forms(opset, group)), dtype=bool)
    X = rule_a_data(33, np.float64, 0)["control"]
    return np.array([not control_gradient_is_finite(parse_expression(f.expr, opts), X, opts.operators)
                     for f in rule_a_forms(opset, group)])


# ------------------------------------------------------------------------------------------- rule B
def rule_b_data(n, T):
    """x1 sums to 0.75 floatmax, x3 to 1.5 floatmax (so x1 * 2.0 and x1 + x1 overflow), x2 = 0.5: with 0.75
    the checked product (x1 + x1) * x2 would sum to 1.125 floatmax, inside the band `verdict` refuses."""
    fmax = float(np.finfo(T).max)
    X = np.stack([np.full(n, fmax / n * 0.75), np.full(n, 0.5), np.full(n, fmax / n * 1.5)]).astype(T)
    assert np.isfinite(X).all() and n >= 4
    X.setflags(write=False)
    return X


RULE_B_SEED = {
    True: ["cos(x1 * 2.0)", "cos(abs(x1))", "tanh(x1 + x1)", "tanh(tanh(x1 + x1))", "atan(neg(x1)) + x2",
           "atan(x1 * 2.0) * 0.5", "cos(x1 * 2.0) * 0.5 + x2", "atan2(x2, x1)", "inv(x1 * 2.0) + x2", "inv(x1 + x1) * x2",
           "(x1 * 1e-30) * x2", "x1 * 1e-30", "x3 * 1e-30", "cos(abs(x3))", "tanh(x3 * 1e-30) + x3 * 1e-30", "cos(x1)",
           "x1", "max(x1, x2) * 1e-30", "abs(x1) * 1e-30", "abs(neg(x1)) * 1e-30", "sqrt(abs(x1))", "sqrt(abs(x1)) * 2.0"],
    False: ["(x1 * 2.0) * 1e-30", "1e-30 * (x1 * 2.0)", "(x1 * 2.0) * (x2 * 1e-30)", "cos(abs(x1 * 2.0))",
            "atan2(x2, x1 * 2.0)", "inv((x1 + x1) * x2)", "cos(x3)", "x3", "abs(x3) * 1e-30", "max(x3, x2) * 1e-30",
            "(x2 + x2) * (x3 * 1.0)", "neg(neg(x3 * 1.0))"],
}
# forms whose only failing check rides on a fused POST unary / on a post-binary constant (asserted from the programs)
RULE_B_POST_CHECK, RULE_B_PBC_CHECK = "cos(abs(x1 * 2.0))", "cos(abs(x1) * 2.0)"
# the roles an overflowing array must appear in, somewhere in the set (analyse()'s role names)
RULE_B_ROLES = {"root", "deg1_l2_ll0_lr0.child", "deg1_l1_ll0.child", "deg1.child", "deg1.feature", "deg2_l0_r0.left",
                "deg2_l0_r0.right", "deg2_r0.left", "deg2_r0.right", "deg2_l0.left", "deg2_l0.right", "deg2.left",
                "deg2.right", "deg2.const", "deg2_l0.const", "deg2_r0.const"}


def _has(opset, expr):
    un, bi = OPSETS[opset]["unary_operators"], OPSETS[opset]["binary_operators"]
    return all(w in un or w in bi for w in re.findall(r"[a-z][a-z0-9]*(?=\()", expr))


@functools.lru_cache(maxsize=None)
def rule_b_forms(opset, dtype_name, n):
    """[(expression, complete)] for rule_b_data(n, T): the seed forms the operator set can express, the forms whose
    check rides on a POST unary or a post-binary constant, and constant subtrees K = floatmax / n * 1.5 (its array
    overflows) / H = K / 2 (it does not) in the roles where DynamicExpressions checks a constant array."""
    T = DTYPES[dtype_name]
    K = repr(float(T(float(np.finfo(T).max) / n * 1.5)))
    H = repr(float(T(float(np.finfo(T).max) / n * 0.75)))
    K2 = repr(float(T(float(np.finfo(T).max) / n * 3.0)))
    extra = {
        True: ["cos(abs(x1) * 1.0)", "cos((x1 + x2) * 1.0)", "((x1 + x2) * 1.0) * 1e-30", "cos(abs(x1 * 1.0))",
               "sin(x3 * 1.0) * x2", "x3 * x2",
               "x2 * x3", "cos(x1 + x1) + (x1 * 1e-30)", "(x2 * 1e-30) * x3", "x3 * (x2 * 1e-30)",
               f"(x2 * 1e-30) * ({H} * 1.0)", f"x2 * ({H} * 1.0)", f"({H} * 1.0) * x2", f"{H} * 1.0", H, f"cos({K} * 1.0)",
               f"cos(x2 * {K2})"],
        False: ["cos(abs(x1) * 2.0)", "(abs(x1) * 2.0) * 1e-30", "cos((x1 + x2) * 2.0)", "((x1 + x2) * 2.0) * 1e-30",
                "cos(abs(x1 + x1)) * x2", "abs(x1 * 2.0) * 1e-30",
                "x3 * 1.0", "x3 + x2", "(x3 * 1.0) * x2 + (x1 * 1e-30)", "(x2 * 1e-30) * (x3 * 1e-30 + x3)",
                "(x3 * 1e-30 + x3) * (x2 * 1e-30)", "cos(x3) * (x2 * x2)",
                f"(x2 * 1e-30) * ({K} * 1.0)", f"x2 * ({K} * 1.0)", f"({K} * 1.0) * x2", f"{K} * 1.0", K,
                f"cos(x2 * 0.0) * {K}"],
    }
    opts = options(opset)
    X = rule_b_data(n, T)
    forms = []
    for want in (True, False):
        for e in RULE_B_SEED[want] + extra[want]:
            if not _has(opset, e):
                continue
            got, _ = verdict(parse_expression(e, opts), X, T, opts.operators)
            assert got == want, (e, dtype_name, n, got)  # (the table's verdict is the restatement's)
            forms.append((e, want))
    assert len(forms) >= 40 and len(set(e for e, _ in forms)) == len(forms)
    return tuple(forms)


def rule_b_roles(opset, dtype_name, n):
    """The roles in which an array that overflows appears in the set."""
    T = DTYPES[dtype_name]
    opts = options(opset)
    X = rule_b_data(n, T)
    fmax = Fraction(float(np.finfo(T).max))
    seen = set()
    for e, _ in rule_b_forms(opset, dtype_name, n):
        tree = parse_expression(e, opts)
        a = analyse(tree)
        vals, _ = evaluate(tree, X, T, opts.operators)
        for k, v in vals.items():
            if k in a["role"] and np.isfinite(v).all() and exact_sum(v)[1] * 10 >= fmax * 14:
                seen.add(a["role"][k])
    return seen


@functools.lru_cache(maxsize=None)
def rule_b_batch(opset, dtype_name, n, parametric=False):
    """(batch, expected complete).  The parametric twin reads p1 for x1 and p2 for x3, as rule_a_batch's; with one
    class and rule_b_params it is the same tree on the same values."""
    opts = options(opset)
    forms = rule_b_forms(opset, dtype_name, n)
    exprs = [e.replace("x1", "x4").replace("x3", "x5") if parametric else e for e, _ in forms]
    tb = flatten_trees([parse_expression(e, opts) for e in exprs], DTYPES[dtype_name])
    return tb, np.array([c for _, c in forms], dtype=bool)


def rule_b_params(n, T):
    """[2, 1]: p1 and p2 hold the constant columns x1 and x3 of rule_b_data."""
    X = rule_b_data(n, T)
    return np.array([[X[0, 0]], [X[2, 0]]], dtype=T)
