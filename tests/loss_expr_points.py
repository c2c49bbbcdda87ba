"""TEST HELPER: expression-loss programs (csrc/sr_loss_expr.h) per element.

Three parts, shared by test_loss_expr_forms_host.py, test_gpu_loss_expr_forms.py and test_gpu_loss_expr_ops.py:

  * an exact reference: loss bodies parsed into tuples and evaluated recursively over ``fractions.Fraction`` (signed
    zeros carried as IEEE does), independent of csrc/sr_ops.h; d L / d p is the exact central difference with
    h = 2^-8 — exact for a degree of at most 2 inside a branch, so the reference holds no derivative rule;
  * a restatement of the header's documented live-value rule (``plan``): instruction kinds, DX / DY flags, leaf
    sources and live values of a body, from which the tests assert what the fixed table covers;
  * the device harness: ``device_elements`` (L and dL/dp per point, one one-row view per point) and ``device_mean``
    (the same points as one plain 1153-row dataset through the non-gathered builds).

What the harness can and cannot see.  A one-row view's loss is the f64 sum of a single T value divided by 1 (by
w_k, a power of two, when weighted): that value's bits — but for the sign of a zero, which the padding rows' +0.0
of the tile's sum removes.  ``device_elements`` therefore reads a zero's sign from a second call with the body
``1.0 / (BODY)``, whose +-Inf carries it (the same program, one more instruction).  A zero derivative is returned
as the device gives it; the central difference has no signed zero, so the tests compare it by value.
"""
import ast
import functools
from fractions import Fraction

import numpy as np

import loss_expr_util
import op_values_util
from sr_amd import (Dataset, LossExpression, Node, Options, eval_grad_batch, eval_grad_batch_views, eval_loss_batch,
                    eval_loss_batch_views, flatten_trees, get_context, parse_expression)

H = Fraction(1, 256)
KINK_MARGIN = Fraction(1, 16)
N_FULL = 1153  # two full 512-row tiles of the widest build (8 rows x 64 lanes) and a ragged tail
INFIX = ("+", "-", "*", "/", "^", ">", "<", ">=", "<=")
_PY_BIN = {ast.Add: "+", ast.Sub: "-", ast.Mult: "*", ast.Div: "/", ast.Pow: "^"}
_PY_CMP = {ast.Gt: ">", ast.Lt: "<", ast.GtE: ">=", ast.LtE: "<="}
EXACT_UNARY = ("neg", "abs", "square", "relu")
EXACT_BINARY = ("+", "-", "*", "/", "max", "min", ">", "<", ">=", "<=", "cond")


# ------------------------------------------------------------------------------------------------- bodies
def parse(body):
    """Body string -> tuples: ("p",) ("t",) ("w",) ("c", Fraction) ("u", name, a) ("b", name, a, b)."""
    def rec(e):
        if isinstance(e, ast.Constant):
            return ("c", Fraction(float(e.value)))
        if isinstance(e, ast.UnaryOp) and isinstance(e.op, ast.USub):
            if isinstance(e.operand, ast.Constant):
                return ("c", -Fraction(float(e.operand.value)))
            return ("u", "neg", rec(e.operand))
        if isinstance(e, ast.Name):
            assert e.id in "ptw", e.id
            return (e.id,)
        if isinstance(e, ast.BinOp):
            return ("b", _PY_BIN[type(e.op)], rec(e.left), rec(e.right))
        if isinstance(e, ast.Compare) and len(e.ops) == 1:
            return ("b", _PY_CMP[type(e.ops[0])], rec(e.left), rec(e.comparators[0]))
        if isinstance(e, ast.Call) and len(e.args) == 1:
            return ("u", e.func.id, rec(e.args[0]))
        if isinstance(e, ast.Call) and len(e.args) == 2:
            return ("b", e.func.id, rec(e.args[0]), rec(e.args[1]))
        raise ValueError(ast.dump(e))

    return rec(ast.parse(body.replace("^", "**"), mode="eval").body)


def render(e):
    if e[0] == "c":
        return repr(float(e[1]))
    if e[0] in "ptw":
        return e[0]
    if e[0] == "u":
        return f"{e[1]}({render(e[2])})"
    if e[1] in INFIX:
        return f"({render(e[2])} {e[1]} {render(e[3])})"
    return f"{e[1]}({render(e[2])}, {render(e[3])})"


def uses_w(e):
    return e[0] == "w" or any(uses_w(k) for k in e[2:] if e[0] in "ub")


def spec(body):
    """The ``elementwise_loss`` string: three arguments exactly when the body names the weight."""
    return f"loss(p, t, w) = {body}" if uses_w(parse(body)) else f"loss(p, t) = {body}"


# ------------------------------------------------------------------------------------------------- exact reference
# a value: (Fraction, negative-zero flag); the flag is set only on a zero
def _mk(v, neg=False):
    return (v, bool(neg) and v == 0)


def _sign(x):
    return x[0] < 0 or x[1]


def _neg(x):
    return (-x[0], (not x[1]) if x[0] == 0 else False)


def _add(a, b):
    if a[0] == 0 and b[0] == 0:
        return (Fraction(0), a[1] and b[1])
    return _mk(a[0] + b[0])  # (an exact cancellation is +0.0)


class Trace:
    """What one evaluation met: every node's value, every kink's distance, the branches taken."""

    def __init__(self):
        self.values, self.kinks, self.branch = [], [], []

    def kink(self, dist, taken):
        self.kinks.append(abs(dist))
        self.branch.append(bool(taken))


def ref_eval(e, p, t, w, tr=None):
    """L(p, t, w) of a parsed body over Fractions (the exact operators only)."""
    tr = tr if tr is not None else Trace()

    def rec(e):
        k = e[0]
        if k == "c":
            v = _mk(e[1])
        elif k in "ptw":
            v = _mk({"p": p, "t": t, "w": w}[k])
        elif k == "u":
            x = rec(e[2])
            if e[1] == "neg":
                v = _neg(x)
            elif e[1] == "abs":
                tr.kink(x[0], x[0] > 0)
                v = _mk(abs(x[0]))
            elif e[1] == "square":
                v = _mk(x[0] * x[0])
            elif e[1] == "relu":  # (x > 0) * x: false * x = copysign(0, x)
                tr.kink(x[0], x[0] > 0)
                v = x if x[0] > 0 else (Fraction(0), _sign(x))
            else:
                raise ValueError(e[1])
        else:
            a, b = rec(e[2]), rec(e[3])
            op = e[1]
            if op == "+":
                v = _add(a, b)
            elif op == "-":
                v = _add(a, _neg(b))
            elif op == "*":
                v = _mk(a[0] * b[0], _sign(a) != _sign(b))
            elif op == "/":
                assert b[0] != 0
                v = _mk(a[0] / b[0], _sign(a) != _sign(b))
            elif op in ("max", "min"):
                tr.kink(a[0] - b[0], a[0] > b[0])
                v = (a if a[0] > b[0] else b) if op == "max" else (a if a[0] < b[0] else b)
            elif op in (">", "<", ">=", "<="):
                tr.kink(a[0] - b[0], a[0] > b[0])
                v = _mk(Fraction(int((a[0] > b[0]) == (op[0] == ">"))))
            elif op == "cond":  # (a > 0) * b: false * b = copysign(0, b)
                tr.kink(a[0], a[0] > 0)
                v = b if a[0] > 0 else (Fraction(0), _sign(b))
            else:
                raise ValueError(op)
        tr.values.append(v[0])
        return v

    return rec(e), tr


def in_float32(v):
    return Fraction(float(np.float32(float(v)))) == v


def _to_float(x):
    return -0.0 if x[1] else float(x[0])


def reference(body, pts):
    """(value [n], derivative [n]) as Float64 arrays holding numbers exact in Float32 (asserted, with every
    intermediate value), the points at least KINK_MARGIN from every kink and the two difference points on the
    point's own branches (asserted)."""
    e = parse(body)
    val, der = [], []
    for p, t, w in pts:
        v, tr = ref_eval(e, p, t, w)
        vp, trp = ref_eval(e, p + H, t, w)
        vm, trm = ref_eval(e, p - H, t, w)
        assert all(d >= KINK_MARGIN for d in tr.kinks), (body, p, t, w, "kink within 1/16")
        assert tr.branch == trp.branch == trm.branch, (body, p, t, w, "difference point on another branch")
        d = (vp[0] - vm[0]) / (2 * H)
        assert all(in_float32(x) for x in tr.values) and in_float32(d), (body, p, t, w, "not exact in Float32")
        val.append(_to_float(v))
        der.append(float(d))
    return np.array(val), np.array(der)


def degree(e):
    """Degree in p inside a branch."""
    if e[0] in "ctw":
        return 0
    if e[0] == "p":
        return 1
    if e[0] == "u":
        return degree(e[2]) * (2 if e[1] == "square" else 1)
    a, b = degree(e[2]), degree(e[3])
    op = e[1]
    if op == "*":
        return a + b
    if op == "/":
        assert b == 0
        return a
    if op in (">", "<", ">=", "<="):
        return 0
    if op == "cond":
        return b
    return max(a, b)


def mul_depth(e):
    """The most multiplications (`*`, square) on a root-to-leaf path."""
    if e[0] in "cptw":
        return 0
    own = int((e[0] == "u" and e[1] == "square") or (e[0] == "b" and e[1] == "*"))
    return own + max(mul_depth(k) for k in e[2:])


def divisors_ok(e):
    """Every divisor is a product of the weight and power-of-two constants."""
    def pow2(d):
        if d[0] == "w":
            return True
        if d[0] == "c":
            return d[1] > 0 and (d[1].numerator == 1 or d[1].denominator == 1) and \
                (d[1].numerator & (d[1].numerator - 1)) == 0 and (d[1].denominator & (d[1].denominator - 1)) == 0
        return d[0] == "b" and d[1] == "*" and pow2(d[2]) and pow2(d[3])

    if e[0] in "cptw":
        return True
    if e[0] == "b" and e[1] == "/" and not pow2(e[3]):
        return False
    return all(divisors_ok(k) for k in e[2:])


def constants_ok(e):
    if e[0] == "c":
        return (e[1] * 4).denominator == 1
    return all(constants_ok(k) for k in e[2:]) if e[0] in "ub" else True


def count_nodes(e):
    return 1 + sum(count_nodes(k) for k in e[2:]) if e[0] in "ub" else 1


# ------------------------------------------------------------------------------------------------- the live-value rule
def plan(body):
    """The header's documented rule restated: {live, folded, ins: [(kind, op, DX, DY, srcA, srcB)]}.
    live(leaf) = 1, live(u(x)) = live(x), live(b(leaf, leaf)) = 1, live(b(x, leaf)) = live(x),
    live(b(x, y)) = max(hi, lo + 1); the child needing more live values runs first (SW when that is the right
    one); a subtree without p, t, w is one constant leaf."""
    e = parse(body) if isinstance(body, str) else body

    def const(e):
        return e[0] == "c" or (e[0] in "ub" and all(const(k) for k in e[2:]))

    def leaf(e):
        return e[0] in "ptw" or const(e)

    def dep(e):
        return e[0] == "p" or (e[0] in "ub" and any(dep(k) for k in e[2:]))

    def src(e):
        return "c" if const(e) else e[0]

    def live(e):
        if leaf(e):
            return 1
        if e[0] == "u":
            return live(e[2])
        a, b = e[2], e[3]
        if leaf(a) and leaf(b):
            return 1
        if leaf(b):
            return live(a)
        if leaf(a):
            return live(b)
        hi, lo = max(live(a), live(b)), min(live(a), live(b))
        return max(hi, lo + 1)

    ins, folded = [], [0]

    def emit(e, pushed=True):
        if leaf(e):
            folded[0] += int(e[0] != "c" and const(e))
            if pushed:
                ins.append(("PUSH", None, 0, 0, src(e), None))
            return
        if e[0] == "u":
            emit(e[2])
            ins.append(("UNARY", e[1], int(dep(e[2])), 0, None, None))
            return
        _, op, a, b = e
        dx, dy = int(dep(a)), int(dep(b))
        if leaf(a) and leaf(b):
            emit(a, False), emit(b, False)
            ins.append(("LL", op, dx, dy, src(a), src(b)))
        elif leaf(b):
            emit(a), emit(b, False)
            ins.append(("SL", op, dx, dy, src(b), None))
        elif leaf(a):
            emit(b), emit(a, False)
            ins.append(("LS", op, dx, dy, src(a), None))
        elif live(a) >= live(b):
            emit(a), emit(b)
            ins.append(("SS", op, dx, dy, None, None))
        else:
            emit(b), emit(a)
            ins.append(("SW", op, dx, dy, None, None))

    emit(e)
    return dict(live=live(e), folded=folded[0], ins=ins)


# ------------------------------------------------------------------------------------------------- points and bodies
def points():
    """32 points (p, t, w): p an odd multiple of 1/8 in (-4, 4), t = (4 j + 2) / 8 in (-4, 4) — so p, p +- t and t
    are at least 1/8 from 0 and from every multiple of 1/4 — and w in {0.5, 1, 2, 4}."""
    out = []
    for k in range(32):
        p = Fraction(2 * ((7 * k + 3) % 32) - 31, 8)
        t = Fraction(4 * ((5 * k + 1) % 16) - 30, 8)
        out.append((p, t, (Fraction(1, 2), Fraction(1), Fraction(2), Fraction(4))[(k + k // 4) % 4]))
    return out


def arrays(pts, dtype):
    return tuple(np.array([float(x[i]) for x in pts], dtype=dtype) for i in range(3))


def _minus_tree(levels, leaves):
    """A perfect tree of `-` over the next 2^levels leaf-operand nodes: levels + 1 live values."""
    if levels == 0:
        return leaves.pop(0)
    a = _minus_tree(levels - 1, leaves)
    return f"({a} - {_minus_tree(levels - 1, leaves)})"


_LL = ["(p - t)", "(p * 0.5)", "(t * 0.25)", "(p + 1.5)", "(p * 1.5)", "(t + 0.5)", "(p * 2.0)", "(t * 0.75)",
       "(t - p)", "(p * 0.25)", "(t * 1.5)", "(p - 0.75)", "(0.5 - p)", "(t * 0.5)", "(p + t)", "(1.25 - t)"]


def _live(n, at=0):
    return _minus_tree(n - 1, list(_LL[at:]))


def chain31():
    """test_loss_expr_host.py's test_limits chain: 31 nodes, one live value."""
    chain = "p"
    for i in range(15):
        chain = f"{'t' if i % 2 else 'p'} + ({chain})"
    return chain


FIXED = [
    # one instruction of each leaf form, with - and with /
    "p", "t", "p - t", "t - p", "p / 4.0", "p / w", "p - p", "p * p", "t - w", "w - 0.5", "0.25 - w", "w / 2.0",
    "abs(p)", "abs(t)", "neg(p - t)", "square(p - t)", "relu(p - t)", "relu(t - p)",
    "abs(p) - t", "abs(p) - w", "abs(p) - 0.25", "abs(t) - p", "abs(p) / w", "abs(p) / 0.5", "abs(t) / w",
    "t - abs(p)", "w - abs(p)", "0.75 - abs(p)", "p - abs(t)", "p / (w * 2.0)", "t / (w * 0.5)", "1.5 - abs(t)",
    # two stack operands: SS (left first) and SW (right first, operands swapped), - and /, every DX / DY
    "abs(p) - abs(t)", "abs(t) - abs(p)", "abs(p) - abs(p - t)", "abs(t) - abs(w)",
    "abs(p) / (w * 2.0)", "abs(t) / (w * 2.0)", "abs(p - t) / (w * 4.0)",
    "abs(p) - (abs(p - t) * abs(p + t))", "abs(t) - (abs(p - t) * abs(p + t))", "abs(p) - (abs(t) * abs(t - w))",
    "abs(t) - (abs(t) - abs(t - w))", "abs(p) / ((w * 2.0) * (w * 0.5))", "abs(t) / ((w * 2.0) * (w * 0.5))",
    "abs(p - t) / ((w * 2.0) * (w * 4.0))", "(p - t) - (abs(p) - abs(t))",
    # exactly 1, 2, 3 and 4 live values, - at every level; SW under and over deeper trees
    _live(1), _live(2), _live(3), _live(4), f"{_live(3, 8)} - {_live(4)}", f"{_live(2, 8)} - {_live(3)}",
    f"abs(p) - {_live(4)}", f"{_live(4)} - {_live(3, 8)}", f"abs(t) - {_live(4, 8)}",
    # the other exact operators, and comparisons as factors
    "max(p, t)", "min(p, t)", "max(t, p) - min(p, 0.5)", "max(abs(p), abs(t))", "min(abs(p - t), w)",
    "(p - t) * ((p > t) - 0.25)", "(p - t) * ((p < t) - 0.25)", "(p >= t) - (p <= t)", "cond(p - t, p)",
    "cond(t - p, square(p))", "cond(t, p - 0.5)", "(abs(p) > abs(t)) * (p - t)", "square(max(0.0, 1.0 - p * 0.5))",
    "square(abs(p) - abs(t))", "square(p) - square(t)", "relu(abs(p) - abs(t)) * 0.5", "neg(abs(p)) * (t - w)",
    # a folded constant subtree; the 31-node chain
    "(0.5 + 0.25) * p", "p - (0.5 * (1.5 - 0.25))", "abs(p - t) * (neg(0.25) - 1.0)", chain31(),
]


def admissible(body, pts):
    """The constraints on a table body: constants multiples of 1/4, at most three multiplications on a path, degree
    in p at most 2, divisors powers of two, inside the compiler's limits, and exact with room at every point."""
    e = parse(body)
    pl = plan(e)
    if not (constants_ok(e) and divisors_ok(e) and mul_depth(e) <= 3 and count_nodes(e) <= 127 and pl["live"] <= 4
            and len(pl["ins"]) <= 60):
        return False
    try:
        if degree(e) > 2:
            return False
        reference(body, pts)
    except (AssertionError, ZeroDivisionError):
        return False
    return True


@functools.lru_cache(maxsize=None)
def random_bodies(n=60, seed=20261020):
    """`n` seeded random bodies under FIXED's constraints (redrawn until `n` satisfy them at every point)."""
    rng = np.random.default_rng(seed)
    pts = points()
    consts = [c / 4 for c in range(-8, 9) if c != 0]

    def leaf(weighted):
        r = rng.random()
        if r < 0.45:
            return "p"
        if r < 0.7:
            return "t"
        if weighted and r < 0.8:
            return "w"
        return repr(float(consts[rng.integers(len(consts))]))

    def gen(budget, weighted):
        if budget <= 1 or rng.random() < 0.06:
            return leaf(weighted)
        r = rng.random()
        if r < 0.2:
            return f"{EXACT_UNARY[rng.integers(4)]}({gen(budget - 1, weighted)})"
        op = EXACT_BINARY[rng.integers(len(EXACT_BINARY))]
        if op == "/":
            d = "w" if weighted and rng.random() < 0.5 else ("2.0", "4.0", "0.5", "(w * 2.0)" if weighted else "0.25")[rng.integers(4)]
            return f"({gen(budget - 1, weighted)} / {d})"
        left = int(rng.integers(1, budget - 1)) if budget > 2 else 1
        a, b = gen(left, weighted), gen(budget - 1 - left, weighted)
        return f"({a} {op} {b})" if op in INFIX else f"{op}({a}, {b})"

    out = []
    while len(out) < n:
        weighted = bool(rng.integers(2))
        body = gen(int(rng.integers(4, 30)), weighted)
        e = parse(body)
        if plan(e)["ins"][-1][2:4] == (0, 0) or body in out or body in FIXED:  # (the root must depend on p)
            continue
        if admissible(body, pts):
            out.append(body)
    return tuple(out)


def table():
    return list(FIXED) + list(random_bodies())


# ------------------------------------------------------------------------------------------------- the device harness
TIERS = ("BASIC", "FULL")


def tier_operators(tier, gradient=False):
    """The search's operator set decides the tile build: loss_expr_util.OPS runs the BASIC builds, the whole catalog
    (op_values_util.options()'s lists) the FULL ones.  gamma has no derivative rule and an operator set that holds
    it is refused by the gradient calls (the gradient kernels have no tiers): those calls leave it out."""
    if tier == "BASIC":
        return dict(loss_expr_util.OPS)
    un = [u for u in op_values_util.UNARY if not (gradient and u == "gamma")]
    return dict(binary_operators=list(op_values_util.BINARY), unary_operators=un)


def _options(body, tier, gradient=False):
    return Options(elementwise_loss=spec(body), **tier_operators(tier, gradient))


def _dataset(body, p, t, w):
    weighted = uses_w(parse(body))
    X = np.ascontiguousarray(np.asarray(p)[None, :])
    with np.errstate(over="ignore"):  # (operands near floatmax: the dataset's own statistics may overflow)
        return Dataset(X, np.ascontiguousarray(t), **(dict(weights=np.ascontiguousarray(w)) if weighted else {})), weighted


def one_row_losses(opts, ds, n, dtype):
    """(loss [n], complete [n]): tree k = x1 on the one-row view [k] of `ds` (also loss_values_util.py's harness)."""
    tb = flatten_trees([Node(feature=1) for _ in range(n)], dtype)  # x1 keeps -0.0
    return eval_loss_batch_views(tb, ds, opts, np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int64)[:, None])


def one_row_gradients(opts, ds, n, dtype):
    """(gradient [n], complete [n]): tree k = x1 + 0.0 on the one-row view [k]; its single entry is dL/dp."""
    tb = flatten_trees([parse_expression("x1 + 0.0", opts) for _ in range(n)], dtype)
    _, g, gc = eval_grad_batch_views(tb, ds, opts, np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int64)[:, None])
    assert g.shape == (n,), g.shape
    return g, gc


def _one_row_values(body, ds, n, dtype, tier):
    return one_row_losses(_options(body, tier), ds, n, dtype)


def device_elements(body, p, t, w, dtype, tier, deriv=True):
    """(L [n], dL/dp [n] or None, complete [n]) of the device per point k: row k of the dataset is point k (X[0] = p,
    y = t, weights w when the body names it), tree k runs on the one-row view [k].  Values: the tree x1; a weighted
    call returns L_k / w_k, undone exactly (w_k a power of two); a zero's sign from ``1.0 / (BODY)`` (module
    docstring).  Derivatives: the tree x1 + 0.0, whose single gradient entry is dL/dp (divided by w_k)."""
    p, t, w = (np.ascontiguousarray(a, dtype=dtype) for a in (p, t, w))
    n = len(p)
    ds, weighted = _dataset(body, p, t, w)
    try:
        loss, comp = _one_row_values(body, ds, n, dtype, tier)
        scale = w if weighted else dtype(1)
        with np.errstate(all="ignore"):
            val = (loss * scale).astype(dtype)
        zero = np.nonzero(comp & (val == 0))[0]
        if len(zero):
            inv, _ = _one_row_values(f"1.0 / ({body})", ds, n, dtype, tier)
            assert np.all(np.isinf(inv[zero])), (body, "1 / 0 must be +-Inf", inv[zero])
            val[zero] = np.where(inv[zero] < 0, dtype(-0.0), dtype(0.0))
        der = None
        if deriv:
            g, gc = one_row_gradients(_options(body, tier, gradient=True), ds, n, dtype)
            assert np.array_equal(gc, comp), (body, gc, comp)
            with np.errstate(all="ignore"):
                der = (g * scale).astype(dtype)
    finally:
        ds.free_device()
    return val, der, comp


def full_rows(n_points, n_rows=N_FULL):
    """Point of each row of the full-view dataset: the point list tiled, rotated by one per repetition, so every
    row slot of a lane holds distinct values."""
    r = np.arange(n_rows)
    return (r + r // n_points) % n_points


def device_mean(body, p, t, w, dtype, tier, deriv=True):
    """(loss, gradient entry or None, rows-per-lane of the loss call) of the same points as ONE plain dataset of
    N_FULL rows (eval_loss_batch / eval_grad_batch: the non-gathered builds); rows as full_rows."""
    idx = full_rows(len(p))
    p, t, w = (np.ascontiguousarray(np.asarray(a, dtype=dtype)[idx]) for a in (p, t, w))
    ds, _ = _dataset(body, p, t, w)
    try:
        loss, comp = eval_loss_batch(flatten_trees([Node(feature=1)], dtype), ds, _options(body, tier))
        rows = get_context().last_rows_per_lane()
        assert comp.all()
        g = None
        if deriv:
            opts = _options(body, tier, gradient=True)
            _, g, gc = eval_grad_batch(flatten_trees([parse_expression("x1 + 0.0", opts)], dtype), ds, opts)
            assert gc.all() and g.shape == (1,)
            g = g[0]
    finally:
        ds.free_device()
    return loss[0], g, rows


def mean_tolerances(val, der, w, weighted, dtype):
    """What device_mean must meet, from the per-element device values `val`, `der` (Float64 arrays) alone.
    Loss: the f64 sum of the T values divided once and rounded to T — 1 ulp of T at the mean plus the f64 sum's own
    n 2^-53 Σ|L_k| / n (a tile's own 64 R values are first summed in T: exact for the table's dyadic values, so the
    bound has no term for it).  Gradient: K_T eps_T Σ|d_k| / n, test_gpu_grad_rules.py's K_T (the gradient kernel sums
    row terms in T).  Returns (mean, loss tolerance, gradient mean, gradient tolerance)."""
    from test_gpu_grad_rules import K_T

    name = "float32" if dtype == np.float32 else "float64"
    denom = float(np.sum(w.astype(np.float64))) if weighted else float(len(val))
    mean = float(np.sum(val)) / denom
    ulp = float(np.spacing(np.abs(dtype(mean))))
    tol_l = ulp + len(val) * 2.0 ** -53 * float(np.sum(np.abs(val))) / denom
    gmean = float(np.sum(der)) / denom
    tol_g = K_T[name] * float(np.finfo(dtype).eps) * float(np.sum(np.abs(der))) / denom
    return mean, tol_l, gmean, tol_g


def host_elements(body, p, t, w, dtype):
    """(L, dL/dp) of the library's host interpreter at the points."""
    ex = LossExpression(spec(body))
    args = [np.asarray(a, dtype=dtype) for a in ((p, t, w) if ex.n_args == 3 else (p, t))]
    return ex.host_eval(*args, deriv=True)
