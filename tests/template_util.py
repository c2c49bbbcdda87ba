"""Helpers of the TemplateExpression tests: fixture loading, random templates, and an independent
stage-by-stage restatement of the reference's evaluation (``ValidVector`` semantics,
src/ComposableExpression.jl:198-289) that never composes a tree.

The restatement parses the structure's text itself and walks it: every call ``f(a1..am)`` evaluates ALL its arguments, stacks them and
runs the CPU oracle's ``eval_tree_array`` on ``f``'s own tree; every structure operation is applied to its
operand arrays on its own (the oracle on the two-leaf tree ``op(x1, x2)``, i.e. the operator broadcast and
``is_valid_array`` of the result); evaluation stops at the first invalid stage.  A number (a literal, ``p[1]``,
the value of an argument-less call) is valid whatever it holds and is broadcast when it meets a vector.
"""
import ast
import json
import os

import numpy as np

import sr_amd
from oracle import Oracle
from sr_amd import Node, Options, TemplateExpression, TemplateStructure, flatten_trees, parse_expression
from sr_amd.operators import BINARY_ALIASES, UNARY_ALIASES

HERE = os.path.dirname(os.path.abspath(__file__))


def load_cases():
    with open(os.path.join(HERE, "golden", "template_known_answers.json")) as f:
        return json.load(f)["cases"]


def build_case(c):
    """(options, template, X, y, rows) of a fixture case."""
    opts = Options(binary_operators=c["binary_operators"], unary_operators=c["unary_operators"])
    st = TemplateStructure(tuple(c["expressions"]), c["combine"], arguments=c["arguments"], parameters=c["parameters"])
    trees = {k: parse_expression(v, opts) for k, v in c["trees"].items()}
    ex = TemplateExpression(trees, structure=st, parameters=c["parameter_values"])
    dtype = np.dtype(c["dtype"])
    X = np.asarray(c["X"], dtype=dtype)
    y = None if c["y"] is None else np.asarray(c["y"], dtype=dtype)
    return opts, ex, X, y, c["rows"]


class Invalid(Exception):
    pass


_SYMBOL = {ast.Add: "+", ast.Sub: "-", ast.Mult: "*", ast.Div: "/"}
_ORACLES = {}


def _oracle(unary, binary):
    key = (tuple(unary), tuple(binary))
    if key not in _ORACLES:
        _ORACLES[key] = Oracle(*key)
    return _ORACLES[key]


def staged_eval(ex, X, options, skip_dropped=False):
    """(values or None, complete): the restatement.  It reads only the template's inputs — the structure's TEXT
    (parsed here with ``ast``, not the package's parse), its argument names, the sub-expression trees and the
    parameter values — and ``options`` (the sub-expressions' operators).  A structure operation runs on an
    oracle of that one operator.  With ``skip_dropped`` an argument its callee does not reference is not
    evaluated (what composition alone sees)."""
    X = np.asarray(X)
    dtype, n = X.dtype, X.shape[1]
    st = ex.structure
    keys = set(st.expressions)
    body = ast.parse(st.combine.replace("^", "**"), mode="eval").body
    sub_oracle = _oracle(options.operators.unaops, options.operators.binops)
    # a sub-expression holding a feature above the number of arguments it is called with: incomplete
    arity = {c.func.id: len(c.args) for c in ast.walk(body)
             if isinstance(c, ast.Call) and isinstance(c.func, ast.Name) and c.func.id in keys}
    for k, tree in ex.trees.items():
        if any(x.degree == 0 and not x.constant and x.feature > arity[k] for x in tree.preorder()):
            return None, False

    def as_array(v):
        return v if isinstance(v, np.ndarray) else np.full(n, v, dtype=dtype)

    def run(oracle, tree, cols):
        tb = flatten_trees([tree], dtype)
        return oracle.eval_tree_array(tb, 0, np.stack(cols) if cols else np.zeros((1, 1), dtype=dtype))

    def apply(name, vals):
        """One structure operation on its operand arrays, checked on its own."""
        assert any(isinstance(v, np.ndarray) for v in vals), "the generator makes no number-only operations"
        cols = [as_array(v) for v in vals]
        if len(cols) == 1:
            out, ok = run(_oracle((UNARY_ALIASES[name],), ()), Node(op=1, l=Node(feature=1)), cols)
        else:
            out, ok = run(_oracle((), (BINARY_ALIASES[name],)), Node(op=1, l=Node(feature=1), r=Node(feature=2)), cols)
        if not ok:
            raise Invalid
        return out

    def feature(name):
        if st.arguments is not None:
            return list(st.arguments).index(name) + 1
        assert name[0] == "x"
        return int(name[1:])

    def ev(e):
        if isinstance(e, ast.Constant):
            return dtype.type(e.value)
        if isinstance(e, ast.Name):
            return X[feature(e.id) - 1]
        if isinstance(e, ast.UnaryOp):
            if isinstance(e.operand, ast.Constant):
                return dtype.type(-e.operand.value)
            return apply("neg", [ev(e.operand)])
        if isinstance(e, ast.Subscript):
            return dtype.type(ex.parameters[e.value.id][e.slice.value - 1])
        if isinstance(e, ast.BinOp) and isinstance(e.op, ast.Pow):
            if isinstance(e.right, ast.Constant) and isinstance(e.right.value, int):  # Base.literal_pow: x ONCE
                x = ev(e.left)
                out = x
                for _ in range(e.right.value - 1):
                    out = apply("*", [out, x])
                return out
            return apply("^", [ev(e.left), ev(e.right)])
        if isinstance(e, ast.BinOp):
            return apply(_SYMBOL[type(e.op)], [ev(e.left), ev(e.right)])
        assert isinstance(e, ast.Call)
        if e.func.id not in keys:
            return apply(e.func.id, [ev(a) for a in e.args])
        tree = ex.trees[e.func.id]
        vals = []
        for i, a in enumerate(e.args, start=1):
            used = any(x.degree == 0 and not x.constant and x.feature == i for x in tree.preorder())
            vals.append(None if (skip_dropped and not used) else ev(a))
        if not e.args:  # an argument-less call is a number: NaN when its evaluation is incomplete
            out, ok = run(sub_oracle, tree, [])
            return out[0] if ok else dtype.type(np.nan)
        out, ok = run(sub_oracle, tree, [as_array(dtype.type(0) if v is None else v) for v in vals])
        if not ok:
            raise Invalid
        return out

    try:
        out = ev(body)
    except Invalid:
        return None, False
    return as_array(out), True


# ---------------------------------------------------------------------- random templates
SUB_OPS = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
STRUCT_UNARY = ("sin", "log", "sqrt", "exp")
STRUCT_BINARY = ("+", "-", "*", "/", "max")


def random_template(rng, options, dtype, nfeat=3):
    """A random structure over K = 1..3 sub-expressions of arity 0..3 (every key called at least once, every
    call with its first argument a vector) and random sub-trees of 1..9 nodes."""
    keys = ("f", "g", "h")[:int(rng.integers(1, 4))]
    arity = {k: int(rng.integers(0, 4)) for k in keys}
    if all(a == 0 for a in arity.values()):
        arity[keys[0]] = int(rng.integers(1, 4))
    pending = list(keys)
    rng.shuffle(pending)

    def data():
        return f"x{int(rng.integers(1, nfeat + 1))}"

    def call(key, depth):
        if arity[key] == 0:
            return f"{key}()"
        args = [vector(depth + 1)] + [argument(depth + 1) for _ in range(arity[key] - 1)]
        return f"{key}({', '.join(args)})"

    def any_call(depth, vector_only):
        if pending:
            cand = [k for k in pending if arity[k] > 0 or not vector_only]
            if cand:
                pending.remove(cand[0])
                return call(cand[0], depth)
        cand = [k for k in keys if arity[k] > 0 or not vector_only]
        return call(cand[int(rng.integers(0, len(cand)))], depth)

    def vector(depth):
        r = rng.random()
        if depth >= 3 or r < 0.45:
            return data()
        if r < 0.60:
            return f"{STRUCT_UNARY[int(rng.integers(0, len(STRUCT_UNARY)))]}({vector(depth + 1)})"
        if r < 0.75:
            op = STRUCT_BINARY[int(rng.integers(0, len(STRUCT_BINARY)))]
            a, b = vector(depth + 1), vector(depth + 1)
            return f"max({a}, {b})" if op == "max" else f"({a} {op} {b})"
        if r < 0.80:
            return f"({vector(depth + 1)})^{int(rng.integers(2, 4))}"
        return any_call(depth, True)

    def argument(depth):
        r = rng.random()
        if r < 0.08:
            return repr(round(float(rng.standard_normal()), 3))
        if r < 0.16:
            return any_call(depth, False)
        return vector(depth)

    def term():
        return any_call(0, True) if rng.random() < 0.7 else vector(1)

    text = term()
    while pending or rng.random() < 0.3:
        if pending and arity[pending[0]] == 0:  # an argument-less call: a number beside a vector
            text = f"({text} + {call(pending.pop(0), 0)})"
            continue
        op = STRUCT_BINARY[int(rng.integers(0, len(STRUCT_BINARY)))]
        t = term()
        text = f"max({text}, {t})" if op == "max" else f"({text} {op} {t})"
    st = TemplateStructure(keys, text)
    trees = {}
    for k in keys:
        size = int(rng.integers(1, 10))
        t = sr_amd.gen_random_tree_fixed_size(size, options, max(1, arity[k]), dtype, rng)
        if arity[k] == 0:
            for nd in t.preorder():
                if nd.degree == 0 and not nd.constant:
                    nd.set_node(Node(val=dtype(rng.standard_normal())))
        trees[k] = t
    return TemplateExpression(trees, structure=st)
