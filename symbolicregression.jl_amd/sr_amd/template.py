"""``TemplateExpression`` candidates (reference src/TemplateExpression.jl, src/ComposableExpression.jl).

A template is a fixed structure around K sub-expressions: ``TemplateStructure(("f", "g"),
"sin(f(x1, x2)) + g(x3)^2")`` is the body of the reference's ``@template_spec ... do`` block given as text
(closures cannot cross the C ABI).  ``compose`` turns a candidate into ONE tree, the way the reference's
``DE.get_tree(::TemplateExpression)`` does, and the existing device paths evaluate it; what composition
loses is carried beside the tree:

* a sub-expression called several times puts its constants into the composed tree several times: the
  copies are one scalar (``slots``: the index into ``get_scalar_constants(ex)``);
* literals of the structure are frozen (slot -1): no tangent, never optimised;
* an argument the callee does not use vanishes from the composed tree, and with it any NaN it produced:
  it is kept as a *guard* tree, scored in the same device call, and the candidate is complete only if its
  main tree and all its guards are.
"""
from __future__ import annotations

import ast
import copy as _copy
import ctypes
import re
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from . import node as _node
from .node import Node, ParametricExpression, flatten_trees
from .operators import BINARY_ALIASES, UNARY_ALIASES, OperatorEnum

SECTION = "DESIGN.md §16"
_BINOPS = {ast.Add: "+", ast.Sub: "-", ast.Mult: "*", ast.Div: "/"}


class TemplateStructure:
    """``TemplateStructure(expressions, combine, arguments=None, parameters=None, num_features=None)``.

    ``combine`` is parsed with ``ast``: infix ``+ - * / ^``, unary minus (``neg``), calls of the
    sub-expressions, calls of any operator of the device catalog by name (not only ``options.operators``),
    data arguments (default ``x1..xn``; argument i is dataset feature i), numeric literals, and parameter
    vectors read as ``p[1]`` (a literal 1-based index) or ``p[category]`` with ``category`` a data argument.
    Integer literal powers follow ``Base.literal_pow`` (``^1``, ``^2`` = ``x * x``, ``^3`` = ``(x * x) * x``;
    other literal integers are refused).  ``D(f, i)`` is refused."""

    def __init__(self, expressions: Sequence[str], combine: str, arguments: Optional[Sequence[str]] = None,
                 parameters: Optional[Dict[str, int]] = None, num_features: Optional[Dict[str, int]] = None):
        self.expressions = tuple(expressions)
        if not self.expressions or len(set(self.expressions)) != len(self.expressions):
            raise ValueError("expressions must be a non-empty tuple of distinct names")
        self.combine = str(combine)
        self.arguments = None if arguments is None else tuple(arguments)
        self.parameters = dict(parameters or {})
        for name, n in self.parameters.items():
            if int(n) < 1:
                raise ValueError(f"parameter vector {name} needs a positive length")
        clash = set(self.expressions) & set(self.parameters)
        if clash:
            raise ValueError(f"names used both as expression and parameter: {sorted(clash)}")
        self._arity: Dict[str, int] = {}
        self.unary_ops: List[str] = []   # canonical names the structure itself uses, in order of appearance
        self.binary_ops: List[str] = []
        self._how: Dict[str, str] = {}   # parameter vector -> "literal" / "category"
        self.category: Optional[int] = None  # the feature (1-based) that indexes p[category]
        try:
            body = ast.parse(self.combine.replace("^", "**"), mode="eval").body
        except SyntaxError as e:
            raise ValueError(f"combine {self.combine!r}: cannot parse ({e.msg})") from None
        if any(isinstance(n, ast.Name) and n.id == "D" for n in ast.walk(body)) and "D" not in self.expressions:
            raise ValueError(f"combine: D(f, i) (derivatives of sub-expressions) is not supported ({SECTION})")
        self.ir = self._parse(body)
        missing = tuple(k for k in self.expressions if k not in self._arity)
        if num_features is not None:
            for k, n in dict(num_features).items():
                if k in self._arity and self._arity[k] != int(n):
                    raise ValueError(f"Inconsistent number of arguments passed to {k}")
                self._arity[k] = int(n)
            missing = tuple(k for k in self.expressions if k not in self._arity)
        if missing:
            raise ValueError(f"Failed to infer number of features used by {missing}")
        self.num_features = {k: self._arity[k] for k in self.expressions}
        # category-indexed vectors, in declared order: row k of the composed ParametricExpression's matrix
        self.category_vectors = tuple(n for n in self.parameters if self._how.get(n) == "category")

    # ------------------------------------------------------------------ parsing
    def _feature(self, name: str) -> Optional[int]:
        if self.arguments is not None:
            return self.arguments.index(name) + 1 if name in self.arguments else None
        m = re.fullmatch(r"x([1-9][0-9]*)", name)
        return int(m.group(1)) if m else None

    def _use_op(self, lst: List[str], name: str) -> str:
        if name not in lst:
            lst.append(name)
        return name

    def _parse(self, e):
        if isinstance(e, ast.Constant):
            if isinstance(e.value, bool) or not isinstance(e.value, (int, float)):
                raise ValueError(f"combine: unsupported literal {e.value!r}")
            return ("lit", float(e.value))
        if isinstance(e, ast.Name):
            if e.id in ("inf", "Inf"):
                return ("lit", float("inf"))
            if e.id in ("nan", "NaN"):
                return ("lit", float("nan"))
            f = self._feature(e.id)
            if f is None:
                raise ValueError(f"combine: unknown name {e.id!r}")
            return ("arg", f)
        if isinstance(e, ast.UnaryOp) and isinstance(e.op, ast.USub):
            if isinstance(e.operand, ast.Constant) and isinstance(e.operand.value, (int, float)):
                return ("lit", -float(e.operand.value))
            return ("op1", self._use_op(self.unary_ops, "neg"), self._parse(e.operand))
        if isinstance(e, ast.BinOp) and type(e.op) in _BINOPS:
            return ("op2", self._use_op(self.binary_ops, BINARY_ALIASES[_BINOPS[type(e.op)]]),
                    self._parse(e.left), self._parse(e.right))
        if isinstance(e, ast.BinOp) and isinstance(e.op, ast.Pow):
            r = e.right
            neg = isinstance(r, ast.UnaryOp) and isinstance(r.op, ast.USub) and isinstance(r.operand, ast.Constant)
            lit = r.operand.value if neg else (r.value if isinstance(r, ast.Constant) else None)
            if isinstance(lit, int) and not isinstance(lit, bool):  # Base.literal_pow
                p = -lit if neg else lit
                x = self._parse(e.left)
                if p == 1:
                    return x
                if p not in (2, 3):
                    raise ValueError(f"combine: the literal integer power ^{p} is not supported (only ^1, ^2, ^3; "
                                     "write a Float exponent for safe_pow)")
                mul = self._use_op(self.binary_ops, "*")
                sq = ("op2", mul, x, x)
                return sq if p == 2 else ("op2", mul, sq, x)
            return ("op2", self._use_op(self.binary_ops, "safe_pow"), self._parse(e.left), self._parse(r))
        if isinstance(e, ast.Subscript) and isinstance(e.value, ast.Name):
            name = e.value.id
            if name not in self.parameters:
                raise ValueError(f"combine: {name!r} is not a parameter vector")
            idx = e.slice
            if isinstance(idx, ast.Constant) and isinstance(idx.value, int) and not isinstance(idx.value, bool):
                if not 1 <= idx.value <= int(self.parameters[name]):
                    raise ValueError(f"combine: {name}[{idx.value}] is outside 1..{self.parameters[name]}")
                how, out = "literal", ("plit", name, idx.value - 1)
            elif isinstance(idx, ast.Name) and self._feature(idx.id) is not None:
                f = self._feature(idx.id)
                if self.category is not None and self.category != f:
                    raise ValueError(f"combine: several category columns are not supported ({SECTION})")
                self.category = f
                how, out = "category", ("pcat", name)
            else:
                raise ValueError(f"combine: {name}[...] takes a literal index or a data argument ({SECTION}: no "
                                 "iteration over a parameter vector)")
            if self._how.setdefault(name, how) != how:
                raise ValueError(f"combine: parameter vector {name} is indexed both by a literal and by a category")
            return out
        if isinstance(e, ast.Call) and isinstance(e.func, ast.Name) and not e.keywords:
            fname = e.func.id
            if fname == "D":
                raise ValueError(f"combine: D(f, i) (derivatives of sub-expressions) is not supported ({SECTION})")
            if fname in self.expressions:
                args = [self._parse(a) for a in e.args]
                if self._arity.setdefault(fname, len(args)) != len(args):
                    raise ValueError(f"Inconsistent number of arguments passed to {fname}")
                return ("call", fname, args)
            args = [self._parse(a) for a in e.args]
            if len(args) == 1 and fname in UNARY_ALIASES:
                return ("op1", self._use_op(self.unary_ops, UNARY_ALIASES[fname]), args[0])
            if len(args) == 2 and fname in BINARY_ALIASES:
                return ("op2", self._use_op(self.binary_ops, BINARY_ALIASES[fname]), args[0], args[1])
            raise ValueError(f"combine: {fname!r} with {len(args)} argument(s) is neither a sub-expression nor an "
                             "operator of the device catalog")
        raise ValueError(f"combine: cannot parse {ast.dump(e)}")

    def union_operators(self, operators: OperatorEnum) -> OperatorEnum:
        """``operators`` with the structure-only operators appended: sub-expression op indices stay valid."""
        un = list(operators.unaops) + [u for u in self.unary_ops if u not in operators.unaops]
        bi = list(operators.binops) + [b for b in self.binary_ops if b not in operators.binops]
        return OperatorEnum(un, bi)

    def key(self):
        return (self.expressions, self.combine, self.arguments, tuple(self.parameters.items()))

    def __repr__(self):
        return f"TemplateStructure({self.expressions!r}, {self.combine!r})"


class TemplateExpressionSpec:
    """``TemplateExpressionSpec(structure=...)``, accepted by ``Options(expression_spec=...)``."""

    def __init__(self, *, structure: TemplateStructure):
        if not isinstance(structure, TemplateStructure):
            raise ValueError("structure must be a TemplateStructure")
        self.structure = structure

    def __repr__(self):
        return f"TemplateExpressionSpec({self.structure!r})"


class TemplateExpression:
    """``TemplateExpression(trees, structure=..., parameters=None)``: one ``Node`` per key of the structure (its
    feature leaf ``#i`` is the call's i-th argument) and the parameter vectors (zeros when omitted)."""

    def __init__(self, trees: Dict[str, Node], *, structure: TemplateStructure, parameters: Optional[dict] = None):
        if set(trees) != set(structure.expressions):
            raise ValueError(f"trees must have exactly the keys {structure.expressions}")
        self.trees = {k: trees[k] for k in structure.expressions}
        self.structure = structure
        given = dict(parameters or {})
        if set(given) - set(structure.parameters):
            raise ValueError(f"unknown parameter vectors {sorted(set(given) - set(structure.parameters))}")
        self.parameters = {}
        for name, n in structure.parameters.items():
            v = np.zeros(int(n)) if name not in given else np.array(given[name], dtype=np.float64).reshape(-1)
            if name in given and v.size != int(n) and structure._how.get(name) != "category":
                raise ValueError(f"parameter vector {name} has {v.size} entries, the structure declares {n}")
            self.parameters[name] = v

    def copy(self) -> "TemplateExpression":
        return TemplateExpression({k: t.copy() for k, t in self.trees.items()}, structure=self.structure,
                                  parameters={k: v.copy() for k, v in self.parameters.items()})

    def has_invalid_variables(self) -> bool:
        """A sub-expression holding a feature above its arity (reference :942-958)."""
        for k, t in self.trees.items():
            n = self.structure.num_features[k]
            if any(x.degree == 0 and not x.constant and not x.is_parameter and x.feature > n for x in t.preorder()):
                return True
        return False

    def __repr__(self):
        return f"TemplateExpression({string_tree(self)})"


# ---------------------------------------------------------------------- accessors (reference behaviour)
def get_scalar_constants(ex):
    """A tree's constants in pre-order; for a template every sub-expression's, in key order, then every
    parameter vector in declared order."""
    if not isinstance(ex, TemplateExpression):
        return _node.get_scalar_constants(ex)
    parts = [_node.get_scalar_constants(t).astype(np.float64) for t in ex.trees.values()]
    parts += [np.asarray(v, dtype=np.float64) for v in ex.parameters.values()]
    return np.concatenate(parts) if parts else np.zeros(0)


def set_scalar_constants(ex, values) -> None:
    if not isinstance(ex, TemplateExpression):
        return _node.set_scalar_constants(ex, values)
    values = np.asarray(values)
    want = sum(t.count_constants() for t in ex.trees.values()) + sum(v.size for v in ex.parameters.values())
    if values.shape != (want,):
        raise ValueError(f"expected {want} scalars, got shape {values.shape}")
    at = 0
    for t in ex.trees.values():
        n = t.count_constants()
        _node.set_scalar_constants(t, [v.item() for v in values[at:at + n]])
        at += n
    for name, v in ex.parameters.items():
        ex.parameters[name] = np.array(values[at:at + v.size], dtype=np.float64)
        at += v.size
    if at != values.size:
        raise ValueError(f"expected {at} scalars, got {values.size}")


def string_tree(ex, operators=None) -> str:
    """``"f = #1 * #2; g = #1"`` for a template (a plain tree as before)."""
    ops = getattr(operators, "operators", operators)
    if not isinstance(ex, TemplateExpression):
        return _node.string_tree(ex, ops)

    def one(t):
        s = _node.string_tree(t, ops)
        s = re.sub(r"\bx([0-9]+)\b", r"#\1", s)
        return s[1:-1] if s.startswith("(") and s.endswith(")") and _balanced(s[1:-1]) else s

    return "; ".join(f"{k} = {one(t)}" for k, t in ex.trees.items())


def _balanced(s: str) -> bool:
    d = 0
    for c in s:
        d += c == "("
        d -= c == ")"
        if d < 0:
            return False
    return d == 0


def compute_complexity(ex, options=None) -> int:
    """The SUM of the sub-expressions' complexities (reference :552-561), not the composed tree's."""
    return sum(t.count_nodes() for t in ex.trees.values())


# ---------------------------------------------------------------------- composition
class ComposedTemplate:
    """``tree``: the composed Node; ``guards``: the composed trees of call arguments the callee drops;
    ``slots`` / ``guard_slots``: per constant node (pre-order) the index into ``get_scalar_constants(ex)``, -1
    for a structure literal; ``operators``: the union operator set; ``invalid``: a sub-expression holds a
    feature above its arity (no tree then); ``matrix``: ``[K, n_classes]`` rows of the category-indexed
    vectors in declared order (None for a parameter-free candidate)."""

    def __init__(self):
        self.tree = None
        self.guards: List[Node] = []
        self.slots: List[int] = []
        self.guard_slots: List[List[int]] = []
        self.operators = None
        self.invalid = False
        self.matrix = None
        self.n_scalars = 0
        self.category = None
        self.category_entries = {}  # vector name -> offset of its entries in get_scalar_constants order


def _uses_feature(tree: Node, i: int) -> bool:
    return any(n.degree == 0 and not n.constant and not n.is_parameter and n.feature == i for n in tree.preorder())


def compose(ex: TemplateExpression, options) -> ComposedTemplate:
    """The structure with every call ``f(a1..am)`` replaced by a copy of ``f``'s tree whose feature leaf ``#i``
    is a copy of the composed ``a_i`` (``DE.get_tree(::TemplateExpression)``), plus what that loses."""
    st = ex.structure
    base = getattr(options, "operators", options)
    out = ComposedTemplate()
    out.operators = ops = st.union_operators(base)
    out.category = st.category
    # where each sub-expression's constants and each parameter vector start in the scalar vector
    koff, at = {}, 0
    for k, t in ex.trees.items():
        koff[k] = at
        at += t.count_constants()
    poff = {}
    for name, v in ex.parameters.items():
        poff[name] = at
        at += v.size
    out.n_scalars = at
    out.category_entries = {n: poff[n] for n in st.category_vectors}
    if st.category_vectors:
        sizes = {n: ex.parameters[n].size for n in st.category_vectors}
        if len(set(sizes.values())) != 1:
            raise ValueError(f"category-indexed parameter vectors have {sizes} entries: each needs one per class")
        out.matrix = np.stack([np.asarray(ex.parameters[n], dtype=np.float64) for n in st.category_vectors])
    if ex.has_invalid_variables():
        out.invalid = True
        return out
    slot: Dict[int, int] = {}
    keep: List[Node] = []  # (every constant node made here stays alive while `slot` is keyed by id)

    def const(v, s):
        n = Node(val=v)
        slot[id(n)] = s
        keep.append(n)
        return n

    def cp(n: Node) -> Node:
        m = n.copy()
        for a, b in zip(n.preorder(), m.preorder()):
            if a.degree == 0 and a.constant:
                slot[id(b)] = slot[id(a)]
                keep.append(b)
        return m

    def build(ir) -> Node:
        kind = ir[0]
        if kind == "arg":
            return Node(feature=ir[1])
        if kind == "lit":
            return const(ir[1], -1)
        if kind == "plit":
            return const(float(ex.parameters[ir[1]][ir[2]]), poff[ir[1]] + ir[2])
        if kind == "pcat":
            return Node(parameter=st.category_vectors.index(ir[1]) + 1)
        if kind == "op1":
            return Node(op=ops.unary_index(ir[1]), l=build(ir[2]))
        if kind == "op2":
            l = build(ir[2])
            return Node(op=ops.binary_index(ir[1]), l=l, r=build(ir[3]))
        key, args = ir[1], ir[2]
        callee = ex.trees[key]
        made = [build(a) for a in args]
        for i, (a, m) in enumerate(zip(args, made), start=1):
            # (a number is valid whatever it holds — a literal, p[1], the value of an argument-less call: the
            #  reference broadcasts it into a ValidVector marked valid — and a data argument is finite)
            if a[0] in ("arg", "lit", "plit", "pcat") or (a[0] == "call" and not a[2]) or _uses_feature(callee, i):
                continue
            out.guards.append(cp(m))
        ci = [koff[key]]

        def inst(n: Node) -> Node:
            if n.degree == 0:
                if n.is_parameter:
                    raise ValueError(f"sub-expression {key} holds a parameter leaf: parameters belong to the structure")
                if n.constant:
                    c = const(n.val, ci[0])
                    ci[0] += 1
                    return c
                return cp(made[n.feature - 1])
            l = inst(n.l)
            r = inst(n.r) if n.degree == 2 else None
            return Node(op=n.op, l=l, r=r)

        return inst(callee)

    out.tree = build(st.ir)
    slots_of = lambda t: [slot[id(n)] for n in t.preorder() if n.degree == 0 and n.constant]  # noqa: E731
    out.slots = slots_of(out.tree)
    out.guard_slots = [slots_of(g) for g in out.guards]
    return out


def get_tree(ex: TemplateExpression, options) -> Node:
    """The composed ``Node``; raises for a structure with parameters, as the reference does."""
    if ex.structure.parameters:
        raise ValueError("get_tree: a TemplateExpression with parameters has no plain tree (the reference raises too)")
    c = compose(ex, options)
    if c.invalid:
        raise ValueError("get_tree: a sub-expression holds a feature above its arity")
    return c.tree


# ---------------------------------------------------------------------- the device calls
def is_template_batch(trees) -> bool:
    if isinstance(trees, TemplateExpression):
        return True
    if isinstance(trees, (list, tuple)) and trees:
        unwrap = [getattr(t, "tree", t) if not isinstance(t, TemplateExpression) else t for t in trees]
        n = sum(isinstance(t, TemplateExpression) for t in unwrap)
        if n and n != len(unwrap):
            raise ValueError("a batch must be all templates of one structure (or hold none)")
        return n > 0
    return False


def refuse(trees, what: str) -> None:
    """Raise for a TemplateExpression batch in a call that does not take one."""
    if is_template_batch(trees):
        raise NotImplementedError(f"{what} does not take TemplateExpression candidates ({SECTION})")


def _check_category(st: TemplateStructure, full) -> None:
    if not st.category_vectors:
        return
    if not full.n_classes:
        raise ValueError("a template with p[category] needs a dataset that carries classes (extra={'class': ...})")
    done = full.__dict__.setdefault("_template_category_ok", set())
    if st.category not in done:  # once per dataset
        if st.category > full.nfeatures or not np.array_equal(full.X[st.category - 1], full.classes.astype(full.dtype)):
            raise ValueError(f"feature row {st.category} of X (the category argument) does not equal the dataset's "
                             "class ids (1-based)")
        done.add(st.category)


class _Plan:
    """A template batch composed for one device call: the valid candidates' main trees, then their guards."""

    def __init__(self, templates, dataset, options):
        templates = [templates] if isinstance(templates, TemplateExpression) else [
            t if isinstance(t, TemplateExpression) else t.tree for t in templates]
        self.templates = templates
        st = templates[0].structure
        if any(t.structure is not st and t.structure.key() != st.key() for t in templates):
            raise ValueError("a batch must be all templates of one structure")
        self.structure = st
        full = dataset.full
        _check_category(st, full)
        self.composed = [compose(t, options) for t in templates]
        self.options = _copy.copy(options)
        self.options.operators = st.union_operators(options.operators)
        self.options.expression_spec = None
        self.parametric = bool(st.category_vectors)
        if self.parametric:
            if getattr(options, "loss_expression", None) is not None:
                raise NotImplementedError("expression losses take parameter-free templates only (DESIGN.md §14, §16)")
            for c in self.composed:
                if c.matrix.shape[1] != full.n_classes:
                    raise ValueError(f"a category-indexed parameter vector has {c.matrix.shape[1]} entries, the dataset "
                                     f"{full.n_classes} classes")
        self.valid = [i for i, c in enumerate(self.composed) if not c.invalid]
        wrap = (lambda t, c: ParametricExpression(t, c.matrix)) if self.parametric else (lambda t, c: t)
        c0 = self.composed[0]
        self._ranges = sorted((off, off + templates[0].parameters[n].size) for n, off in c0.category_entries.items())
        items, self.owner, slots, nsc = [], [], [], []
        for i in self.valid:
            c = self.composed[i]
            items.append(wrap(c.tree, c))
            self.owner.append(-1)
            slots.extend(c.slots)
            nsc.append(c.n_scalars - self._n_cat(c))
        for j, i in enumerate(self.valid):
            c = self.composed[i]
            for g, gs in zip(c.guards, c.guard_slots):
                items.append(wrap(g, c))
                self.owner.append(j)
                slots.extend([-1] * len(gs))  # (a guard only has to be finite: nothing of it is differentiated)
                nsc.append(0)
        self.n_main = len(self.valid)
        self.batch = flatten_trees(items, full.dtype) if items else None
        # device scalar slots: the category-indexed vectors' entries are not constants of the composed tree but
        # rows of its parameter matrix, so the scalars in front of them keep their index and those behind move up
        self.slot = np.asarray([self._dev_slot(s) for s in slots], dtype=np.int32)
        self.n_scalars = np.asarray(nsc, dtype=np.int32)

    def _n_cat(self, c) -> int:
        return sum(self.templates[0].parameters[n].size for n in self.structure.category_vectors) if c.matrix is not None else 0

    def _cat_ranges(self):
        return self._ranges

    def _dev_slot(self, s: int) -> int:
        if s < 0:
            return -1
        return s - sum(hi - lo for lo, hi in self._cat_ranges() if hi <= s)

    def ties(self):
        t = _lib.SrScalarTies()
        self._slot_keep = np.ascontiguousarray(self.slot if self.slot.size else np.zeros(1, np.int32))
        self._nsc_keep = np.ascontiguousarray(self.n_scalars if self.n_scalars.size else np.zeros(1, np.int32))
        t.slot = self._slot_keep.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        t.n_scalars = self._nsc_keep.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        return t

    def fold_flags(self, comp) -> np.ndarray:
        """Per template: its main tree and all its guards complete; an invalid candidate is incomplete."""
        ok = np.array(comp[:self.n_main], dtype=bool)
        for pos, j in enumerate(self.owner):
            if j >= 0 and not comp[pos]:
                ok[j] = False
        out = np.zeros(len(self.templates), dtype=bool)
        out[self.valid] = ok
        return out

    def to_template_order(self, dev_vec, c, n_classes) -> np.ndarray:
        """A device vector ``[scalars | K x C column-major]`` of one candidate -> ``get_scalar_constants`` order."""
        out = np.zeros(c.n_scalars, dtype=dev_vec.dtype)
        ranges = self._cat_ranges()
        keep = np.ones(c.n_scalars, dtype=bool)
        for lo, hi in ranges:
            keep[lo:hi] = False
        ns = int(keep.sum())
        out[keep] = dev_vec[:ns]
        K = len(self.structure.category_vectors)
        for k, name in enumerate(self.structure.category_vectors):
            lo = c.category_entries[name]
            out[lo:lo + n_classes] = dev_vec[ns + k + K * np.arange(n_classes)]
        return out


def eval_loss_batch(templates, dataset, options, *, ctx=None):
    from . import loss as _loss

    plan = _Plan(templates, dataset, options)
    nt = len(plan.templates)
    losses = np.full(nt, np.inf, dtype=dataset.full.dtype)
    if plan.batch is None:
        return losses, np.zeros(nt, dtype=bool)
    l, comp = _loss.eval_loss_batch(plan.batch, dataset, plan.options, ctx=ctx)
    ok = plan.fold_flags(comp)
    losses[plan.valid] = l[:plan.n_main]
    losses[~ok] = np.inf
    return losses, ok


def eval_tree_array_batch(templates, dataset, options, *, ctx=None):
    from . import loss as _loss

    plan = _Plan(templates, dataset, options)
    full, idx = dataset.full, dataset.indices
    n_rows = full.n if idx is None else int(idx.size)
    out = np.zeros((len(plan.templates), n_rows), dtype=full.dtype)
    if plan.batch is None:
        return out, np.zeros(len(plan.templates), dtype=bool)
    o, comp = _loss.eval_tree_array_batch(plan.batch, dataset, plan.options, ctx=ctx)
    out[plan.valid] = o[:plan.n_main]
    return out, plan.fold_flags(comp)


def eval_grad_batch(templates, dataset, options, *, ctx=None):
    """``(losses, grads, complete)``: ``grads`` holds every template's gradient in ``get_scalar_constants``
    order, concatenated (zero for an incomplete candidate)."""
    from . import loss as _loss
    from .device import get_context

    if options.loss_function is not None or options.loss_function_expression is not None:
        raise NotImplementedError("custom objectives are evaluated by the reference CPU path")
    plan = _Plan(templates, dataset, options)
    nt = len(plan.templates)
    full, idx = dataset.full, dataset.indices
    losses = np.full(nt, np.inf, dtype=full.dtype)
    grads = [np.zeros(c.n_scalars, dtype=full.dtype) for c in plan.composed]
    if plan.batch is None:
        return losses, np.concatenate(grads), np.zeros(nt, dtype=bool)
    if full.y is None:
        raise ValueError("dataset has no y")
    ctx = ctx or get_context()
    tb = plan.batch
    K, C = (int(tb.parameters.shape[1]), int(tb.parameters.shape[2])) if tb.parametric else (0, 0)
    offs = np.concatenate([[0], np.cumsum(plan.n_scalars.astype(np.int64) + K * C)])
    l = np.empty(tb.n_trees, dtype=full.dtype)
    comp = np.empty(tb.n_trees, dtype=np.uint8)
    g = np.zeros(int(offs[-1]) + 1, dtype=full.dtype)
    s, ties = tb.to_struct(), plan.ties()
    ps = _loss._param_struct(tb, full, plan.options) if tb.parametric else None
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    _lib.check(_lib.lib.sr_eval_grad_batch_tied(
        ctx.handle, full.device_handle(ctx), ctx.opset_id(plan.options.operators), ctypes.byref(s),
        None if ps is None else ctypes.byref(ps), ctypes.byref(ties), None if idx is None else p(idx),
        0 if idx is None else int(idx.size), ctx.loss_code(plan.options), p(l), p(g), p(comp)))
    ok = plan.fold_flags(comp.astype(bool))
    for j, i in enumerate(plan.valid):
        if ok[i]:
            losses[i] = l[j]
            grads[i] = plan.to_template_order(g[offs[j]:offs[j + 1]], plan.composed[i], C)
    return losses, np.concatenate(grads), ok


def optimize_constants_batch(templates, dataset, options, rng=None, *, iterations=None, nrestarts=None, ctx=None,
                             f_calls_limit=None):
    """``(new_templates, losses, improved, num_evals)``: the templates with sub-expression constants and
    parameters set, the structure untouched.  The optimiser iterates on the scalar vector (ties)."""
    from . import loss as _loss
    from .constant_optimization import device_optimizer_supported
    from .device import get_context

    if not device_optimizer_supported(options):
        raise NotImplementedError(f"optimizer_algorithm={options.optimizer_algorithm!r} runs on the reference's CPU "
                                  "optimize_constants; the device optimiser is BFGS + BackTracking")
    plan = _Plan(templates, dataset, options)
    nt = len(plan.templates)
    full, idx = dataset.full, dataset.indices
    iterations = iterations if iterations is not None else getattr(options, "optimizer_iterations", 8)
    f_calls_limit = f_calls_limit if f_calls_limit is not None else getattr(options, "optimizer_f_calls_limit", 10_000)
    nrestarts = nrestarts if nrestarts is not None else getattr(options, "optimizer_nrestarts", 2)
    seed = int((rng if rng is not None else np.random.default_rng()).integers(0, 2 ** 63))
    new = [t.copy() for t in plan.templates]
    losses = np.full(nt, np.inf, dtype=full.dtype)
    improved = np.zeros(nt, dtype=bool)
    num_evals = np.zeros(nt)
    if plan.batch is None:
        return new, losses, improved, num_evals
    ctx = ctx or get_context()
    # a candidate with guards is optimised on its main tree; its guards depend on the scalars too, so whether
    # the adopted scalars keep them finite is checked by the final loss call below
    tb = plan.batch.take(np.arange(plan.n_main)) if plan.batch.n_trees > plan.n_main else plan.batch
    n_const_main = int(np.count_nonzero(tb.constant_mask()))
    plan_slot, plan_nsc = plan.slot[:n_const_main], plan.n_scalars[:plan.n_main]
    K, C = (int(tb.parameters.shape[1]), int(tb.parameters.shape[2])) if tb.parametric else (0, 0)
    ties = _lib.SrScalarTies()
    slot_keep = np.ascontiguousarray(plan_slot if plan_slot.size else np.zeros(1, np.int32))
    nsc_keep = np.ascontiguousarray(plan_nsc)
    ties.slot = slot_keep.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    ties.n_scalars = nsc_keep.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    scal = np.zeros(max(1, int(plan_nsc.sum())), dtype=full.dtype)
    mats = np.zeros((max(1, plan.n_main), max(1, C), max(1, K)), dtype=full.dtype)
    l = np.zeros(plan.n_main, dtype=full.dtype)
    imp = np.zeros(plan.n_main, dtype=np.uint8)
    fc = np.zeros(plan.n_main, dtype=np.int64)
    rows = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    s = tb.to_struct()
    ps = _loss._param_struct(tb, full, plan.options) if tb.parametric else None
    _lib.check(_lib.lib.sr_optimize_constants_batch_tied(
        ctx.handle, full.device_handle(ctx), ctx.opset_id(plan.options.operators), ctypes.byref(s),
        None if ps is None else ctypes.byref(ps), ctypes.byref(ties), p(rows), 0 if rows is None else rows.size,
        ctx.loss_code(plan.options), int(iterations), int(f_calls_limit), int(nrestarts), ctypes.c_uint64(seed),
        p(scal), p(mats) if tb.parametric else None, p(l), p(imp), p(fc)))
    so = np.concatenate([[0], np.cumsum(plan_nsc.astype(np.int64))])
    for j, i in enumerate(plan.valid):
        dev = np.concatenate([scal[so[j]:so[j + 1]], mats[j].reshape(-1)[:K * C] if K else np.zeros(0, full.dtype)])
        vec = plan.to_template_order(dev, plan.composed[i], C)
        # a scalar with no constant node in the main tree (an unread parameter entry, a sub-expression called
        # only inside a dropped argument) is not fitted: the library returns 0 for it, the template keeps its own
        absent = np.ones(vec.size, dtype=bool)
        absent[[s for s in plan.composed[i].slots if s >= 0]] = False
        for lo, hi in plan._ranges:
            absent[lo:hi] = False
        vec[absent] = get_scalar_constants(plan.templates[i])[absent]
        set_scalar_constants(new[i], vec)
        losses[i], improved[i] = l[j], bool(imp[j])
        num_evals[i] = (fc[j] + int(imp[j])) * dataset.dataset_fraction()
    if any(plan.composed[i].guards for i in plan.valid):
        lg, ok = eval_loss_batch(new, dataset, options, ctx=ctx)
        for i in plan.valid:
            if plan.composed[i].guards and not ok[i]:  # the adopted scalars break a guard: keep the start
                new[i], improved[i] = plan.templates[i].copy(), False
                losses[i] = eval_loss_batch([plan.templates[i]], dataset, options, ctx=ctx)[0][0]
    return new, losses, improved, num_evals
