"""Expression trees with DynamicExpressions' ``Node{T,2}`` fields, and their pre-order flattening.

Fields follow DE 2.x: ``degree`` (0 leaf / 1 unary / 2 binary), ``constant``, ``val``, ``feature``
(1-based), ``op`` (1-based index into ``options.operators.ops[degree]``), children ``l``/``r``.
``flatten_trees`` produces the struct-of-arrays ``sr_tree_batch`` the C ABI takes (pre-order =
``get_scalar_constants`` order, test/integration/ad/zygote/test_derivatives.jl:127-155).

``ParametricExpression`` (src/ParametricExpression.jl) adds DE's ``ParametricNode`` fields: a leaf with
``is_parameter`` reads ``parameters[parameter, class[row]]`` of its expression's own
``(max_parameters, n_classes)`` matrix; ``flatten_trees`` of such expressions also yields the
``sr_param_batch`` arrays (a batch is all plain or all parametric).
"""
from __future__ import annotations

import ast
import ctypes
from typing import Iterable, List, Optional, Sequence

import numpy as np

from . import _lib
from .operators import OperatorEnum, canonical_binary, canonical_unary, print_name


class Node:
    __slots__ = ("degree", "constant", "val", "feature", "op", "l", "r", "is_parameter", "parameter")

    def __init__(self, *args, val=None, feature=None, op=None, l=None, r=None, children=None, parameter=None):
        # Node("x3") / Node(feature=3) / Node(val=1.5) / Node(op=1, l=..) / Node(op=2, l=.., r=..)
        # Node("p2") / Node(parameter=2): a ParametricNode's parameter leaf
        self.is_parameter = False
        self.parameter = 0
        self.degree = 0
        self.constant = False
        self.val = 0.0
        self.feature = 0
        self.op = 0
        self.l = None
        self.r = None
        if args:
            if len(args) == 1 and isinstance(args[0], str):
                s = args[0]
                if s.startswith("p") and s[1:].isdigit():
                    parameter = int(s[1:])
                elif not s.startswith("x"):
                    raise ValueError(f"variable names must look like 'x1' (parameters 'p1'), got {s!r}")
                else:
                    feature = int(s[1:])
            elif isinstance(args[0], int) and len(args) in (2, 3):
                op = args[0]
                children = args[1:]
            else:
                raise ValueError(f"unsupported Node constructor arguments {args!r}")
        if children is not None:
            children = tuple(children)
            if len(children) == 1:
                l = children[0]
            elif len(children) == 2:
                l, r = children
        if op is not None:
            if l is None:
                raise ValueError("operator node needs children")
            self.op = int(op)
            self.l = l
            self.r = r
            self.degree = 2 if r is not None else 1
        elif parameter is not None:
            if int(parameter) < 1:
                raise ValueError("parameters are numbered from 1")
            self.is_parameter = True
            self.parameter = int(parameter)
        elif feature is not None:
            self.feature = int(feature)
        elif val is not None:
            self.constant = True
            self.val = val
        else:
            raise ValueError("Node needs val=, feature=, parameter= or op=")

    # ------------------------------------------------------------------ DE-style utilities
    def copy(self) -> "Node":
        n = Node.__new__(Node)
        n.degree, n.constant, n.val, n.feature, n.op = self.degree, self.constant, self.val, self.feature, self.op
        n.is_parameter, n.parameter = self.is_parameter, self.parameter
        n.l = self.l.copy() if self.l is not None else None
        n.r = self.r.copy() if self.r is not None else None
        return n

    def set_node(self, other: "Node") -> None:
        """DE ``set_node!``: overwrite this node's contents with ``other``'s."""
        self.degree, self.constant, self.val, self.feature, self.op = (
            other.degree, other.constant, other.val, other.feature, other.op)
        self.is_parameter, self.parameter = other.is_parameter, other.parameter
        self.l, self.r = other.l, other.r

    def preorder(self) -> List["Node"]:
        out, stack = [], [self]
        push, pop, emit = stack.append, stack.pop, out.append  # hot in the host search loop
        while stack:
            n = pop()
            emit(n)
            d = n.degree
            if d:
                if d == 2:
                    push(n.r)
                push(n.l)
        return out

    def count_nodes(self) -> int:
        return len(self.preorder())

    def count_constants(self) -> int:
        return sum(1 for n in self.preorder() if n.degree == 0 and n.constant)

    def count_depth(self) -> int:
        if self.degree == 0:
            return 1
        if self.degree == 1:
            return 1 + self.l.count_depth()
        return 1 + max(self.l.count_depth(), self.r.count_depth())

    def is_constant(self) -> bool:
        return all(n.constant for n in self.preorder() if n.degree == 0)

    def __repr__(self):
        return f"Node({string_tree(self)})"

    # arithmetic sugar, resolved against the operators activated by `extend_operators`
    def _bin(self, name, other, swap=False):
        ops = _active_operators()
        o = other if isinstance(other, Node) else Node(val=other)
        a, b = (o, self) if swap else (self, o)
        return Node(op=ops.binary_index(name), l=a, r=b)

    def __add__(self, o): return self._bin("+", o)
    def __radd__(self, o): return self._bin("+", o, True)
    def __sub__(self, o): return self._bin("-", o)
    def __rsub__(self, o): return self._bin("-", o, True)
    def __mul__(self, o): return self._bin("*", o)
    def __rmul__(self, o): return self._bin("*", o, True)
    def __truediv__(self, o): return self._bin("/", o)
    def __rtruediv__(self, o): return self._bin("/", o, True)
    def __pow__(self, o): return self._bin("^", o)
    def __rpow__(self, o): return self._bin("^", o, True)
    def __neg__(self): return apply_unary("neg", self)


def get_scalar_constants(tree: Node) -> np.ndarray:
    return np.array([n.val for n in tree.preorder() if n.degree == 0 and n.constant])


def set_scalar_constants(tree: Node, values: Sequence[float]) -> None:
    k = 0
    for n in tree.preorder():
        if n.degree == 0 and n.constant:
            n.val = values[k]
            k += 1


# ------------------------------------------------------------------ operator context (@extend_operators)
_ACTIVE: List[OperatorEnum] = []


def extend_operators(options_or_ops) -> None:
    """Make Node arithmetic and ``apply_unary`` resolve operator indices against these operators
    (the role of DynamicExpressions' ``@extend_operators``)."""
    ops = getattr(options_or_ops, "operators", options_or_ops)
    _ACTIVE[:] = [ops]


def _active_operators() -> OperatorEnum:
    if not _ACTIVE:
        raise RuntimeError("call extend_operators(options) before building trees with operators")
    return _ACTIVE[0]


def apply_unary(name, child, operators: Optional[OperatorEnum] = None) -> Node:
    ops = operators or _active_operators()
    c = child if isinstance(child, Node) else Node(val=child)
    return Node(op=ops.unary_index(name), l=c)


def apply_binary(name, a, b, operators: Optional[OperatorEnum] = None) -> Node:
    ops = operators or _active_operators()
    a = a if isinstance(a, Node) else Node(val=a)
    b = b if isinstance(b, Node) else Node(val=b)
    return Node(op=ops.binary_index(name), l=a, r=b)


# ------------------------------------------------------------------ printing / parsing
def string_tree(tree: Node, operators: Optional[OperatorEnum] = None) -> str:
    ops = operators or (_ACTIVE[0] if _ACTIVE else None)

    def name(deg, op):
        if ops is None:
            return f"op{deg}_{op}"
        return print_name(ops.ops[deg][op - 1])

    def rec(n: Node) -> str:
        if n.degree == 0:
            if n.is_parameter:
                return f"p{n.parameter}"
            return repr(n.val) if n.constant else f"x{n.feature}"
        if n.degree == 1:
            return f"{name(1, n.op)}({rec(n.l)})"
        nm = name(2, n.op)
        if nm in ("+", "-", "*", "/", "^", ">", "<", ">=", "<="):
            return f"({rec(n.l)} {nm} {rec(n.r)})"
        return f"{nm}({rec(n.l)}, {rec(n.r)})"

    return rec(tree)


_PY_BINOPS = {ast.Add: "+", ast.Sub: "-", ast.Mult: "*", ast.Div: "/", ast.Pow: "^"}
_PY_CMP = {ast.Gt: ">", ast.Lt: "<", ast.GtE: ">=", ast.LtE: "<="}


def parse_expression(expr: str, operators) -> Node:
    """Parse e.g. ``"cos(x1 * 3.0) + x2 ^ 2"`` into a Node using ``operators`` (or Options)."""
    ops = getattr(operators, "operators", operators)
    expr = expr.replace("^", "**")

    def rec(e):
        if isinstance(e, ast.Expression):
            return rec(e.body)
        if isinstance(e, ast.Constant):
            return Node(val=float(e.value))
        if isinstance(e, ast.Name):
            if e.id in ("inf", "Inf"):
                return Node(val=float("inf"))
            if e.id in ("nan", "NaN"):
                return Node(val=float("nan"))
            return Node(e.id)
        if isinstance(e, ast.UnaryOp) and isinstance(e.op, ast.USub):
            if isinstance(e.operand, ast.Constant):
                return Node(val=-float(e.operand.value))
            if "neg" in ops.unaops:
                return Node(op=ops.unary_index("neg"), l=rec(e.operand))
            return Node(op=ops.binary_index("*"), l=Node(val=-1.0), r=rec(e.operand))
        if isinstance(e, ast.BinOp):
            return Node(op=ops.binary_index(_PY_BINOPS[type(e.op)]), l=rec(e.left), r=rec(e.right))
        if isinstance(e, ast.Compare) and len(e.ops) == 1:
            return Node(op=ops.binary_index(_PY_CMP[type(e.ops[0])]), l=rec(e.left), r=rec(e.comparators[0]))
        if isinstance(e, ast.Call):
            fname = e.func.id
            args = [rec(a) for a in e.args]
            if len(args) == 1:
                return Node(op=ops.unary_index(fname), l=args[0])
            if len(args) == 2:
                return Node(op=ops.binary_index(fname), l=args[0], r=args[1])
        raise ValueError(f"cannot parse {ast.dump(e)}")

    return rec(ast.parse(expr, mode="eval"))


class ParametricExpression:
    """``ParametricExpression(tree, parameters)``: a tree whose ``p_k`` leaves read
    ``parameters[k - 1, class - 1]`` per row (``parameters``: ``[max_parameters, n_classes]``, the layout
    of ``get_metadata(ex).parameters``)."""

    def __init__(self, tree: "Node", parameters):
        self.tree = tree
        self.parameters = np.asarray(parameters)
        if self.parameters.ndim != 2:
            raise ValueError("parameters must be a [max_parameters, n_classes] matrix")
        kmax = max((n.parameter for n in tree.preorder() if n.degree == 0 and n.is_parameter), default=0)
        if kmax > self.parameters.shape[0]:
            raise ValueError(f"tree uses p{kmax} but parameters has {self.parameters.shape[0]} rows")

    @property
    def max_parameters(self) -> int:
        return int(self.parameters.shape[0])

    @property
    def n_classes(self) -> int:
        return int(self.parameters.shape[1])

    def copy(self) -> "ParametricExpression":
        return ParametricExpression(self.tree.copy(), self.parameters.copy())

    def __repr__(self):
        return f"ParametricExpression({string_tree(self.tree)}, parameters={self.parameters.tolist()})"


# ------------------------------------------------------------------ flattening for the C ABI
class TreeBatch:
    """Pre-order struct-of-arrays of many trees, kept alive while the C call runs.  A parametric batch
    also holds ``is_parameter`` / ``parameter`` per node and ``parameters[n_trees, max_parameters,
    n_classes]`` (the ``sr_param_batch`` arrays); a plain batch has ``is_parameter = None``."""

    def __init__(self, offsets, degree, op, feature, constant, val, is_parameter=None, parameter=None,
                 parameters=None):
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.degree = np.ascontiguousarray(degree, dtype=np.uint8)
        self.op = np.ascontiguousarray(op, dtype=np.uint8)
        self.feature = np.ascontiguousarray(feature, dtype=np.uint16)
        self.constant = np.ascontiguousarray(constant, dtype=np.uint8)
        self.val = np.ascontiguousarray(val)
        self.n_trees = len(self.offsets) - 1
        self.is_parameter = self.parameter = self.parameters = None
        if is_parameter is not None:
            self.is_parameter = np.ascontiguousarray(is_parameter, dtype=np.uint8)
            self.parameter = np.ascontiguousarray(parameter, dtype=np.uint16)
            self.parameters = np.ascontiguousarray(parameters, dtype=self.val.dtype)
            if self.parameters.ndim != 3 or self.parameters.shape[0] != self.n_trees:
                raise ValueError("parameters must be [n_trees, max_parameters, n_classes]")
            if self.is_parameter.shape != self.degree.shape or self.parameter.shape != self.degree.shape:
                raise ValueError("is_parameter / parameter must have one entry per node")

    @property
    def parametric(self) -> bool:
        return self.is_parameter is not None

    def _sel(self, offs, nodes, trees, val=None) -> "TreeBatch":
        """The batch of the given nodes / trees (index arrays or slices), parameter side included."""
        p = self.parametric
        return TreeBatch(offs, self.degree[nodes], self.op[nodes], self.feature[nodes], self.constant[nodes],
                         self.val[nodes] if val is None else val, self.is_parameter[nodes] if p else None,
                         self.parameter[nodes] if p else None, self.parameters[trees] if p else None)

    def to_param_struct(self) -> "_lib.SrParamBatch":
        """The ``sr_param_batch`` of a parametric batch (keep the returned struct alive during the call)."""
        if not self.parametric:
            raise ValueError("not a parametric batch")
        s = _lib.SrParamBatch()
        # each tree's matrix in Julia's column-major (max_parameters, n_classes) layout
        self._params_jl = np.ascontiguousarray(self.parameters.transpose(0, 2, 1))
        s.is_parameter = self.is_parameter.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        s.parameter = self.parameter.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))
        s.max_parameters = int(self.parameters.shape[1])
        s.n_classes = int(self.parameters.shape[2])
        s.parameters = self._params_jl.ctypes.data_as(ctypes.c_void_p)
        return s

    @property
    def n_nodes(self) -> int:
        return int(self.offsets[-1])

    @property
    def n_operator_nodes(self) -> int:
        return int(np.count_nonzero(self.degree))

    def astype(self, dtype) -> "TreeBatch":
        return TreeBatch(self.offsets, self.degree, self.op, self.feature, self.constant, self.val.astype(dtype),
                         self.is_parameter, self.parameter,
                         self.parameters.astype(dtype) if self.parametric else None)

    def tree_sizes(self) -> np.ndarray:
        return np.diff(self.offsets)

    def take(self, idx) -> "TreeBatch":
        """The batch of trees idx (in that order): the node arrays of each, concatenated."""
        idx = np.asarray(idx, dtype=np.int64)
        b, e = self.offsets[idx], self.offsets[idx + 1]
        nodes = np.concatenate([np.arange(x, y) for x, y in zip(b, e)]) if idx.size else np.zeros(0, np.int64)
        offs = np.concatenate([[0], np.cumsum(e - b)])
        return self._sel(offs, nodes, idx)

    def to_struct(self) -> _lib.SrTreeBatch:
        def ptr(a, t):
            return a.ctypes.data_as(ctypes.POINTER(t))

        s = _lib.SrTreeBatch()
        s.n_trees = self.n_trees
        s.offsets = ptr(self.offsets, ctypes.c_int64)
        s.degree = ptr(self.degree, ctypes.c_uint8)
        s.op = ptr(self.op, ctypes.c_uint8)
        s.feature = ptr(self.feature, ctypes.c_uint16)
        s.constant = ptr(self.constant, ctypes.c_uint8)
        s.val = self.val.ctypes.data_as(ctypes.c_void_p)
        return s

    def constant_mask(self) -> np.ndarray:
        return (self.degree == 0) & (self.constant != 0)

    def constant_offsets(self) -> np.ndarray:
        """[n_trees + 1] prefix sum of per-tree constant counts (pre-order, get_scalar_constants)."""
        m = self.constant_mask().astype(np.int64)
        c = np.concatenate([[0], np.cumsum(m)])
        return c[self.offsets]

    def get_constants(self) -> np.ndarray:
        """All trees' constants, pre-order per tree, concatenated (see constant_offsets)."""
        return self.val[self.constant_mask()].copy()

    def with_constants(self, consts) -> "TreeBatch":
        """Same trees with their constants replaced (set_scalar_constants! for the whole batch)."""
        val = self.val.copy()
        val[self.constant_mask()] = np.asarray(consts, dtype=val.dtype)
        return self._sel(self.offsets, slice(None), slice(None), val)

    # The scalars the optimiser fits and the gradient calls differentiate: a plain tree's constants; for a
    # ParametricExpression tree DynamicExpressions' get_scalar_constants order, the constants in pre-order
    # followed by vec(parameters) column-major (entry (k-1) + max_parameters (c-1): ``parameters[t].T.ravel()``),
    # every entry present whether the tree uses it or not.
    def scalar_offsets(self) -> np.ndarray:
        """[n_trees + 1]: where each tree's scalars start in ``get_scalar_constants()`` / a flat gradient
        (``constant_offsets()`` for a plain batch)."""
        c = self.constant_offsets()
        if not self.parametric:
            return c
        kc = int(self.parameters.shape[1]) * int(self.parameters.shape[2])
        return c + kc * np.arange(self.n_trees + 1, dtype=np.int64)

    def get_scalar_constants(self) -> np.ndarray:
        """All trees' scalars, concatenated (see ``scalar_offsets``)."""
        if not self.parametric:
            return self.get_constants()
        c, co = self.get_constants(), self.constant_offsets()
        so = self.scalar_offsets()
        x = np.empty(int(so[-1]), dtype=self.val.dtype)
        for t in range(self.n_trees):
            nc = int(co[t + 1] - co[t])
            x[so[t]:so[t] + nc] = c[co[t]:co[t + 1]]
            x[so[t] + nc:so[t + 1]] = self.parameters[t].T.ravel()
        return x

    def split_scalars(self, flat):
        """A flat vector in the ``scalar_offsets`` layout (scalars or a gradient) -> (the constants' part,
        concatenated as ``get_constants``; the parameters' part as ``[n_trees, max_parameters, n_classes]``,
        None for a plain batch)."""
        flat = np.asarray(flat)
        if not self.parametric:
            return flat.copy(), None
        co, so = self.constant_offsets(), self.scalar_offsets()
        if flat.shape != (int(so[-1]),):
            raise ValueError(f"expected {int(so[-1])} scalars, got {flat.shape}")
        K, C = int(self.parameters.shape[1]), int(self.parameters.shape[2])
        consts = np.empty(int(co[-1]), dtype=flat.dtype)
        mats = np.empty((self.n_trees, K, C), dtype=flat.dtype)
        for t in range(self.n_trees):
            nc = int(co[t + 1] - co[t])
            consts[co[t]:co[t + 1]] = flat[so[t]:so[t] + nc]
            mats[t] = flat[so[t] + nc:so[t + 1]].reshape(C, K).T
        return consts, mats

    def with_scalar_constants(self, x) -> "TreeBatch":
        """Same trees with their scalars replaced (set_scalar_constants! for the whole batch)."""
        if not self.parametric:
            return self.with_constants(x)
        consts, mats = self.split_scalars(np.asarray(x, dtype=self.val.dtype))
        out = self.with_constants(consts)
        out.parameters = np.ascontiguousarray(mats, dtype=self.val.dtype)
        return out

    def subset(self, idx) -> "TreeBatch":
        idx = np.asarray(idx, dtype=np.int64)
        starts, ends = self.offsets[idx], self.offsets[idx + 1]
        sel = np.concatenate([np.arange(s, e) for s, e in zip(starts, ends)]) if len(idx) else np.zeros(0, np.int64)
        offs = np.concatenate([[0], np.cumsum(ends - starts)])
        return self._sel(offs, sel, idx)

    def tree(self, k: int) -> Node:
        b, e = int(self.offsets[k]), int(self.offsets[k + 1])
        pos = [b]

        def rec():
            i = pos[0]
            pos[0] += 1
            d = int(self.degree[i])
            if d == 0:
                if self.parametric and self.is_parameter[i]:
                    return Node(parameter=int(self.parameter[i]))
                if self.constant[i]:
                    return Node(val=self.val[i].item())
                return Node(feature=int(self.feature[i]))
            l = rec()
            r = rec() if d == 2 else None
            return Node(op=int(self.op[i]), l=l, r=r)

        t = rec()
        assert pos[0] == e
        return ParametricExpression(t, self.parameters[k].copy()) if self.parametric else t


def flatten_trees(trees: Iterable[Node], dtype=np.float32) -> TreeBatch:
    nodes, offsets, mats = [], [0], []
    n_items = 0
    for t in trees:
        n_items += 1
        if isinstance(getattr(t, "tree", None), ParametricExpression):  # a PopMember holding one
            t = t.tree
        if isinstance(t, ParametricExpression):
            mats.append(t.parameters)
        t = getattr(t, "tree", t)  # PopMember / Expression wrappers
        nodes.extend(t.preorder())
        offsets.append(len(nodes))
    if mats and len(mats) != n_items:
        raise ValueError("a batch is either all plain trees or all ParametricExpressions")
    if not mats and any(n.degree == 0 and n.is_parameter for n in nodes):
        raise ValueError("a tree with parameter leaves needs its ParametricExpression (its parameters)")
    if mats and len({m.shape for m in mats}) != 1:
        raise ValueError("every ParametricExpression of a batch needs the same (max_parameters, n_classes)")
    degree = [n.degree for n in nodes]
    op = [n.op for n in nodes]
    feature = [n.feature for n in nodes]
    constant = [1 if (n.degree == 0 and n.constant) else 0 for n in nodes]
    val = [n.val if n.constant else 0.0 for n in nodes]
    if mats:
        isp = [1 if (n.degree == 0 and n.is_parameter) else 0 for n in nodes]
        par = [n.parameter if (n.degree == 0 and n.is_parameter) else 0 for n in nodes]
        return TreeBatch(offsets, degree, op, feature, constant, np.array(val, dtype=dtype), isp, par,
                         np.stack(mats).astype(dtype))
    return TreeBatch(offsets, degree, op, feature, constant, np.array(val, dtype=dtype))
