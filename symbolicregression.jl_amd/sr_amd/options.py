"""``Options`` — the subset of SymbolicRegression's options that the scoring path reads.

Reference: src/Options.jl:502-1214 (constructor + defaults), src/OptionsStruct.jl:177-259 (struct).
The scoring path uses: the operator enum (after OP_MAP), ``elementwise_loss`` (default
``L2DistLoss()``, src/Options.jl:772), ``parsimony`` (stored as Float32, src/OptionsStruct.jl:198),
``loss_function``/``loss_function_expression`` (custom objectives stay on the caller's CPU path) and
the new ``device`` switch that selects this evaluator (it rides next to ``turbo``/``bumper``,
src/OptionsStruct.jl:186-187).
"""
from __future__ import annotations

import ast
import re

import numpy as np

from .operators import BINARY_ALIASES, UNARY_ALIASES, OperatorEnum

# Elementwise losses the device evaluates: the LossFunctions.jl catalog src/Options.jl:301-328 lists,
# as (SrLossKind, parameter name or None).  Kinds match include/sr_amd.h SR_LOSS_*.
LOSS_KINDS = {
    "L2DistLoss": (0, None), "L1DistLoss": (1, None), "LPDistLoss": (2, "P"), "LogitDistLoss": (3, None),
    "HuberLoss": (4, "d"), "L1EpsilonInsLoss": (5, "eps"), "L2EpsilonInsLoss": (6, "eps"),
    "PeriodicLoss": (7, "circ"), "QuantileLoss": (8, "tau"), "ZeroOneLoss": (9, None),
    "PerceptronLoss": (10, None), "L1HingeLoss": (11, None), "L2HingeLoss": (12, None),
    "SmoothedL1HingeLoss": (13, "gamma"), "ModifiedHuberLoss": (14, None), "L2MarginLoss": (15, None),
    "ExpLoss": (16, None), "SigmoidLoss": (17, None), "DWDMarginLoss": (18, "q"),
}
LOSS_DEFAULTS = {"HuberLoss": 1.0}  # LossFunctions' HuberLoss() default delta
LOSSES = {"l2": 0, "l1": 1}  # short aliases
# Parameters that must be positive (sr_register_loss refuses the same): every one but QuantileLoss's tau.
# LossFunctions' constructors assert these as far as memory of the package goes (it is not vendored); circ and
# gamma are divisors of the device formulas, so 0 is refused whatever the package does.
LOSS_POSITIVE = ("P", "d", "eps", "circ", "gamma", "q")


def parse_loss(spec):
    """'HuberLoss(1.5)', 'LPDistLoss{3}()', 'QuantileLoss(0.3)', 'L2DistLoss()', ... -> (kind, param)."""
    if isinstance(spec, str) and spec in LOSSES:
        return LOSSES[spec], 0.0
    if not isinstance(spec, str):
        raise ValueError(f"elementwise_loss {spec!r} is not supported by the device path")
    m = re.fullmatch(r"\s*([A-Za-z0-9]+)\s*(?:\{\s*([^}]*)\s*\})?\s*(?:\(\s*([^)]*)\s*\))?\s*", spec)
    if not m or m.group(1) not in LOSS_KINDS:
        raise ValueError(f"elementwise_loss {spec!r} is not supported by the device path")
    name, curly, paren = m.group(1), m.group(2), m.group(3)
    kind, pname = LOSS_KINDS[name]
    arg = (curly or "").strip() or (paren or "").strip()
    if pname is None:
        if arg:
            raise ValueError(f"{name} takes no parameter")
        return kind, 0.0
    if not arg:
        if name not in LOSS_DEFAULTS:
            raise ValueError(f"{name} needs its parameter {pname}, e.g. {name}(1.0)")
        return kind, LOSS_DEFAULTS[name]
    value = float(arg)
    if not np.isfinite(value) or (pname in LOSS_POSITIVE and not value > 0):
        raise ValueError(f"{name}: the parameter {pname} must be {'positive' if pname in LOSS_POSITIVE else 'finite'}, got {arg}")
    return kind, value


# An elementwise loss given as an expression (include/sr_amd.h sr_register_loss_expr): SrLossKind's
# SR_LOSS_EXPR, after the catalog.
LOSS_KIND_EXPR = 19
# The expression's operators: the whole device catalog, whatever the search's own operator set is.
LOSS_OPERATORS = OperatorEnum(sorted(set(UNARY_ALIASES.values())), sorted(set(BINARY_ALIASES.values())))
_LOSS_FORMS = (
    re.compile(r"\s*[A-Za-z_]\w*\s*\(([^()]*)\)\s*=(?!=)(.+)", re.S),  # loss(pred, target[, weight]) = BODY
    re.compile(r"\s*\(([^()]*)\)\s*->(.+)", re.S),                     # (pred, target[, weight]) -> BODY
)


class LossExpression:
    """``"loss(prediction, target) = BODY"`` or ``"(prediction, target) -> BODY"``, with two or three
    argument names of the user's choice (the third is the weight) — the forms SymbolicRegression.jl
    (``elementwise_loss = (x, y) -> ...``, src/LossFunctions.jl:38-58) and PySR users write.  ``BODY`` is an
    expression over those names, numbers and the operators of the device catalog (``LOSS_OPERATORS``); it is
    parsed by ``parse_expression`` into ``tree``, whose leaves are feature 1 = prediction, 2 = target,
    3 = weight.  ``ValueError`` for an unknown name or operator and for fewer than two or more than three
    arguments.  The device evaluates it in the dataset's element type (constants rounded to it)."""

    def __init__(self, spec: str):
        from .node import parse_expression

        m = next((m for m in (f.fullmatch(spec) for f in _LOSS_FORMS) if m), None)
        if m is None:
            raise ValueError(f"elementwise_loss {spec!r}: expected 'loss(prediction, target) = BODY' or "
                             "'(prediction, target) -> BODY'")
        names = [a.strip() for a in m.group(1).split(",")]
        if not 2 <= len(names) <= 3:
            raise ValueError(f"elementwise_loss {spec!r}: a loss takes (prediction, target) or (prediction, target, "
                             f"weight), got {len(names)} arguments")
        if any(not n.isidentifier() for n in names) or len(set(names)) != len(names):
            raise ValueError(f"elementwise_loss {spec!r}: bad argument names {names}")
        try:
            body = ast.parse(m.group(2).strip().replace("^", "**"), mode="eval")
        except SyntaxError as e:
            raise ValueError(f"elementwise_loss {spec!r}: cannot parse the body ({e.msg})") from None
        called = {id(c.func) for c in ast.walk(body) if isinstance(c, ast.Call)}
        for n in ast.walk(body):
            if isinstance(n, ast.Name) and id(n) not in called:
                if n.id in names:
                    n.id = f"x{names.index(n.id) + 1}"
                elif n.id not in ("inf", "Inf", "nan", "NaN"):
                    raise ValueError(f"elementwise_loss {spec!r}: unknown name {n.id!r} (arguments: {names})")
        try:
            self.tree = parse_expression(ast.unparse(body), LOSS_OPERATORS)
        except ValueError as e:
            raise ValueError(f"elementwise_loss {spec!r}: {e}") from None
        except (AttributeError, KeyError) as e:
            raise ValueError(f"elementwise_loss {spec!r}: cannot parse the body ({e!r})") from None
        self.spec = spec
        self.n_args = len(names)
        self.operators = LOSS_OPERATORS

    def batch(self):
        """The tree as a one-tree TreeBatch with Float64 constants (what sr_register_loss_expr takes)."""
        from .node import flatten_trees

        return flatten_trees([self.tree], np.float64)

    def key(self):
        b = self.batch()
        return (b.degree.tobytes(), b.op.tobytes(), b.feature.tobytes(), b.constant.tobytes(), b.val.tobytes())

    def host_eval(self, prediction, target, weight=None, deriv=False):
        """The library's host interpreter (sr_loss_expr_host: the compiler and interpreter the kernels run,
        no device needed) on arrays of one dtype (Float32 / Float64): L(prediction, target, weight), and with
        ``deriv`` also d L / d prediction by forward mode."""
        import ctypes

        from . import _lib

        p = np.ascontiguousarray(prediction)
        if p.dtype not in (np.float32, np.float64):
            raise ValueError("host_eval takes Float32 or Float64 arrays")
        t = np.ascontiguousarray(target, dtype=p.dtype)
        w = None if weight is None else np.ascontiguousarray(weight, dtype=p.dtype)
        if t.shape != p.shape or (w is not None and w.shape != p.shape):
            raise ValueError("prediction, target and weight must have one shape")
        ops, b = self.operators, self.batch()
        un = (ctypes.c_char_p * max(1, len(ops.unaops)))(*[s.encode() for s in ops.unaops])
        bi = (ctypes.c_char_p * max(1, len(ops.binops)))(*[s.encode() for s in ops.binops])
        ts = b.to_struct()
        out = np.empty_like(p)
        dout = np.empty_like(p) if deriv else None
        ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        _lib.check(_lib.lib.sr_loss_expr_host(_lib.SR_DTYPE_F32 if p.dtype == np.float32 else _lib.SR_DTYPE_F64,
                                              len(ops.unaops), un, len(ops.binops), bi, ctypes.byref(ts), p.size,
                                              ptr(p), ptr(t), ptr(w), ptr(out), ptr(dout)))
        return (out, dout) if deriv else out

    def __repr__(self):
        return f"LossExpression({self.spec!r})"


class ParametricExpressionSpec:
    """``ParametricExpressionSpec(max_parameters=...)`` (src/ParametricExpression.jl): expressions are
    ``ParametricExpression``s with ``p1..p<max_parameters>`` leaves, one parameter column per class."""

    def __init__(self, *, max_parameters: int):
        if int(max_parameters) < 1:
            raise ValueError("max_parameters must be positive")
        self.max_parameters = int(max_parameters)

    def __repr__(self):
        return f"ParametricExpressionSpec(max_parameters={self.max_parameters})"


class Options:
    def __init__(
        self,
        binary_operators=("+", "-", "/", "*"),
        unary_operators=(),
        *,
        operators: OperatorEnum | None = None,
        elementwise_loss="L2DistLoss",
        loss_function=None,
        loss_function_expression=None,
        parsimony: float = 0.0,
        maxsize: int = 30,
        maxdepth: int | None = None,
        populations: int = 31,
        population_size: int = 27,
        ncycles_per_iteration: int = 380,
        tournament_selection_n: int = 15,
        tournament_selection_p: float = 0.982,
        batching: bool = False,
        batch_size: int = 50,
        should_optimize_constants: bool = True,
        optimizer_probability: float = 0.14,
        optimizer_nrestarts: int = 2,
        optimizer_iterations: int | None = None,
        optimizer_f_calls_limit: int | None = None,
        optimizer_algorithm: str = "BFGS",
        turbo: bool = False,
        bumper: bool = False,
        device: str = "mi355x",
        deterministic: bool = False,
        seed=None,
        expression_spec=None,
    ):
        self.operators = operators if operators is not None else OperatorEnum(unary_operators, binary_operators)
        if callable(elementwise_loss) and not isinstance(elementwise_loss, str):
            raise ValueError("custom elementwise loss functions stay on the reference CPU path")
        self.elementwise_loss = elementwise_loss
        # "loss(pred, target) = BODY" / "(pred, target) -> BODY": an expression loss (its tree is kept here;
        # Context.loss_code registers it once per context); any other string is a catalog loss, as before
        self.loss_expression = None
        if isinstance(elementwise_loss, str) and ("=" in elementwise_loss or "->" in elementwise_loss):
            self.loss_expression = LossExpression(elementwise_loss)
            self.loss_kind, self.loss_param = LOSS_KIND_EXPR, 0.0
        else:
            self.loss_kind, self.loss_param = parse_loss(elementwise_loss)
        self.loss_function = loss_function
        self.loss_function_expression = loss_function_expression
        self.parsimony = np.float32(parsimony)
        self.maxsize = int(maxsize)
        self.maxdepth = int(maxdepth) if maxdepth is not None else int(maxsize)
        self.populations = populations
        self.population_size = population_size
        self.ncycles_per_iteration = ncycles_per_iteration
        self.tournament_selection_n = tournament_selection_n
        self.tournament_selection_p = tournament_selection_p
        self.batching = batching
        self.batch_size = batch_size
        # constant optimisation (src/Options.jl:613-619, 988-997)
        self.should_optimize_constants = should_optimize_constants
        self.optimizer_probability = optimizer_probability
        self.optimizer_nrestarts = optimizer_nrestarts
        self.optimizer_iterations = 8 if optimizer_iterations is None else int(optimizer_iterations)
        self.optimizer_f_calls_limit = 10_000 if optimizer_f_calls_limit is None else int(optimizer_f_calls_limit)
        # the device optimiser is Optim's BFGS with BackTracking (Newton for one constant, as the
        # reference chooses); any other algorithm (the reference accepts "NelderMead",
        # src/Options.jl:738-746) stays on the reference's CPU optimize_constants
        if str(optimizer_algorithm) not in ("BFGS", "NelderMead"):
            raise ValueError(f"unknown optimizer_algorithm {optimizer_algorithm!r}")
        self.optimizer_algorithm = str(optimizer_algorithm)
        self.turbo = turbo
        self.bumper = bumper
        if device not in ("mi355x", "gpu", "hip"):
            raise ValueError("this package implements only the MI355X device path (device='mi355x')")
        self.device = "mi355x"
        self.deterministic = deterministic
        self.seed = seed
        # None (plain Expression{T,Node{T,2}}), a ParametricExpressionSpec or a TemplateExpressionSpec; the scoring calls take either
        # kind of tree whatever the spec says, the spec bounds a parametric tree's parameter indices
        if expression_spec is not None and not isinstance(expression_spec, ParametricExpressionSpec):
            from .template import TemplateExpressionSpec  # (imports this module's neighbours: resolved here)

            if not isinstance(expression_spec, TemplateExpressionSpec):
                raise ValueError("expression_spec: only ParametricExpressionSpec and TemplateExpressionSpec are "
                                 "supported by the device path")
        self.expression_spec = expression_spec

    @property
    def nops(self):
        return self.operators.nops

    def __repr__(self):
        return f"Options(operators={self.operators!r}, elementwise_loss={self.elementwise_loss}, parsimony={self.parsimony})"
