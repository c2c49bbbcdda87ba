"""CPU: elementwise losses given as expressions — the two string forms ``Options`` accepts, their
``ValueError`` cases, the catalog strings untouched, and the library's host interpreter
(``sr_loss_expr_host``: the compiler and interpreter the kernels run, csrc/sr_loss_expr.h) against numpy and
closed-form derivatives, both element types, and the compiler's limits.  No kernel launches here.
"""
import numpy as np
import pytest

from sr_amd import LossExpression, Options, _lib
from sr_amd.options import LOSS_KIND_EXPR, parse_loss

# (body over p, t; numpy value; numpy d value / d p) — the restated catalog losses and log-cosh
EXPRS = {
    "square(p - t)": (lambda p, t: (p - t) ** 2, lambda p, t: 2 * (p - t)),
    "abs(p - t)": (lambda p, t: np.abs(p - t), lambda p, t: np.sign(p - t)),
    "abs(p - t)^3": (lambda p, t: np.abs(p - t) ** 3, lambda p, t: 3 * (p - t) ** 2 * np.sign(p - t)),
    "-log(4.0) - (p - t) + 2.0*log(1.0 + exp(p - t))":
        (lambda p, t: -np.log(4.0) - (p - t) + 2 * np.log(1 + np.exp(p - t)), lambda p, t: np.tanh((p - t) / 2)),
    "(p - t) * (((p - t) > 0.0) - 0.3)":
        (lambda p, t: (p - t) * ((p - t > 0) - 0.3), lambda p, t: (p - t > 0) - 0.3),
    "square(max(0.0, 1.0 - t*p))":
        (lambda p, t: np.maximum(0, 1 - t * p) ** 2, lambda p, t: -2 * np.maximum(0, 1 - t * p) * t),
    "square(1.0 - t*p)": (lambda p, t: (1 - t * p) ** 2, lambda p, t: -2 * (1 - t * p) * t),
    "exp(-(t*p))": (lambda p, t: np.exp(-(t * p)), lambda p, t: -t * np.exp(-(t * p))),
    "1.0 - tanh(t*p)": (lambda p, t: 1 - np.tanh(t * p), lambda p, t: -(1 - np.tanh(t * p) ** 2) * t),
    "log(cosh(p - t))": (lambda p, t: np.log(np.cosh(p - t)), lambda p, t: np.tanh(p - t)),
}


def _inputs(dtype, n=4001, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2, 2, n).astype(dtype), rng.uniform(-2, 2, n).astype(dtype)


def test_both_string_forms_two_and_three_arguments():
    a = Options(elementwise_loss="loss(prediction, target) = abs(prediction - target)")
    b = Options(elementwise_loss="(x, y) -> abs(x - y)")
    assert a.loss_kind == b.loss_kind == LOSS_KIND_EXPR
    assert a.loss_expression.key() == b.loss_expression.key() and a.loss_expression.n_args == 2
    c = Options(elementwise_loss="myloss(p, t, w) = w * abs(p - t)")
    d = Options(elementwise_loss="(a, b, c) -> c * abs(a - b)")
    assert c.loss_expression.key() == d.loss_expression.key() and c.loss_expression.n_args == 3
    assert c.loss_expression.key() != a.loss_expression.key()
    # the leaves: feature 1 = prediction, 2 = target, 3 = weight; >= in a body is not the definition's =
    tb = Options(elementwise_loss="f(p, t, w) = w * (p >= t)").loss_expression.batch()
    assert sorted(tb.feature[(tb.degree == 0) & (tb.constant == 0)]) == [1, 2, 3]
    assert tb.val.dtype == np.float64 and tb.n_trees == 1


@pytest.mark.parametrize("spec", [
    "loss(p, t) = p - z",                # unknown name
    "loss(p, t) = frobnicate(p) - t",    # unknown operator
    "loss(p, t) = p % t",                # an operator parse_expression does not know
    "loss(p, t, w, v) = p - t",          # more than three arguments
    "loss(p) = p",                       # fewer than two
    "(p) -> p",
    "loss(p, p) = p",                    # repeated argument name
    "loss(p, t) = p +",                  # not an expression
    "p -> p",                            # neither form
    "loss = abs(p - t)",
])
def test_value_errors(spec):
    with pytest.raises(ValueError):
        Options(elementwise_loss=spec)


def test_catalog_strings_parse_as_before():
    for spec, want in [("L2DistLoss()", (0, 0.0)), ("L1DistLoss", (1, 0.0)), ("HuberLoss(1.5)", (4, 1.5)),
                       ("LPDistLoss{3}()", (2, 3.0)), ("QuantileLoss(0.3)", (8, 0.3)), ("l2", (0, 0.0)),
                       ("DWDMarginLoss(2)", (18, 2.0)), ("HuberLoss()", (4, 1.0))]:
        o = Options(elementwise_loss=spec)
        assert (o.loss_kind, o.loss_param) == want == parse_loss(spec)
        assert o.loss_expression is None
    for spec in ("CrossEntropyLoss()", "QuantileLoss", "L2DistLoss(1.0)"):
        with pytest.raises(ValueError):
            Options(elementwise_loss=spec)
    with pytest.raises(ValueError, match="reference CPU path"):
        Options(elementwise_loss=lambda x, y: (x - y) ** 2)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("body", list(EXPRS))
def test_host_interpreter_against_numpy(body, dtype):
    value, deriv = EXPRS[body]
    p, t = _inputs(dtype)
    if "t*p" in body:  # margin losses: classification targets
        t = np.where(t >= 0, 1, -1).astype(dtype)
    ex = LossExpression(f"loss(p, t) = {body}")
    v, d = ex.host_eval(p, t, deriv=True)
    assert v.dtype == dtype and d.dtype == dtype
    assert np.array_equal(v, ex.host_eval(p, t))  # the value pass and the derivative pass agree bit for bit
    # every operation rounds in T: a few ulps of the largest intermediate (|.| <= 64 here) per element
    eps = np.finfo(dtype).eps
    p64, t64 = p.astype(np.float64), t.astype(np.float64)
    rv, rd = value(p64, t64), deriv(p64, t64)
    np.testing.assert_allclose(v, rv, rtol=16 * eps, atol=64 * eps)
    np.testing.assert_allclose(d, rd, rtol=64 * eps, atol=256 * eps)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_interpreter_weights(dtype):
    p, t = _inputs(dtype, seed=1)
    w = np.random.default_rng(2).uniform(0.5, 2.0, p.size).astype(dtype)
    ex = LossExpression("loss(p, t, w) = abs(p - t) / (1.0 + w)")
    v, d = ex.host_eval(p, t, w, deriv=True)
    assert np.array_equal(v, np.abs(p - t) / (dtype(1) + w))      # IEEE operations only: bit for bit
    assert np.array_equal(d, np.sign(p - t) / (dtype(1) + w))     # the weight's side adds no term
    with pytest.raises(_lib.SRError, match="weight"):
        ex.host_eval(p, t)                                          # w referenced, none given
    with pytest.raises(_lib.SRError, match="weight"):
        LossExpression("loss(p, t) = abs(p - t)").host_eval(p, t, w)  # weights given, two arguments


def test_constants_rounded_and_folded_in_T():
    ex = LossExpression("loss(p, t) = (0.1 + 0.2) * p - t / 3.0")
    p, t = _inputs(np.float32, n=100, seed=3)
    c = np.float32(0.1) + np.float32(0.2)
    assert np.array_equal(ex.host_eval(p, t), c * p - t / np.float32(3.0))
    p, t = p.astype(np.float64), t.astype(np.float64)
    assert np.array_equal(ex.host_eval(p, t), (0.1 + 0.2) * p - t / 3.0)


def test_limits():
    p, t = _inputs(np.float64, n=8, seed=4)
    # a 31-node right-deep chain: accepted
    chain = "p"
    for i in range(15):
        chain = f"{'t' if i % 2 else 'p'} + ({chain})"
    ex = LossExpression(f"loss(p, t) = {chain}")
    assert ex.batch().n_nodes == 31
    np.testing.assert_allclose(ex.host_eval(p, t), 9 * p + 7 * t, rtol=1e-14)

    def perfect(levels):  # a perfect binary tree over abs(p) leaves: levels + 1 live values
        return "abs(p)" if levels == 0 else f"({perfect(levels - 1)} + {perfect(levels - 1)})"

    np.testing.assert_allclose(LossExpression(f"loss(p, t) = {perfect(3)}").host_eval(p, t), 8 * np.abs(p), rtol=1e-14)
    with pytest.raises(_lib.SRError, match="live values") as e:
        LossExpression(f"loss(p, t) = {perfect(4)}").host_eval(p, t)
    assert e.value.code == _lib.SR_ERR_INVALID_ARG
    big = LossExpression("loss(p, t) = " + " + ".join(["p", "t"] * 50 + ["p"]))
    assert big.batch().n_nodes == 201
    with pytest.raises(_lib.SRError, match="nodes") as e:
        big.host_eval(p, t)
    assert e.value.code == _lib.SR_ERR_INVALID_ARG
