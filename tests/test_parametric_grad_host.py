"""CPU: the scalar vector of ParametricExpression trees (constants, then the parameter matrix column-major:
DynamicExpressions' get_scalar_constants order) in the Python mirror, the new C symbols, and the
stand-alone sanitizer check of the parametric gradient programs and the C packing header.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from sr_amd import Options, ParametricExpression, ParametricExpressionSpec, _lib, flatten_trees, parse_expression
from parametric_util import population, to_parametric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2_OPTS = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "log"])


def test_new_symbols():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sr_eval_grad_batch_parametric", "sr_eval_grad_batch_views_parametric",
                 "sr_optimize_constants_batch_parametric"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert _lib.lib.sr_version() == 2


def test_scalar_packing_order_and_round_trip():
    opts = Options(**C2_OPTS, expression_spec=ParametricExpressionSpec(max_parameters=2))
    t1 = parse_expression("2.5 * p1 + cos(x2 * p2) - 0.5", opts)
    t2 = parse_expression("x1 * x2", opts)
    t3 = parse_expression("p2 / 1.25", opts)
    P = [np.arange(6.0).reshape(2, 3) + 10 * t for t in range(3)]
    tb = flatten_trees([ParametricExpression(t, p) for t, p in zip((t1, t2, t3), P)], np.float64)
    assert tb.constant_offsets().tolist() == [0, 2, 2, 3]
    assert tb.scalar_offsets().tolist() == [0, 8, 14, 21]
    x = tb.get_scalar_constants()
    # constants in pre-order, then parameters[t].T.ravel(): entry (k-1) + K (c-1)
    want = np.concatenate([[2.5, 0.5], P[0].T.ravel(), P[1].T.ravel(), [1.25], P[2].T.ravel()])
    assert x.tolist() == want.tolist()
    assert x[2:8].tolist() == [0.0, 3.0, 1.0, 4.0, 2.0, 5.0]
    back = tb.with_scalar_constants(x)
    assert np.array_equal(back.val, tb.val) and np.array_equal(back.parameters, tb.parameters)
    y = np.arange(21.0) + 100
    moved = tb.with_scalar_constants(y)
    assert moved.get_scalar_constants().tolist() == y.tolist()
    assert moved.get_constants().tolist() == [100.0, 101.0, 114.0]
    assert moved.parameters[0, 1, 2] == 100 + 2 + 1 + 2 * 2  # k = 2, c = 3 of tree 0
    assert np.array_equal(tb.parameters, np.stack(P))  # (the original is untouched)
    consts, mats = tb.split_scalars(y)
    assert consts.tolist() == [100.0, 101.0, 114.0] and mats.shape == (3, 2, 3)
    assert np.array_equal(mats, moved.parameters)
    with pytest.raises(ValueError):
        tb.split_scalars(y[:-1])


def test_scalar_offsets_of_a_plain_batch_are_its_constant_offsets():
    opts = Options(**C2_OPTS)
    ext = population(60, opts, 3, 2, np.float32, seed=3)
    assert np.array_equal(ext.scalar_offsets(), ext.constant_offsets())
    assert np.array_equal(ext.get_scalar_constants(), ext.get_constants())
    c = ext.get_constants() + 1
    assert np.array_equal(ext.with_scalar_constants(c).val, ext.with_constants(c).val)
    consts, mats = ext.split_scalars(c)
    assert mats is None and np.array_equal(consts, c)
    # and a random parametric population round-trips
    par = to_parametric(ext, 3, np.random.default_rng(1).standard_normal((60, 2, 4)))
    x = par.get_scalar_constants()
    assert x.size == par.get_constants().size + 60 * 8 == par.scalar_offsets()[-1]
    back = par.with_scalar_constants(x)
    assert np.array_equal(back.val, par.val) and np.array_equal(back.parameters, par.parameters)


def test_param_grad_check_under_sanitizers():
    """`make param-grad-check`: 2 x 400 random trees — each parametric gradient program equals its plain
    twin's up to the LOAD_FEAT <-> LOAD_PARAM / F <-> P opcodes — and the packing header's pack -> unpack
    and restart draw order, in a stand-alone program built with -fsanitize=address,undefined."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "symbolicregression.jl_amd"), "param-grad-check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "param_grad_check: ok" in r.stdout
