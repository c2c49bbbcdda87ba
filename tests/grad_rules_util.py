"""TEST HELPER: the gradient-rule fixture (tests/golden/grad_rules.json, made by make_grad_rule_fixtures.py)
as Options, datasets and tree batches, shared by test_grad_rules_host.py and test_gpu_grad_rules.py."""
import json
import os
import re

import numpy as np

from sr_amd import Options, ParametricExpression, ParametricExpressionSpec, flatten_trees, parse_expression

HERE = os.path.dirname(os.path.abspath(__file__))
_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        with open(os.path.join(HERE, "golden", "grad_rules.json")) as f:
            _FIXTURE = json.load(f)
    return _FIXTURE


def batches():
    """The fixture's cases by what one eval_grad_batch call can hold: {(group, dataset, loss spec, weighted,
    rows or None): [case, ...]} in fixture order."""
    out = {}
    for c in fixture()["cases"]:
        rows = tuple(c["rows"]) if "rows" in c else None
        out.setdefault((c["group"], c["dataset"], c["loss_spec"], c["weighted"], rows), []).append(c)
    return out


def options(group, loss_spec, parametric=True):
    g = fixture()["groups"][group]
    kw = dict(binary_operators=g["binary"], unary_operators=g["unary"], elementwise_loss=loss_spec)
    if parametric and g["max_parameters"]:
        kw["expression_spec"] = ParametricExpressionSpec(max_parameters=g["max_parameters"])
    return Options(**kw)


def arrays(dataset, options, dtype):
    """(X, y, w, cls) of a fixture dataset in `dtype` (every value is exact in Float32); y is the +-1 target for
    the margin-based losses."""
    d = fixture()["datasets"][dataset]
    conv = lambda v: (np.asarray(v, dtype=np.float64) / d["scale"]).astype(dtype)  # noqa: E731
    y = conv(d["ym"] if options.loss_kind >= 9 else d["y"])
    return conv(d["X"]), y, conv(d["w"]), np.asarray(d["cls"], dtype=np.int32)


def parameters(dtype):
    return np.asarray(fixture()["parameters"], dtype=dtype)


def tree_batch(cases, options, dtype):
    trees = [parse_expression(c["expr"], options) for c in cases]
    if options.expression_spec is not None:
        trees = [ParametricExpression(t, parameters(dtype)) for t in trees]
    return flatten_trees(trees, dtype)


def twin_batch(cases, options, nf, dtype):
    """The plain twins of parametric cases: leaf p_k as feature x_(nf + k) (parametric_util.x_ext's columns)."""
    exprs = [re.sub(r"\bp(\d+)\b", lambda m: f"x{nf + int(m.group(1))}", c["expr"]) for c in cases]
    return flatten_trees([parse_expression(e, options) for e in exprs], dtype)


def sr_ops_header():
    with open(os.path.join(os.path.dirname(HERE), "symbolicregression.jl_amd", "csrc", "sr_ops.h")) as f:
        return f.read()
