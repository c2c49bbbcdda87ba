"""CPU: tests/golden/loss_expr_rules.json (make_loss_expr_fixtures.py: mpmath at 60 digits, no derivative rule)
against the library's host interpreter, before any GPU run.

Per case the predictions of the tree {0} * x1 + {1} * x2 + {2} are formed in numpy, ``host_eval(deriv=True)`` gives L
and dL/dp per row (forward mode with the rules of csrc/sr_ops.h, the interpreter the kernels run), and the chain
rule through (x1, x2, 1) the gradient: both must reproduce the fixture's loss and gradient within the bars of
test_gpu_loss_expr_rules.py (K loss units, K_T gradient units), in both dtypes.  Also: the fixture covers every
operator with a rule in every operand position (gamma, the one operator without a rule, is the GPU test's).
"""
import json
import os

import numpy as np
import pytest

from grad_rules_util import fixture as grad_fixture
from sr_amd import LossExpression

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = {"float64": np.float64, "float32": np.float32}
# the GPU test's bars (measured there on the MI355X; repeated here so that this file needs no GPU test module)
K_T = 8.0
K_L = 4.0
_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        with open(os.path.join(HERE, "golden", "loss_expr_rules.json")) as f:
            _FIXTURE = json.load(f)
    return _FIXTURE


def data(dtype):
    """(X, y, w) of the fixture's dataset (grad_rules.json's "normal"; every value exact in Float32)."""
    d = grad_fixture()["datasets"][fixture()["dataset"]]
    conv = lambda v: (np.asarray(v, dtype=np.float64) / d["scale"]).astype(dtype)  # noqa: E731
    return conv(d["X"]), conv(d["y"]), conv(d["w"])


def host_loss_and_gradient(case, dtype):
    X, y, w = data(dtype)
    c = [dtype(v) for v in case["constants"]]
    pred = (c[0] * X[0] + c[1] * X[1]) + c[2]  # the tree's own order, in T
    ex = LossExpression(case["loss_spec"])
    L, dL = ex.host_eval(pred, y, w if case["weighted"] else None, deriv=True)
    denom = float(np.sum(w.astype(np.float64))) if case["weighted"] else float(len(y))
    L, dL = L.astype(np.float64), dL.astype(np.float64)
    g = [float(np.sum(dL * f)) / denom for f in (X[0].astype(np.float64), X[1].astype(np.float64), np.ones(len(y)))]
    return float(np.sum(L)) / denom, np.array(g)


def ratios(case, dname, loss, g):
    """(|loss - ref| / loss unit, max |g - ref| / u_T over the entries with a unit)."""
    s = "32" if dname == "float32" else "64"
    u = np.asarray(case["u" + s])
    nz = u > 0
    r = np.abs(np.asarray(g, dtype=np.float64)[nz] - np.asarray(case["grad"])[nz]) / u[nz]
    return abs(float(loss) - case["loss"]) / case["lu" + s], float(r.max(initial=0.0))


@pytest.mark.parametrize("dname", list(DTYPES))
def test_host_interpreter_reproduces_the_fixture(dname):
    worst = []
    for case in fixture()["cases"]:
        loss, g = host_loss_and_gradient(case, DTYPES[dname])
        rl, rg = ratios(case, dname, loss, g)
        worst.append((rg, rl, case["name"]))
        zero = np.asarray(case["zero"], dtype=bool)
        assert np.all(g[zero] == 0), (case["name"], g)
        assert rl <= K_L, (case["name"], case["body"], loss, case["loss"], rl)
        assert rg <= K_T, (case["name"], case["body"], g, case["grad"], rg)
    print(dname, "worst gradient ratios:", sorted(worst, reverse=True)[:3], "worst loss ratio:", max(w[1] for w in worst))
    assert len(worst) == 80


def test_fixture_covers_every_rule():
    """32 unary operators with a rule (the catalog without gamma) and 16 binary ones in three operand positions; w is
    the independent operand of the `first` and `second` bodies, which are therefore the three-argument form."""
    from op_values_util import BINARY, UNARY

    alias = {">": "greater", "<": "less", ">=": "greater_equal", "<=": "less_equal", "+": "add", "-": "sub", "*": "mul",
             "/": "div", "^": "pow"}
    cases = fixture()["cases"]
    names = [c["name"] for c in cases]
    assert len(names) == len(set(names)) == 32 + 3 * 16
    assert {n.split("/")[1] for n in names if n.startswith("unary/")} == set(UNARY) - {"gamma"}
    assert sorted(n for n in names if n.startswith("binary/")) == sorted(
        f"binary/{alias.get(b, b)}/{tag}" for b in BINARY for tag in ("first", "second", "both"))
    for c in cases:
        assert c["weighted"] == c["name"].endswith(("/first", "/second")) == ("w" in c["loss_spec"].split("=")[0]), c["name"]
        assert c["weighted"] == (LossExpression(c["loss_spec"]).n_args == 3)
        assert c["lu64"] > 0 and all(u > 0 for u in c["u64"]) and not any(c["zero"]), c["name"]
        assert all(float(np.float32(v)) == v for v in c["constants"]), c["name"]
