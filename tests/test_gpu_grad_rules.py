"""GPU: every derivative rule of the forward-mode gradient kernels against a high-precision reference.

tests/golden/grad_rules.json (make_grad_rule_fixtures.py) holds, per fixed tree, the loss and its gradient
differentiated numerically in mpmath at 60 digits — no hand-written derivative rule on the reference's side —
with an error unit u_T per entry: eps_T times the sum of the absolute row terms of that gradient.  The cases
cover all 32 unary rules (sr_unary_deriv), the 16 binary operators in every operand position the gradient
compiler emits, plain and with a parameter operand (sr_binary_partials through the BASIC forms and the general
tangent form), all 19 catalog losses unweighted and weighted (sr_elem_loss_deriv), the second tangent window
and the constants beyond the 64th; test_grad_rules_host.py shows on the CPU that the programs hold those
opcodes and that the references agree with the oracle's finite differences.

Per case and precision: complete, the loss within the parity bar, every gradient entry within K_T u_T, and
exact zeros exactly zero.  No case is skipped and none is filtered.
"""
import numpy as np
import pytest

import sr_amd
from grad_rules_util import arrays, batches, fixture, options, tree_batch
from parity_util import REL_BAR
from sr_amd import (Dataset, Options, ParametricExpression, ParametricExpressionSpec, SubDataset, UnsupportedOperatorError,
                    _lib, eval_grad_batch, flatten_trees, optimize_constants_batch, parse_expression)

pytestmark = pytest.mark.gpu

DTYPES = {"float64": np.float64, "float32": np.float32}
# the loss bars of the parity tests: 1e-4 relative in Float32 (parity_util.REL_BAR), 1e-10 in Float64
# (test_gpu_losses.py's Float64 bar)
LOSS_BAR = {"float64": 1e-10, "float32": REL_BAR}
# |g - ref| <= K_T u_T.  K_T: the largest |g - ref| / u_T measured on the MI355X over all cases, times 4, rounded
# up to a power of two (the margin: libm differences between ROCm releases and the few-ulp spread of the OCML
# functions behind the non-BASIC operators).  A wrong rule is off by ~1 / eps_T units.
# Measured (ROCm 7.2, gfx950), 271 cases: Float64 1.348 (param/pow/PP; then unary/log2 1.279, unary/log10 1.254),
# Float32 1.359 (param/div/PP; then param/atan2/PP 1.273) -> 4 x 1.36 = 5.4 -> 8 for both.
K_T = {"float64": 8.0, "float32": 8.0}
CASES = [c["name"] for c in fixture()["cases"]]


def _dataset(key, opts, dtype):
    group, dataset, spec, weighted, rows = key
    X, y, w, cls = arrays(dataset, opts, dtype)
    kw = dict(weights=w) if weighted else {}
    if opts.expression_spec is not None:
        kw.update(extra={"class": cls}, n_classes=3)
    ds = Dataset(X, y, **kw)
    return ds if rows is None else SubDataset(ds, np.asarray(rows, dtype=np.int64))


def _run(key, cases, dtype):
    opts = options(key[0], key[2])
    tb = tree_batch(cases, opts, dtype)
    loss, g, comp = eval_grad_batch(tb, _dataset(key, opts, dtype), opts)
    so = tb.scalar_offsets()
    assert g.dtype == dtype and g.shape == (int(so[-1]),)
    return loss, g, comp, so


def device_results():
    """{(case name, dtype name): (loss, gradient, complete)}: one eval_grad_batch call per (operator set, loss,
    dataset, weights, row view) and precision."""
    out = {}
    for key, cases in batches().items():
        for dname, dtype in DTYPES.items():
            loss, g, comp, so = _run(key, cases, dtype)
            for k, c in enumerate(cases):
                out[c["name"], dname] = (float(loss[k]), g[so[k]:so[k + 1]].astype(np.float64), bool(comp[k]))
    return out


@pytest.fixture(scope="module")
def results():
    return device_results()


def ratios(case, dname, results):
    """|g - ref| / u_T per entry with u_T > 0 (the figure K_T bounds)."""
    _, g, _ = results[case["name"], dname]
    u = np.asarray(case["u32" if dname == "float32" else "u64"])
    ref = np.asarray(case["grad"])
    nz = u > 0
    return np.abs(g[nz] - ref[nz]) / u[nz]


def _check(case, dname, results):
    loss, g, comp = results[case["name"], dname]
    assert comp, case["name"]
    assert abs(loss - case["loss"]) <= LOSS_BAR[dname] * abs(case["loss"]), (case["name"], loss, case["loss"])
    ref, zero = np.asarray(case["grad"]), np.asarray(case["zero"], dtype=bool)
    assert g.shape == ref.shape
    assert np.all(g[zero] == 0), (case["name"], "exact zeros", g, zero)
    r = ratios(case, dname, results)
    print(f"{case['name']} {dname}: max |g - ref| / u = {r.max(initial=0.0):.3g}")
    assert np.all(r <= K_T[dname]), (case["name"], case["expr"], g, ref, r)  # (a NaN fails too)
    return 1


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", CASES)
def test_gradient_matches_the_high_precision_reference(name, dname, results):
    _check(next(c for c in fixture()["cases"] if c["name"] == name), dname, results)


def test_no_case_is_skipped(results):
    cases = fixture()["cases"]
    assert CASES == [c["name"] for c in cases] and len(results) == 2 * len(cases)
    n = sum(_check(c, dname, results) for c in cases for dname in DTYPES)
    assert n == 2 * len(cases)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("group", ["binary", "param"])
def test_general_path_gradients_independent_of_rows_per_lane(group, dname):
    """The rows-per-lane tuning must not change a bit of the general tangent form's results either: the
    group holds atan2, mod, min, cond and the comparisons in every operand position, plain and with a
    parameter operand (test_gpu_grad.py's tuning test has none of them, and no parametric tree)."""
    key, cases = max(((k, v) for k, v in batches().items() if k[0] == group), key=lambda kv: len(kv[1]))
    assert len(cases) >= 48
    ctx = sr_amd.get_context()
    try:
        ref = _run(key, cases, DTYPES[dname])
        assert ref[2].all()
        for rows in (1, 2, 8):
            ctx.set_tuning("grad_rows", rows)
            loss, g, comp, _ = _run(key, cases, DTYPES[dname])
            assert np.array_equal(comp, ref[2]) and np.array_equal(_bits(loss), _bits(ref[0])), rows
            assert np.array_equal(_bits(g), _bits(ref[1])), (group, rows)
    finally:
        ctx.set_tuning("grad_rows", 0)


@pytest.mark.parametrize("parametric", [False, True])
def test_operator_without_a_rule_is_refused(parametric):
    """gamma has no derivative rule: the gradient entry points refuse an operator set that holds it."""
    kw = dict(expression_spec=ParametricExpressionSpec(max_parameters=1)) if parametric else {}
    opts = Options(binary_operators=["+", "*"], unary_operators=["cos", "gamma"], **kw)
    X, y, _, cls = arrays("pos", opts, np.float64)
    tree = parse_expression("cos(x1 * p1) + 0.5" if parametric else "cos(x1 * 1.5) + 0.5", opts)
    if parametric:
        tree = ParametricExpression(tree, np.array([[1.5, 0.75, 1.25]]))
    tb = flatten_trees([tree], np.float64)
    ds = Dataset(X, y, **(dict(extra={"class": cls}, n_classes=3) if parametric else {}))
    for call in (lambda: eval_grad_batch(tb, ds, opts),
                 lambda: optimize_constants_batch(tb, ds, opts, np.random.default_rng(0))):
        with pytest.raises(UnsupportedOperatorError) as e:
            call()
        assert e.value.code == _lib.SR_ERR_UNSUPPORTED_OP
