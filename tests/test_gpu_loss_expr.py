"""GPU: elementwise losses given as expressions (``Options(elementwise_loss="loss(p, t) = ...")``,
sr_register_loss_expr) through scoring, gradients, constant optimisation and the native search.

An expression-loss call returns the f64 sum of the element values divided once, so the oracle comparisons
use the oracle's f64 accumulation (loss_expr_util.loss_tolerance_f64).  Every test here fails where
``Options`` refuses the string.

Every test here reads a mean over thousands of rows of random trees.  The per-element suites are
test_gpu_loss_expr_forms.py (every instruction form, DX / DY flag and live-value depth of the loss program, bit
for bit per element on all eight tile builds; the tangent widths), test_gpu_loss_expr_ops.py (every operator of the
catalog inside a loss program, per value) and test_gpu_loss_expr_rules.py (every derivative rule through a loss
program against mpmath); their CPU halves are test_loss_expr_forms_host.py and test_loss_expr_rules_host.py.
"""
import ctypes

import numpy as np
import pytest

from loss_expr_util import OPS, RESTATED, data, loss_tolerance_f64
from oracle import Oracle
from parity_util import REL_BAR, assert_losses_within
from sr_amd import (Dataset, Options, SearchOptions, SubDataset, _lib, equation_search, eval_grad_batch, eval_loss_batch,
                    eval_loss_batch_views, eval_tree_array_batch, flatten_trees, gen_random_population,
                    get_context, optimize_constants_batch, parse_expression)

pytestmark = pytest.mark.gpu

LOGCOSH = "loss(p, t) = log(cosh(p - t))"


def _expr(body, **kw):
    return Options(elementwise_loss=f"loss(p, t) = {body}", **{**OPS, **kw})


# ---------------------------------------------------------------- 1. restated catalog losses
@pytest.mark.parametrize("body", list(RESTATED))
def test_restated_catalog_loss_vs_oracle(body):
    """500 trees x 3000 rows, test_gpu_losses.py's inputs: flags bit-equal to the oracle's, incomplete trees
    Inf, every complete tree within the f64-accumulation bar of the oracle's CATALOG loss, Inf exactly where
    the oracle's f64-accumulated loss is."""
    cat = Options(elementwise_loss=RESTATED[body], **OPS)
    opts = _expr(body)
    X, y = data(3000, 1, np.float32, margin=cat.loss_kind >= 9)
    tb = flatten_trees(gen_random_population(500, opts, 4, max_size=20, seed=2), np.float32)
    loss, comp = eval_loss_batch(tb, Dataset(X, y), opts)
    tol, ol, oc, n_wide = loss_tolerance_f64(Oracle.from_options(cat), tb, X, y, loss_kind=cat.loss_kind,
                                             loss_param=cat.loss_param)
    print(f"{body}: complete {int(oc.sum())}, widened {n_wide}")
    assert np.array_equal(comp, oc), np.nonzero(comp != oc)[0][:10]
    assert np.all(np.isinf(loss[~comp]))
    assert n_wide < 0.3 * comp.sum()
    assert_losses_within(loss, ol, comp, tol, body)


# ---------------------------------------------------------------- 2. padding and shapes
ONE = "1.0 + 0.0*p"


def _pop(n_trees, dtype, nf=4, seed=3):
    opts = _expr(ONE)
    return flatten_trees(gen_random_population(n_trees, opts, nf, max_size=20, dtype=dtype, seed=seed), dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 513, 3000, 70_000])
def test_constant_loss_is_exactly_one(n, dtype):
    """Padding rows contribute 0 and every real row exactly 1: the mean is 1.0 bit for bit (70,000 rows:
    several row blocks and the reduce launch)."""
    X, y = data(n, 5, dtype)
    tb = _pop(40 if n == 70_000 else 200, dtype)
    loss, comp = eval_loss_batch(tb, Dataset(X, y), _expr(ONE))
    ref, rc = eval_loss_batch(tb, Dataset(X, y), Options(**OPS))  # the L2 call: the same complete flags
    assert np.array_equal(comp, rc) and comp.sum() > 10
    assert np.all(loss[comp] == dtype(1.0)) and np.all(np.isinf(loss[~comp]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_subdataset_and_views(dtype):
    X, y = data(5000, 6, dtype)
    ds = Dataset(X, y)
    tb = _pop(300, dtype)
    rng = np.random.default_rng(7)
    views = rng.integers(0, 5000, (2, 777))
    tree_view = rng.integers(0, 2, tb.n_trees)
    one, absd = _expr(ONE), _expr("abs(p - t)")
    lv, cv = eval_loss_batch_views(tb, ds, one, tree_view, views)
    assert np.all(lv[cv] == dtype(1.0)) and np.all(np.isinf(lv[~cv])) and cv.sum() > 10
    la, ca = eval_loss_batch_views(tb, ds, absd, tree_view, views)
    for v in range(2):
        sel = np.nonzero(tree_view == v)[0]
        sub = SubDataset(ds, views[v])
        l1, c1 = eval_loss_batch(tb.take(sel), sub, one)
        assert np.array_equal(c1, cv[sel]) and np.all(l1[c1] == dtype(1.0))
        # the expression |p - t| through a SubDataset: the same kernels over the same rows as the view call,
        # and the catalog L1 loss of the same rows within the bar (f64 sum against the in-order fold)
        l2, c2 = eval_loss_batch(tb.take(sel), sub, absd)
        assert np.array_equal(c2, ca[sel])
        assert np.array_equal(l2.view(np.uint8), la[sel].view(np.uint8))
        l3, c3 = eval_loss_batch(tb.take(sel), sub, Options(elementwise_loss="L1DistLoss()", **OPS))
        assert np.array_equal(c3, c2)
        bar = REL_BAR if dtype == np.float32 else 1e-10
        fin = c2 & np.isfinite(l3)
        assert np.all(np.abs(l2[fin].astype(np.float64) - l3[fin]) <= bar * np.abs(l3[fin].astype(np.float64)))


@pytest.mark.parametrize("dtype,knobs", [
    (np.float32, [("rows_per_lane", 4), ("rows_per_lane", 8), ("rows_per_lane", 16), ("rows_per_lane", 32),
                  ("vstk_rows", 16), ("vstk_rows", 32), ("code_cache", 0), ("probe", 0), ("probe", 1)]),
    (np.float64, [("rows_per_lane", 4), ("rows_per_lane", 8), ("vstk_rows", 8), ("probe", 1)]),
])
def test_forced_launch_knobs_map_onto_the_build_set(dtype, knobs):
    """Every rows-per-lane / register-stack / probe knob the plain path accepts at run time (the 8-wave build
    is chosen at context creation only, and takes the same mapping) maps onto the expression
    builds: the same result (the same kernels run), never an error, never another loss."""
    X, y = data(20_000, 8, dtype)
    ds = Dataset(X, y)
    tb = _pop(300, dtype)
    one, absd = _expr(ONE), _expr("abs(p - t)")
    ctx = get_context()
    base, bc = eval_loss_batch(tb, ds, absd)
    defaults = {"rows_per_lane": 0, "vstk_rows": 0, "code_cache": 1, "probe": 2}
    for name, value in knobs:
        ctx.set_tuning(name, value)
        try:
            l1, c1 = eval_loss_batch(tb, ds, one)
            la, ca = eval_loss_batch(tb, ds, absd)
        finally:
            ctx.set_tuning(name, defaults[name])
        assert np.array_equal(c1, bc) and np.all(l1[c1] == dtype(1.0)), (name, value)
        assert np.array_equal(ca, bc), (name, value)
        bar = REL_BAR if dtype == np.float32 else 1e-10
        d = np.abs(la[bc].astype(np.float64) - base[bc].astype(np.float64))
        with np.errstate(invalid="ignore"):
            assert np.all((la[bc] == base[bc]) | (d <= bar * np.abs(base[bc].astype(np.float64)))), (name, value)


# ---------------------------------------------------------------- 3. a loss outside the catalog
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_logcosh_against_numpy_on_device_predictions(dtype):
    X, y = data(3000, 9, dtype)
    ds = Dataset(X, y)
    opts = Options(elementwise_loss=LOGCOSH, **OPS)
    tb = flatten_trees(gen_random_population(300, opts, 4, max_size=20, dtype=dtype, seed=10), dtype)
    loss, comp = eval_loss_batch(tb, ds, opts)
    pred, pc = eval_tree_array_batch(tb, ds, opts)
    assert np.array_equal(comp, pc) and comp.sum() > 50
    with np.errstate(over="ignore", invalid="ignore"):
        elem = np.log(np.cosh(pred[comp] - y[None, :]))  # in the data's dtype
        ref = elem.astype(np.float64).sum(axis=1) / y.size
    got = loss[comp].astype(np.float64)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))
    fin = np.isfinite(ref)
    bar = REL_BAR if dtype == np.float32 else 1e-10
    assert np.all(np.abs(got[fin] - ref[fin]) <= bar * np.abs(ref[fin]))
    assert np.all(got[~fin] == np.inf)  # cosh overflows: the f64 sum of the T values is +Inf


# ---------------------------------------------------------------- 4. weights
def test_weighted_expression_equals_weighted_l1():
    X, y = data(3000, 11, np.float32)
    w = np.random.default_rng(12).uniform(0.5, 2.0, 3000).astype(np.float32)
    opts = Options(elementwise_loss="loss(p, t, w) = w * abs(p - t)", **OPS)
    tb = flatten_trees(gen_random_population(300, opts, 4, max_size=20, seed=13), np.float32)
    loss, comp = eval_loss_batch(tb, Dataset(X, y, weights=w), opts)
    tol, ol, oc, n_wide = loss_tolerance_f64(Oracle.from_options(opts), tb, X, y, w=w, loss_kind=1)
    assert np.array_equal(comp, oc) and n_wide < 0.3 * comp.sum()
    assert_losses_within(loss, ol, comp, tol, "w * abs(p - t)")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_weight_dependent_expression_against_numpy(dtype):
    X, y = data(2500, 14, dtype)
    w = np.random.default_rng(15).uniform(0.5, 2.0, 2500).astype(dtype)
    ds = Dataset(X, y, weights=w)
    opts = Options(elementwise_loss="loss(p, t, w) = abs(p - t) / (1.0 + w)", **OPS)
    tb = flatten_trees(gen_random_population(200, opts, 4, max_size=20, dtype=dtype, seed=16), dtype)
    loss, comp = eval_loss_batch(tb, ds, opts)
    pred, _ = eval_tree_array_batch(tb, ds, opts)
    elem = np.abs(pred[comp] - y[None, :]) / (dtype(1) + w[None, :])  # IEEE operations in T: the device's values
    ref = elem.astype(np.float64).sum(axis=1) / w.astype(np.float64).sum()  # no further multiplication by w
    fin = np.isfinite(ref)
    bar = REL_BAR if dtype == np.float32 else 1e-10
    got = loss[comp].astype(np.float64)
    assert fin.sum() > 30 and np.all(np.abs(got[fin] - ref[fin]) <= bar * np.abs(ref[fin]))


def test_weight_argument_must_match_the_dataset():
    X, y = data(500, 17, np.float32)
    w = np.ones(500, np.float32)
    tb = _pop(10, np.float32)
    with pytest.raises(_lib.SRError, match="weight") as e:
        eval_loss_batch(tb, Dataset(X, y), Options(elementwise_loss="loss(p, t, w) = w * abs(p - t)", **OPS))
    assert e.value.code == _lib.SR_ERR_INVALID_ARG
    with pytest.raises(_lib.SRError, match="weight") as e:
        eval_loss_batch(tb, Dataset(X, y, weights=w), Options(elementwise_loss="loss(p, t) = abs(p - t)", **OPS))
    assert e.value.code == _lib.SR_ERR_INVALID_ARG
    with pytest.raises(_lib.SRError, match="weight"):
        eval_grad_batch(tb, Dataset(X, y, weights=w), Options(elementwise_loss="loss(p, t) = square(p - t)", **OPS))


# ---------------------------------------------------------------- 5. gradients against finite differences
@pytest.mark.parametrize("body", ["-log(4.0) - (p - t) + 2.0*log(1.0 + exp(p - t))", "abs(p - t)^3", "square(1.0 - t*p)",
                                  "exp(-(t*p))", "1.0 - tanh(t*p)"])
def test_restated_gradient_vs_finite_differences(body):
    """test_loss_catalog_gradient_vs_finite_differences's recipe and inputs, the expression's gradient against
    the oracle's finite differences of the catalog loss it restates (the filter depends on the oracle alone)."""
    cat = Options(elementwise_loss=RESTATED[body], binary_operators=["+", "-", "*"], unary_operators=["cos"])
    opts = Options(elementwise_loss=f"loss(p, t) = {body}", binary_operators=["+", "-", "*"], unary_operators=["cos"])
    X, y = data(1500, 7, np.float64, cat.loss_kind >= 9)
    tb = flatten_trees(gen_random_population(200, opts, 4, max_size=15, dtype=np.float64, seed=8), np.float64)
    loss, g, comp = eval_grad_batch(tb, Dataset(X, y), opts)
    g_fd, _, comp_o, fd_err = Oracle.from_options(cat).loss_grad_fd(tb, X, y, loss_kind=cat.loss_kind,
                                                                     loss_param=cat.loss_param, with_error=True)
    assert np.array_equal(comp, comp_o)
    co = tb.constant_offsets()
    checked = 0
    for t in np.nonzero(comp)[0]:
        a, b, e = g[co[t]:co[t + 1]], g_fd[co[t]:co[t + 1]], fd_err[co[t]:co[t + 1]]
        if len(a) == 0:
            continue
        scale = max(1.0, float(np.abs(b).max()))
        if e.max() > 1e-6 * scale:
            continue
        assert np.all(np.abs(a - b) <= 1e-6 * scale), (body, t, a, b)
        checked += 1
    assert checked > 20


# ---------------------------------------------------------------- 6. gradients, closed form
@pytest.mark.parametrize("dtype,bar", [(np.float64, 1e-10), (np.float32, 2e-5)])
@pytest.mark.parametrize("weighted", [False, True])
def test_logcosh_gradient_closed_form(dtype, bar, weighted):
    """log-cosh on c * x1: d loss / d c = mean(tanh(c x1 - y) x1) (weighted: sum(w tanh(.) x1) / sum(w), the
    weight inside the expression); and on a sum of nine such terms (the 16-tangent kernel), each constant's
    entry is that of the sum."""
    rng = np.random.default_rng(18)
    n = 3001
    X = rng.standard_normal((2, n)).astype(dtype)
    y = (0.4 * X[0] + 0.1 * rng.standard_normal(n)).astype(dtype)
    w = rng.uniform(0.5, 2.0, n).astype(dtype) if weighted else None
    spec = "loss(p, t, w) = w * log(cosh(p - t))" if weighted else LOGCOSH
    opts = Options(elementwise_loss=spec, binary_operators=["+", "*"], unary_operators=["cos"])
    cs = [1.5] + [0.1 * (k + 1) for k in range(9)]
    trees = [parse_expression("1.5 * x1", opts),
             parse_expression(" + ".join(f"{c!r} * x1" for c in cs[1:]), opts)]
    tb = flatten_trees(trees, dtype)
    loss, g, comp = eval_grad_batch(tb, Dataset(X, y, weights=w), opts)
    assert comp.all() and len(g) == 10
    x1, y64 = X[0].astype(np.float64), y.astype(np.float64)
    w64 = np.ones(n) if w is None else w.astype(np.float64)
    for c_sum, got in ((float(dtype(1.5)), g[:1]), (float(sum(dtype(c) for c in cs[1:])), g[1:])):
        want = np.sum(w64 * np.tanh(c_sum * x1 - y64) * x1) / w64.sum()
        assert abs(want) > 0.05
        assert np.all(np.abs(got.astype(np.float64) - want) <= bar * abs(want)), (got, want)
    # a forced "grad_rows" maps onto the one build per width: the same bits
    ctx = get_context()
    for rows in (1, 2, 8):
        ctx.set_tuning("grad_rows", rows)
        try:
            l2, g2, _ = eval_grad_batch(tb, Dataset(X, y, weights=w), opts)
        finally:
            ctx.set_tuning("grad_rows", 0)
        assert np.array_equal(g2.view(np.uint8), g.view(np.uint8)) and np.array_equal(l2, loss)


def test_optimize_constants_lowers_logcosh():
    rng = np.random.default_rng(19)
    X = rng.standard_normal((2, 2000)).astype(np.float32)
    y = (0.5 * X[0]).astype(np.float32)
    opts = Options(elementwise_loss=LOGCOSH, binary_operators=["+", "*"], unary_operators=["cos"])
    tb = flatten_trees([parse_expression("3.0 * x1", opts)], np.float32)
    ds = Dataset(X, y)
    start, _ = eval_loss_batch(tb, ds, opts)
    new, losses, improved, _ = optimize_constants_batch(tb, ds, opts, np.random.default_rng(0))
    assert improved[0] and losses[0] < 0.01 * start[0]
    again, _ = eval_loss_batch(new, ds, opts)
    assert again[0] == losses[0]
    assert abs(float(new.get_constants()[0]) - 0.5) < 1e-2


# ---------------------------------------------------------------- 7. native search
def test_native_search_under_logcosh():
    rng = np.random.default_rng(20)
    X = rng.standard_normal((2, 300)).astype(np.float32)
    y = (2 * np.cos(X[1]) + X[0] ** 2 - 2).astype(np.float32)
    opts = Options(elementwise_loss=LOGCOSH, binary_operators=["+", "*", "-"], unary_operators=["cos"], populations=4,
                   population_size=20, ncycles_per_iteration=20, maxsize=15, should_optimize_constants=True,
                   optimizer_probability=0.5)
    fronts = []
    for _ in range(2):
        res = equation_search(X, y, niterations=2, options=opts, seed=7,
                              search_options=SearchOptions(crossover_probability=0.0))
        front = res.pareto_frontier
        assert len(front) >= 2
        loss, comp = eval_loss_batch(flatten_trees([m.tree for m in front], np.float32), Dataset(X, y), opts)
        stored = np.array([m.loss for m in front], dtype=np.float64)
        assert comp.all()
        assert np.all(np.abs(stored - loss) <= REL_BAR * np.abs(loss.astype(np.float64)))
        fronts.append([(m.tree.count_nodes(), float(m.loss), repr(flatten_trees([m.tree], np.float32).val.tolist()))
                       for m in front])
    assert fronts[0] == fronts[1]


# ---------------------------------------------------------------- 8. refusals
def test_restricted_entry_points_refuse_expression_losses():
    from parametric_util import population, to_parametric
    from sr_amd import ParametricExpressionSpec
    from sr_amd.distributed import gpu_partials_packed

    opts = Options(elementwise_loss=LOGCOSH, expression_spec=ParametricExpressionSpec(max_parameters=2), **OPS)
    rng = np.random.default_rng(21)
    X, y = data(400, 22, np.float32)
    cls = rng.integers(1, 4, 400)
    P = rng.standard_normal((2, 3)).astype(np.float32)
    tbp = to_parametric(population(20, opts, 4, 2, seed=23), 4, P)
    dsc = Dataset(X, y, extra={"class": cls})
    for call in (lambda: eval_loss_batch(tbp, dsc, opts), lambda: eval_grad_batch(tbp, dsc, opts),
                 lambda: optimize_constants_batch(tbp, dsc, opts, np.random.default_rng(0))):
        with pytest.raises(_lib.SRError, match="expression loss") as e:
            call()
        assert e.value.code == _lib.SR_ERR_INVALID_ARG
    # the sharded and partials entry points (the C calls themselves: the refusal comes before any collective)
    tb = _pop(10, np.float32)
    ds = Dataset(X, y)
    ctx = get_context()
    plain = Options(elementwise_loss=LOGCOSH, **OPS)
    with pytest.raises(_lib.SRError, match="expression loss"):
        gpu_partials_packed(tb, ds, plain, 400)
    s = tb.to_struct()
    loss, comp = np.empty(10, np.float32), np.empty(10, np.uint8)
    for fn in (_lib.lib.sr_eval_loss_sharded, _lib.lib.sr_eval_loss_tree_sharded):
        rc = fn(ctx.handle, ds.device_handle(ctx), ctx.opset_id(plain.operators), ctypes.byref(s), ctx.loss_code(plain),
                loss.ctypes.data_as(ctypes.c_void_p), comp.ctypes.data_as(ctypes.c_void_p))
        assert rc == _lib.SR_ERR_INVALID_ARG and "expression loss" in _lib.last_error()
    # and the catalog registration keeps rejecting the new kind
    out = ctypes.c_int()
    assert _lib.lib.sr_register_loss(ctx.handle, 19, 0.0, ctypes.byref(out)) == _lib.SR_ERR_INVALID_ARG
