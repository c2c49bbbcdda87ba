"""GPU: gradients and constant optimisation of ParametricExpression trees (sr_eval_grad_batch_parametric,
sr_eval_grad_batch_views_parametric, sr_optimize_constants_batch_parametric; sr_grad_inst.hip).

Tree t's gradient is [its constants in pre-order | K x C parameter entries, column-major] (DynamicExpressions'
get_scalar_constants order).  A parametric tree's plain twin is the same tree with p_k as feature nf + k on
x_ext(X, P, cls) (parametric_util): the constants' entries equal the twin's bit for bit, the parameters'
entries are checked against closed forms and central differences of the CPU oracle's Float64 loss.
"""
import ctypes

import numpy as np
import pytest

import sr_amd
from oracle import Oracle
from sr_amd import (Dataset, Options, ParametricExpression, ParametricExpressionSpec, SubDataset, _lib, eval_grad_batch,
                    eval_grad_batch_views, eval_loss_batch, flatten_trees, optimize_constants_batch, parse_expression)
from parametric_grad_util import param_grad_fd, uses_parameter
from parametric_util import data, population, to_parametric, x_ext

pytestmark = pytest.mark.gpu

OPS4 = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "log", "sin"])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _pds(X, y, cls, n_classes, **kw):
    return Dataset(X, y, extra={"class": cls}, n_classes=n_classes, **kw)


def _popts(K, **kw):
    return Options(**{**OPS4, **kw}, expression_spec=ParametricExpressionSpec(max_parameters=K))


def _one(expr, opts, P, dtype):
    return flatten_trees([ParametricExpression(parse_expression(expr, opts), np.asarray(P, dtype=dtype))], dtype)


# ------------------------------------------------------------------ 3. closed forms
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-12), (np.float32, 2e-5)])
def test_known_answer_x1_times_p1(dtype, tol):
    """x1 * p1, K = 2, C = 3: d L / d P[1, c] = (1/n) sum_{class = c} 2 (x1 P[1, c] - y) x1; p2 is unused:
    exactly 0.  On a SubDataset whose rows omit class 3 that column is exactly 0 too."""
    opts = _popts(2)
    X, y, cls = data(1000, 3, 3, dtype=dtype, seed=4)
    P = np.array([[1.5, -0.75, 0.25], [9.0, 8.0, 7.0]], dtype=dtype)
    tb = _one("x1 * p1", opts, P, dtype)
    ds = _pds(X, y, cls, 3)
    x1, yy, P64 = X[0].astype(np.float64), y.astype(np.float64), P.astype(np.float64)

    def ref_for(rows):
        r = np.zeros((2, 3))
        for c in range(3):
            m = rows[cls[rows] == c + 1]
            r[0, c] = np.sum(2 * (x1[m] * P64[0, c] - yy[m]) * x1[m]) / len(rows)
        return r

    loss, g, comp = eval_grad_batch(tb, ds, opts)
    assert comp[0] and g.shape == (6,) and g.dtype == dtype
    gc, gp = tb.split_scalars(g)
    ref = ref_for(np.arange(1000))
    assert gc.size == 0 and gp.shape == (1, 2, 3)
    assert np.all(np.abs(gp[0, 0] - ref[0]) <= tol * np.maximum(1.0, np.abs(ref[0]))), (gp, ref)
    assert np.all(gp[0, 1] == 0)
    l0, c0 = eval_loss_batch(tb, ds, opts)
    assert _bits(loss)[0] == _bits(l0)[0] and c0[0]
    rows = np.nonzero(cls != 3)[0][::2].astype(np.int64)
    loss, g, comp = eval_grad_batch(tb, SubDataset(ds, rows), opts)
    gp = tb.split_scalars(g)[1]
    ref = ref_for(rows)
    assert comp[0] and np.all(np.abs(gp[0, 0, :2] - ref[0, :2]) <= tol * np.maximum(1.0, np.abs(ref[0, :2])))
    assert np.all(gp[0, 1] == 0) and gp[0, 0, 2] == 0 and np.all(ref[0, :2] != 0)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-12), (np.float32, 2e-5)])
def test_known_answer_mixed_tree(dtype, tol):
    """2.1 * p1 + cos(x2 * p2) - 0.5: both constants and all six parameter entries against the closed form."""
    opts = _popts(2)
    X, y, cls = data(1000, 3, 3, dtype=dtype, seed=5)
    P = np.array([[1.5, -0.75, 0.25], [0.5, 1.25, -2.0]], dtype=dtype)
    tb = _one("2.1 * p1 + cos(x2 * p2) - 0.5", opts, P, dtype)
    loss, g, comp = eval_grad_batch(tb, _pds(X, y, cls, 3), opts)
    x2, yy, P64, ci = X[1].astype(np.float64), y.astype(np.float64), P.astype(np.float64), cls - 1
    c1 = float(dtype(2.1))
    p1, p2 = P64[0, ci], P64[1, ci]
    d = 2 * (c1 * p1 + np.cos(x2 * p2) - 0.5 - yy) / 1000
    ref_c = np.array([np.sum(d * p1), np.sum(-d)])
    ref_p = np.zeros((2, 3))
    for c in range(3):
        m = ci == c
        ref_p[0, c] = np.sum(d[m] * c1)
        ref_p[1, c] = np.sum(d[m] * -np.sin(x2[m] * p2[m]) * x2[m])
    gc, gp = tb.split_scalars(g)
    assert comp[0] and gc.shape == (2,)
    assert np.all(np.abs(gc - ref_c) <= tol * np.maximum(1.0, np.abs(ref_c))), (gc, ref_c)
    assert np.all(np.abs(gp[0] - ref_p) <= tol * np.maximum(1.0, np.abs(ref_p))), (gp[0], ref_p)


# ------------------------------------------------------------------ 4. a population against the CPU oracle
@pytest.fixture(scope="module")
def pop64():
    opts = Options(**OPS4)
    X, y, cls = data(1500, 3, 3, np.float64, seed=2)
    ext = population(400, opts, 3, 2, np.float64, seed=5)
    P = np.random.default_rng(8).standard_normal((2, 3))
    par = to_parametric(ext, 3, P)
    g_fd, fd_err = param_grad_fd(Oracle.from_options(opts), ext, X, y, cls, P)
    return opts, X, y, cls, ext, P, par, g_fd, fd_err


def test_population_parameters_vs_oracle_finite_differences(pop64):
    opts, X, y, cls, ext, P, par, g_fd, fd_err = pop64
    loss, g, comp = eval_grad_batch(par, _pds(X, y, cls, 3), opts)
    l0, c0 = eval_loss_batch(par, _pds(X, y, cls, 3), opts)
    assert np.array_equal(comp, c0) and np.array_equal(_bits(loss), _bits(l0))
    gp = par.split_scalars(g)[1]
    so = par.scalar_offsets()
    cand = np.nonzero(comp & uses_parameter(par))[0]
    checked = left_out = 0
    worst = 0.0
    for t in cand:
        scale = max(1.0, float(np.abs(g_fd[t]).max()))
        if not fd_err[t].max() <= 1e-6 * scale:
            left_out += 1
            continue
        dev = float(np.abs(gp[t] - g_fd[t]).max()) / scale
        worst = max(worst, dev)
        assert dev <= 1e-6, (t, gp[t], g_fd[t])
        checked += 1
    print(f"{len(cand)} complete trees with parameter leaves, {checked} checked, {left_out} left out, "
          f"largest deviation {worst:.2e} x scale")
    assert checked >= 60 and left_out <= 0.25 * len(cand), (checked, left_out, len(cand))
    for t in np.nonzero(~comp)[0]:  # incomplete: L(Inf) and an all-zero gradient
        assert np.isinf(loss[t]) and np.all(g[so[t]:so[t + 1]] == 0)
    for t in np.nonzero(~uses_parameter(par))[0]:  # no parameter leaf: every parameter entry exactly 0
        assert np.all(gp[t] == 0)


def test_population_constants_equal_the_plain_twin_bit_for_bit(pop64):
    opts, X, y, cls, ext, P, par, _, _ = pop64
    loss, g, comp = eval_grad_batch(par, _pds(X, y, cls, 3), opts)
    twin = Dataset(x_ext(X, P, cls), y)
    lt, gt, ct = eval_grad_batch(ext, twin, opts)
    twin.free_device()
    gc = par.split_scalars(g)[0]
    assert np.array_equal(comp, ct) and comp.sum() > 100 and gc.size == gt.size > 200
    assert np.array_equal(_bits(gc), _bits(gt))


# ------------------------------------------------------------------ 5. Float32 against Float64
def test_population_f32_close_to_f64():
    opts = Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    X32, y32, cls = data(4096, 3, 3, np.float32, seed=3)
    ext = population(300, opts, 3, 2, np.float32, seed=6)
    P = np.random.default_rng(8).standard_normal((2, 3)).astype(np.float32)
    par = to_parametric(ext, 3, P)
    l32, g32, c32 = eval_grad_batch(par, _pds(X32, y32, cls, 3), opts)
    l64, g64, c64 = eval_grad_batch(par.astype(np.float64), _pds(X32.astype(np.float64), y32.astype(np.float64), cls, 3),
                                    opts)
    so = par.scalar_offsets()
    checked = bad = 0
    for t in np.nonzero(c32 & c64)[0]:
        a, b = g32[so[t]:so[t + 1]].astype(np.float64), g64[so[t]:so[t + 1]]
        if not np.any(b != 0) or not abs(float(l32[t]) - l64[t]) <= 1e-5 * abs(l64[t]):
            continue
        checked += 1
        scale = max(1.0, float(np.abs(b).max()))
        bad += int(not np.all(np.abs(a - b) <= 1e-2 * scale))
    print(f"{checked} trees checked, {bad} beyond 1e-2 x scale")
    assert checked > 100 and bad <= 0.04 * checked, (checked, bad)


def test_both_binning_schemes_agree():
    """Float32 with slots x classes <= 16 bins per lane (one accumulator per lane, slot and class, summed once
    per row block); tuning "grad_lane_bins" 0 runs the masked wave sums per 64-row group instead, which is what
    Float64 and larger shapes always run.  The two add the same f64 products in different orders: Float32
    results agree to rounding, exact zeros stay exact, and Float64 does not read the knob."""
    opts = Options(**OPS4)
    X32, y32, cls = data(4096, 3, 3, np.float32, seed=3)
    ext = population(300, opts, 3, 2, np.float32, seed=6)
    par = to_parametric(ext, 3, np.random.default_rng(8).standard_normal((2, 3)).astype(np.float32))
    ctx = sr_amd.get_context()
    for dtype in (np.float32, np.float64):
        tb, ds = par.astype(dtype), _pds(X32.astype(dtype), y32.astype(dtype), cls, 3)
        try:
            a = eval_grad_batch(tb, ds, opts)
            ctx.set_tuning("grad_lane_bins", 0)
            b = eval_grad_batch(tb, ds, opts)
        finally:
            ctx.set_tuning("grad_lane_bins", 1)
        assert np.array_equal(a[2], b[2]) and np.array_equal(_bits(a[0]), _bits(b[0])) and a[2].sum() > 100
        if dtype == np.float64:
            assert np.array_equal(_bits(a[1]), _bits(b[1]))
            continue
        ga, gb = a[1].astype(np.float64), b[1].astype(np.float64)
        assert np.array_equal(np.isfinite(ga), np.isfinite(gb)) and np.array_equal(ga == 0, gb == 0)
        # Each entry is ONE f64 sum of <= 4,096 products, rounded to Float32 once.  Two summation orders differ
        # by at most 4096 x 2^-53 x sum|terms| = 4.5e-13 x sum|terms|; against the tree's largest entry that
        # stays under 1e-5 unless the terms cancel by more than seven digits, on top of the one Float32 ulp
        # (6e-8) the final rounding can add.
        so = tb.scalar_offsets()
        for t in np.nonzero(a[2])[0]:
            x, z = ga[so[t]:so[t + 1]], gb[so[t]:so[t + 1]]
            fin = np.isfinite(z)
            if fin.any():
                assert np.all(np.abs(x[fin] - z[fin]) <= 1e-5 * max(1.0, float(np.abs(z[fin]).max()))), t


# ------------------------------------------------------------------ 6. edges
EDGE_TREES = ("x1 * p1 + 0.5", "cos(x2 * p2) * 1.5 + p1", "(p1 - x1) / (p2 * p2 + 2.0)")


def _check_against_references(par, ext, X, y, cls, P, opts, loss_g_comp, w=None, loss_kind=0, tol=1e-6):
    """Constants against finite differences of the twin, parameters against finite differences in P."""
    loss, g, comp = loss_g_comp
    orc = Oracle.from_options(opts)
    Xe = x_ext(X, P, cls)
    gc_fd, lo, co = orc.loss_grad_fd(ext, Xe, y, w, loss_kind=loss_kind)
    gp_fd, _ = param_grad_fd(orc, ext, X, y, cls, P, w, loss_kind)
    assert np.array_equal(comp, co) and comp.all()
    np.testing.assert_allclose(loss, lo, rtol=1e-12)
    gc, gp = par.split_scalars(g)
    sc = max(1.0, float(np.abs(gc_fd).max(initial=0)))
    assert np.all(np.abs(gc - gc_fd) <= tol * sc), (gc, gc_fd)
    sp = max(1.0, float(np.abs(gp_fd).max()))
    assert np.all(np.abs(gp - gp_fd) <= tol * sp), (gp, gp_fd)
    return gp


def _edge_batch(exprs, K, C, dtype=np.float64, seed=8, **kw):
    opts = _popts(K, **kw)
    P = np.random.default_rng(seed).uniform(0.5, 1.5, (K, C)).astype(dtype)
    trees = [parse_expression(e, opts) for e in exprs]
    par = flatten_trees([ParametricExpression(t, P) for t in trees], dtype)
    # the plain twins: p_k -> x_(3 + k)
    ext = flatten_trees([parse_expression(_twin_text(e, 3), Options(**{**OPS4, **kw})) for e in exprs], dtype)
    return opts, P, par, ext


def _twin_text(expr, nf):
    import re

    return re.sub(r"\bp(\d+)\b", lambda m: f"x{nf + int(m.group(1))}", expr)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 513, 1025])
def test_row_counts_across_tile_and_block_boundaries(n):
    opts, P, par, ext = _edge_batch(EDGE_TREES, 2, 3)
    X, y, cls = data(n, 3, 3, np.float64, seed=n)
    _check_against_references(par, ext, X, y, cls, P, opts, eval_grad_batch(par, _pds(X, y, cls, 3), opts))


@pytest.mark.parametrize("C", [1, 65])
def test_one_class_and_sixty_five_classes(C):
    opts, P, par, ext = _edge_batch(("x1 * p1 + 1.0", "cos(p1 * x2)"), 1, C)
    X, y, cls = data(1000, 3, C, np.float64, seed=C)
    gp = _check_against_references(par, ext, X, y, cls, P, opts, eval_grad_batch(par, _pds(X, y, cls, C), opts))
    assert gp.shape == (2, 1, C) and np.all(gp[0] != 0)


def test_window_straddles_constants_and_parameters():
    """15 constants, then p1 and p2: the first 16-tangent window holds the constants and p1, the second p2;
    and a tree with more than 16 constants plus parameters."""
    body15 = " + ".join(f"{0.1 * (k + 1)} * cos(x{1 + k % 3} + {0.05 * (k + 1)})" for k in range(7)) + " + 0.3"
    body20 = " + ".join(f"{0.1 * (k + 1)} * cos(x{1 + k % 3} + {0.05 * (k + 1)})" for k in range(10))
    exprs = (f"({body15}) + (p1 * x1 + p2)", f"({body20}) + (p2 * x2 + cos(p1))")
    opts, P, par, ext = _edge_batch(exprs, 2, 3)
    assert np.diff(par.constant_offsets()).tolist() == [15, 20]
    X, y, cls = data(700, 3, 3, np.float64, seed=21)
    _check_against_references(par, ext, X, y, cls, P, opts, eval_grad_batch(par, _pds(X, y, cls, 3), opts))


def test_forty_parameters_one_used():
    opts = _popts(40)
    K, C = 40, 3
    P = np.random.default_rng(3).uniform(0.5, 1.5, (K, C))
    par = _one("x1 * p40 + 0.5", opts, P, np.float64)
    X, y, cls = data(600, 3, C, np.float64, seed=22)
    loss, g, comp = eval_grad_batch(par, _pds(X, y, cls, C), opts)
    gc, gp = par.split_scalars(g)
    x1, p = X[0], P[39, cls - 1]
    d = 2 * (x1 * p + 0.5 - y) / 600
    ref = np.array([np.sum(d[cls == c + 1] * x1[cls == c + 1]) for c in range(C)])
    assert comp[0] and g.shape == (1 + K * C,) and np.all(gp[0, :39] == 0)
    np.testing.assert_allclose(gp[0, 39], ref, rtol=1e-12)
    np.testing.assert_allclose(gc, [np.sum(d)], rtol=1e-12, atol=1e-15)


def test_weights_subdataset_l1():
    opts, P, par, ext = _edge_batch(EDGE_TREES + ("0.7 * cos(x1 + 0.2) + p2 * x3",), 2, 3,
                                    elementwise_loss="L1DistLoss")
    X, y, cls = data(1000, 3, 3, np.float64, seed=23)
    w = np.random.default_rng(9).uniform(0.5, 2.0, 1000)
    idx = np.random.default_rng(10).integers(0, 1000, 300)
    res = eval_grad_batch(par, SubDataset(_pds(X, y, cls, 3, weights=w), idx), opts)
    _check_against_references(par, ext, X[:, idx], y[idx], cls[idx], P, opts, res, w=w[idx], loss_kind=1, tol=1e-5)


def test_two_row_views_with_different_class_mixes():
    opts, P, par, ext = _edge_batch(EDGE_TREES + EDGE_TREES[:1], 2, 3)
    X, y, cls = data(2000, 3, 3, np.float64, seed=24)
    ds = _pds(X, y, cls, 3)
    v0 = np.nonzero(cls != 1)[0][:400]   # classes 2 and 3 only
    v1 = np.nonzero(cls != 3)[0][-400:]  # classes 1 and 2 only
    views = np.stack([v0, v1]).astype(np.int64)
    tv = np.array([0, 1, 1, 1], dtype=np.int32)
    loss, g, comp = eval_grad_batch_views(par, ds, opts, tv, views)
    so = par.scalar_offsets()
    for t in range(4):
        l1, g1, c1 = eval_grad_batch(par.take([t]), SubDataset(ds, views[tv[t]]), opts)
        assert c1[0] == comp[t] and _bits(l1)[0] == _bits(loss[t:t + 1])[0]
        assert np.array_equal(_bits(g1), _bits(g[so[t]:so[t + 1]])), t
    gp = par.split_scalars(g)[1]
    assert np.all(gp[0, :, 0] == 0) and np.all(gp[3, :, 2] == 0) and gp[0, 0, 1] != 0 and gp[3, 0, 0] != 0
    sub = par.take([0])
    _check_against_references(sub, ext.take([0]), X[:, v0], y[v0], cls[v0], P, opts,
                              eval_grad_batch(sub, SubDataset(ds, v0), opts))


# ------------------------------------------------------------------ 7. reproducibility
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bit_reproducible_whatever_the_launch(dtype):
    """Two identical calls, every rows-per-lane choice, both work-item orders, and every tree scored alone: the
    same bits, under either binning scheme (per-lane class accumulators summed once per row block, or
    fixed-tree wave sums per 64-row group in row order: no atomics, nothing that depends on the rows per lane
    or on the other trees of the call)."""
    opts = Options(**OPS4)
    n = 30_001
    X, y, cls = data(n, 3, 4, dtype, seed=31)
    w = (0.5 + np.random.default_rng(32).random(n)).astype(dtype)
    ext = population(300, opts, 3, 3, dtype, seed=33, max_size=25)
    P = np.random.default_rng(34).uniform(0.5, 1.5, (3, 4)).astype(dtype)
    par = to_parametric(ext, 3, P)
    ds = _pds(X, y, cls, 4, weights=w)
    ctx = sr_amd.get_context()
    for lane_bins in (1, 0):  # (Float64 does not read the knob: every tree, then a sample once more)
        try:
            ctx.set_tuning("grad_lane_bins", lane_bins)
            _reproducible(ctx, par, ds, opts, every=1 if lane_bins else 7)
        finally:
            ctx.set_tuning("grad_lane_bins", 1)


def _reproducible(ctx, par, ds, opts, every):
    ref = eval_grad_batch(par, ds, opts)
    assert ref[2].mean() > 0.2 and np.count_nonzero(par.split_scalars(ref[1])[1]) > 300
    same = lambda r, what: (np.array_equal(r[2], ref[2]) and np.array_equal(_bits(r[0]), _bits(ref[0]))  # noqa: E731
                            and np.array_equal(_bits(r[1]), _bits(ref[1]))) or pytest.fail(str(what))
    same(eval_grad_batch(par, ds, opts), "second call")
    try:
        for rows in (1, 2, 4, 8):
            ctx.set_tuning("grad_rows", rows)
            same(eval_grad_batch(par, ds, opts), ("grad_rows", rows))
        ctx.set_tuning("grad_rows", 0)
        ctx.set_tuning("grad_sort", 0)
        same(eval_grad_batch(par, ds, opts), "grad_sort 0")
    finally:
        ctx.set_tuning("grad_rows", 0)
        ctx.set_tuning("grad_sort", 1)
    so = par.scalar_offsets()
    for t in range(0, 300, every):  # (every tree under the default scheme, a sample under the other)
        l1, g1, c1 = eval_grad_batch(par.take([t]), ds, opts)
        assert c1[0] == ref[2][t] and np.array_equal(_bits(g1), _bits(ref[1][so[t]:so[t + 1]])), t


# ------------------------------------------------------------------ 8. the optimiser
def _recovery_problem():
    rng = np.random.default_rng(11)
    X = rng.standard_normal((3, 2000))
    cls = rng.integers(1, 4, 2000).astype(np.int32)
    a = np.array([3.0, -1.5, 0.5])
    y = a[cls - 1] * X[0] + 1.5
    return X, y, cls, a


def test_optimiser_recovers_parameters_and_constant():
    opts = _popts(2, unary_operators=["cos", "exp"])
    X, y, cls, a = _recovery_problem()
    ds = _pds(X, y, cls, 3)
    tb = _one("p1 * x1 + 1.0", opts, np.ones((2, 3)), np.float64)
    new_tb, losses, improved, n_evals = optimize_constants_batch(tb, ds, opts, np.random.default_rng(0))
    assert improved[0] and new_tb.parametric
    np.testing.assert_allclose(new_tb.parameters[0, 0], a, rtol=1e-6)
    np.testing.assert_allclose(new_tb.get_constants(), [1.5], rtol=1e-6)
    l1, c1 = eval_loss_batch(new_tb, ds, opts)
    assert c1[0] and _bits(l1)[0] == _bits(losses)[0] and n_evals[0] > 1
    # the same seed gives the same result
    again = optimize_constants_batch(tb, ds, opts, np.random.default_rng(0))
    assert np.array_equal(_bits(again[0].parameters), _bits(new_tb.parameters))
    assert np.array_equal(_bits(again[0].val), _bits(new_tb.val)) and np.array_equal(again[3], n_evals)
    assert np.array_equal(tb.parameters, np.ones((1, 2, 3)))  # (the input batch is untouched)


def test_optimiser_newton_case_and_nothing_to_optimise():
    X, y, cls, a = _recovery_problem()
    # one scalar in all (K = C = 1): Newton
    opts1 = _popts(1, unary_operators=["cos", "exp"])
    ones = np.ones(2000, dtype=np.int32)
    ds1 = _pds(X, 3.0 * X[0], ones, 1)
    tb = _one("x1 * p1", opts1, [[1.0]], np.float64)
    new_tb, losses, improved, _ = optimize_constants_batch(tb, ds1, opts1, np.random.default_rng(0))
    assert improved[0] and abs(new_tb.parameters[0, 0, 0] - 3.0) <= 1e-6 and losses[0] < 1e-10
    # nothing to optimise: x1 * x2 does not read its matrix (every gradient entry is 0, every restart scores
    # the same): not improved, constants and parameters bit-unchanged
    ds = _pds(X, y, cls, 3)
    opts2 = _popts(2, unary_operators=["cos", "exp"])
    P = np.random.default_rng(5).standard_normal((2, 3))
    tb2 = _one("x1 * x2", opts2, P, np.float64)
    l2, _ = eval_loss_batch(tb2, ds, opts2)
    new2, losses2, improved2, _ = optimize_constants_batch(tb2, ds, opts2, np.random.default_rng(0))
    assert not improved2[0] and _bits(losses2)[0] == _bits(l2)[0]
    assert np.array_equal(_bits(new2.parameters), _bits(tb2.parameters)) and np.array_equal(_bits(new2.val), _bits(tb2.val))


def test_plain_batch_takes_the_plain_entry_point():
    """A plain batch through optimize_constants_batch: exactly sr_optimize_constants_batch's results."""
    opts = Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    X, y, cls, a = _recovery_problem()
    tb = flatten_trees([parse_expression(e, opts) for e in ("1.0 * x1 + 1.0", "x1 * 1.0", "cos(x2 * 0.5) * 0.3 + x1")],
                       np.float64)
    ds = Dataset(X, y)
    new_tb, losses, improved, n_evals = optimize_constants_batch(tb, ds, opts, np.random.default_rng(7))
    ctx = sr_amd.get_context()
    seed = int(np.random.default_rng(7).integers(0, 2 ** 63))
    consts, lo = np.zeros(int(tb.constant_mask().sum())), np.zeros(3)
    imp, fc = np.zeros(3, dtype=np.uint8), np.zeros(3, dtype=np.int64)
    s = tb.to_struct()
    p = lambda v: v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    _lib.check(_lib.lib.sr_optimize_constants_batch(
        ctx.handle, ds.device_handle(ctx), ctx.opset_id(opts.operators), ctypes.byref(s), None, 0, ctx.loss_code(opts),
        8, 10_000, 2, ctypes.c_uint64(seed), p(consts), p(lo), p(imp), p(fc)))
    assert np.array_equal(_bits(new_tb.get_constants()), _bits(consts)) and np.array_equal(_bits(losses), _bits(lo))
    assert np.array_equal(improved, imp.astype(bool)) and improved[0]
