"""GPU: the loss catalog per point (sr_elem_loss / sr_elem_loss_deriv, csrc/sr_ops.h) on every device path that
evaluates an elementwise loss, against tests/golden/loss_values.json (mpmath at 60 digits from the published
LossFunctions.jl definitions; test_loss_values_host.py pins the fixture and the host restatements).

1. Elements: every loss, parameter and point, Float32 and Float64, under the BASIC and the FULL operator set (the
   tile builds of both tiers, and the gradient kernels), unweighted and with power-of-two weights: exact class
   bit-equal, inexact class within loss_values_util.BARS["device"], overflow points +-Inf on a complete tree.
2. Builds: the same element values and derivatives under every knob setting that reaches another build.
3. The same points as one plain 1,153-row dataset: the loss is the in-order fold in T of the device's own element
   values, bit for bit in Float32 on the stored-loss path, the FOLD-mode path, the forced fallback (SrFoldRows) and
   a gathered view; weighted with non-dyadic weights; ref_fold = 0 and Float64 within loss_expr_points'
   mean_tolerances.
4. The candidate-composing and register-stack FOLD generic builds, which run only in a large plain Float32 call:
   2^18 rows, 520 trees x1 * c_k, bit-equal to numpy's fold of the formula evaluated step by step in Float32.
"""
import ctypes
import functools

import numpy as np
import pytest

import loss_values_util as U
import sr_amd
from loss_expr_points import N_FULL, TIERS, full_rows, mean_tolerances
from sr_amd import Dataset, Node, Options, _lib, batch, eval_grad_batch, eval_loss_batch, flatten_trees, parse_expression
from test_gpu_build_table import DEFAULTS, _knob_cases
from test_gpu_ref_fold import _jl_sum32

pytestmark = pytest.mark.gpu

DT = list(U.DTYPES)


@functools.lru_cache(maxsize=None)
def _elements(dtype_name, spec, tier, weighted):
    """The device's element values, computed once and shared; never modified (read-only arrays)."""
    pts = U.Points(dtype_name, spec)
    val, der, comp = U.device_elements(pts, tier, weighted)
    for a in (val, der, comp):
        a.setflags(write=False)
    return pts, val, der, comp


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("dtype_name", DT)
def test_elements(dtype_name, tier, weighted):
    counts = {}
    for spec in U.specs(dtype_name):
        pts, val, der, comp = _elements(dtype_name, spec, tier, weighted)
        what = (spec, dtype_name, tier, "weighted" if weighted else "plain")
        assert comp.all(), (what, pts.pred[~comp], pts.target[~comp])  # (an overflowing loss leaves the tree complete)
        U.assert_meets(pts, val, der, "device", what, counts)
    want = {(dtype_name, s): len(U.fixture()[dtype_name][s]["points"]) for s in U.fixture()[dtype_name]}
    assert counts == want and sum(counts.values()) > 1900, (len(counts), len(want))


BUILD_SPECS = ["HuberLoss(0.5)", "DWDMarginLoss(2)", "L1DistLoss()", "L2DistLoss()"]


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("dtype_name", DT)
@pytest.mark.parametrize("spec", BUILD_SPECS)
def test_builds(spec, dtype_name, tier):
    """The element values under every ("rows_per_lane", "vstk_rows", "max_row_blocks") setting
    test_gpu_build_table._knob_cases lists for a plain call of this dtype and tier over a row view, and the element
    derivatives under every forced "grad_rows": bit-identical to the default's."""
    from loss_expr_points import one_row_gradients, one_row_losses

    pts, val, der, comp = _elements(dtype_name, spec, tier, False)
    ctx = sr_amd.get_context()
    ds = U.dataset(pts)
    cases = _knob_cases("plain", pts.T, tier == "BASIC", False)
    assert len(cases) >= 4
    try:
        for rpl, vstk, mrb in cases:
            for name, value in (("rows_per_lane", rpl), ("vstk_rows", vstk), ("max_row_blocks", mrb)):
                ctx.set_tuning(name, value)
            got, gc = one_row_losses(U.options(spec, tier), ds, pts.n, pts.T)
            assert np.array_equal(gc, comp) and np.array_equal(U.bits(got), U.bits(val)), (spec, dtype_name, tier, rpl, vstk, mrb)
        for name, value in DEFAULTS.items():
            ctx.set_tuning(name, value)
        for rows in (1, 2, 4, 8):
            ctx.set_tuning("grad_rows", rows)
            g, gc = one_row_gradients(U.options(spec, tier, gradient=True), ds, pts.n, pts.T)
            assert np.array_equal(gc, comp) and np.array_equal(U.bits(g), U.bits(der)), (spec, dtype_name, tier, "grad_rows", rows)
    finally:
        for name, value in DEFAULTS.items():
            ctx.set_tuning(name, value)
        ctx.set_tuning("grad_rows", 0)
        ds.free_device()


# ------------------------------------------------------------------------------------------------- 3. the full view
FOLD_DEFAULTS = {"ref_fold": 1, "fold_store_mb": 512, "fold_delta_log2": 8, "fold_debug_fail": 0}


def _scored(tb, target, opts, **knobs):
    ctx = sr_amd.get_context()
    for k, v in knobs.items():
        ctx.set_tuning(k, v)
    try:
        loss, comp = eval_loss_batch(tb, target, opts)
        info = ctx.last_ref_fold()
    finally:
        for k, v in FOLD_DEFAULTS.items():
            ctx.set_tuning(k, v)
    assert comp.all()
    return loss[0], info


def _fold(terms, T):
    return np.add.accumulate(terms.astype(T), dtype=T)[-1]


def _full_view_rows(pts):
    """Fixture point of each of the N_FULL rows: the finite points (an overflow point would make every sum Inf),
    tiled with loss_expr_points.full_rows' rotation."""
    keep = np.nonzero(pts.cls != U.OVERFLOW)[0]
    return keep[full_rows(len(keep))]


@pytest.mark.parametrize("spec", list(U.specs("float32")))
def test_full_view_in_order_fold_float32(spec):
    """1,153 rows (two full 512-row tiles and a ragged one; every path engages at this count).  The loss is the
    sequential Float32 fold of the device's own element values divided by Float32(n): no tolerance.  Routes: stored
    losses (path 1), FOLD mode (path 2), the forced fallback through the prediction pass (SrFoldRows), a gathered
    view (a permutation of the rows with repeats), non-dyadic weights — the fold of T(value_k w_k) divided by
    Base.sum(w) — and both (the fallback's 16-byte reads serve a full view, its scalar reads a gathered one)."""
    T = np.float32
    pts, val, der, _ = _elements("float32", spec, "BASIC", False)
    rows = _full_view_rows(pts)
    opts = U.options(spec, "BASIC")
    tb = flatten_trees([Node(feature=1)], T)
    want = T(_fold(val[rows], T) / T(N_FULL))
    rng = np.random.default_rng(1153)
    gather = rng.integers(0, N_FULL, size=N_FULL)
    gather[:600] = rng.permutation(N_FULL)[:600]
    want_g = T(_fold(val[rows][gather], T) / T(N_FULL))
    w = (0.25 + rng.random(N_FULL)).astype(T)
    want_w = T(_fold((val[rows] * w).astype(T), T) / _jl_sum32(w))
    want_wg = T(_fold((val[rows] * w).astype(T)[gather], T) / _jl_sum32(w[gather]))
    ds, dsw = U.dataset(pts, rows=rows), U.dataset(pts, weights=w, rows=rows)
    try:
        for target, expect, name in ((ds, want, "plain"), (batch(ds, gather), want_g, "gathered"), (dsw, want_w, "weighted"),
                                     (batch(dsw, gather), want_wg, "weighted, gathered")):
            got, info = _scored(tb, target, opts)
            assert info["path"] == 1 and info["folded"] == 1 and info["fallback"] == 0, (spec, name, info)
            assert U.bits(got) == U.bits(expect), (spec, name, "stored", got, expect)
            got, info = _scored(tb, target, opts, fold_store_mb=0)
            assert info["path"] == 2 and info["folded"] + info["fallback"] == 1, (spec, name, info)
            assert U.bits(got) == U.bits(expect), (spec, name, "FOLD mode", got, expect)
            got, info = _scored(tb, target, opts, fold_store_mb=0, fold_delta_log2=30, fold_debug_fail=3)
            assert info["path"] == 2 and info["fallback"] == 1, (spec, name, info)
            assert U.bits(got) == U.bits(expect), (spec, name, "fallback", got, expect)
    finally:
        ds.free_device()
        dsw.free_device()


@pytest.mark.parametrize("dtype_name", DT)
@pytest.mark.parametrize("spec", list(U.specs("float32")))
def test_full_view_f64_sum_and_gradient(spec, dtype_name):
    """ref_fold = 0 (Float32) and Float64 (path 0 at this size, asserted): the loss within mean_tolerances of the
    f64 mean of the device's element values; the gradient of x1 + 0.0 is the mean of the element derivatives within
    the gradient kernel's bound (test_gpu_grad_rules.K_T).  Unweighted and with the power-of-two weights 0.5, 2, 4.

    Not with non-dyadic weights: mean_tolerances' loss bound (1 ulp_T of the mean plus the f64 sum's own error) has
    no term for the tile's sum, which the loss kernel takes in T over its 512 values before the f64 sum (its
    docstring: exact for dyadic values).  Measured on an MI355X with weights 0.25 + U(0, 1) in Float32: 60 of the 62
    cases inside the bound; QuantileLoss(0.75) 1.34e-7 off against 1.19e-7 and PeriodicLoss(4.0) 3.12e-8 against
    2.98e-8 (1.13 and 1.05 ulp of the mean), which nine roundings of a 512-value pairwise sum explain.  The in-order
    fold above, which is what a default call returns, holds those weights bit for bit."""
    if spec not in U.specs(dtype_name):
        return
    T = U.DTYPES[dtype_name]
    pts, val, der, _ = _elements(dtype_name, spec, "BASIC", False)
    rows = _full_view_rows(pts)
    opts, gopts = U.options(spec, "BASIC"), U.options(spec, "BASIC", gradient=True)
    tb = flatten_trees([Node(feature=1)], T)
    gtb = flatten_trees([parse_expression("x1 + 0.0", gopts)], T)
    w = np.array([U.WEIGHTS[k % 3] for k in range(N_FULL)], dtype=T)
    for weights in (None, w):
        ds = U.dataset(pts, weights=weights, rows=rows)
        try:
            v, d = val[rows], der[rows]
            if weights is not None:  # (exact products)
                v, d = (v * w).astype(T), (d * w).astype(T)
            v, d = v.astype(np.float64), d.astype(np.float64)
            mean, tol_l, gmean, tol_g = mean_tolerances(v, d, w, weights is not None, T)
            got, info = _scored(tb, ds, opts, ref_fold=0)
            assert info["path"] == 0, info
            print(spec, dtype_name, "weighted" if weights is not None else "plain", "loss", got, mean, abs(float(got) - mean), tol_l)
            assert abs(float(got) - mean) <= tol_l, (spec, dtype_name, got, mean, tol_l)
            _, g, gc = eval_grad_batch(gtb, ds, gopts)
            assert gc.all() and g.shape == (1,)
            print(spec, dtype_name, "gradient", g[0], gmean, abs(float(g[0]) - gmean), tol_g)
            assert abs(float(g[0]) - gmean) <= tol_g, (spec, dtype_name, g[0], gmean, tol_g)
        finally:
            ds.free_device()


# ------------------------------------------------------------------------------------------------- 4. the large call
N_BIG, NT_BIG = 1 << 18, 520


def _step_by_step(spec, pred, y):
    """The published formula step by step in Float32 over arrays (Huber(0.5), L2Hinge, L2)."""
    T = np.float32
    if spec == "L2DistLoss()":
        d = pred - y
        return d * d
    if spec == "HuberLoss(0.5)":
        d = pred - y
        ad, p = np.abs(d), T(0.5)
        return np.where(ad <= p, T(0.5) * (d * d), p * ad - T(0.5) * (p * p))
    if spec == "L2HingeLoss()":
        a = y * pred
        e = T(1) - a
        return np.where(a >= 1, T(0), e * e)
    raise ValueError(spec)


@functools.lru_cache(maxsize=None)
def _big_data():
    """x1: multiples of 1/64 in [-4, 4); c_k: multiples of 1/8 in [-2, 2] but 0 — x1 * c_k is exact in Float32, so
    numpy restates the predictions; targets: multiples of 1/16 (distance) and +-1 (margin)."""
    rng = np.random.default_rng(218)
    x = (rng.integers(-256, 256, size=N_BIG) / 64.0).astype(np.float32)
    c = np.array([(k % 16 + 1) / 8.0 * (1 if (k // 16) % 2 == 0 else -1) for k in range(NT_BIG)], dtype=np.float32)
    y_d = (rng.integers(-64, 64, size=N_BIG) / 16.0).astype(np.float32)
    y_m = np.where(rng.random(N_BIG) < 0.5, -1.0, 1.0).astype(np.float32)
    return x, c, y_d, y_m


@pytest.mark.parametrize("spec", ["HuberLoss(0.5)", "L2HingeLoss()", "L2DistLoss()"])
def test_large_plain_call_generic_fold_builds(spec):
    """2^18 rows and 520 register-stack trees, the smallest shape at which the listed loss launch composes the
    fold's steps under candidate binades and the FOLD-mode pass runs (test_gpu_validity.py): the launch counters as
    there, and every tree's loss the sequential Float32 fold of the step-by-step losses of x1 * c_k, bit for bit.
    L2 is the control (a build of its own); Huber(0.5) and L2Hinge run the generic builds."""
    T = np.float32
    x, c, y_d, y_m = _big_data()
    y = y_m if spec == "L2HingeLoss()" else y_d
    opts = U.options(spec, "BASIC")
    tb = flatten_trees([parse_expression(f"x1 * {float(ck)!r}", opts) for ck in c], T)
    ctx = sr_amd.get_context()
    ds = Dataset(np.ascontiguousarray(x[None, :]), y)
    try:
        loss, comp = eval_loss_batch(tb, ds, opts)
        info = ctx.last_ref_fold()
        cand = ctx.last_fold_cand()
        out = (ctypes.c_double * 19)()
        _lib.check(_lib.lib.sr_last_phase_ms(ctx.handle, out, 19))
    finally:
        ds.free_device()
    listed, live, excl = int(out[16]), int(out[17]), int(out[18])
    print(spec, info, cand, listed, live, excl)
    assert comp.all()
    assert info["path"] == 2 and info["folded"] + info["fallback"] == NT_BIG, info
    assert listed >= 1 and live + excl == NT_BIG and excl == 0, (listed, live, excl)
    assert cand["taken"] > 0, cand  # (steps composed by the loss launch under its candidate binades)
    want = np.array([T(_fold(_step_by_step(spec, x * ck, y), T) / T(N_BIG)) for ck in c], dtype=T)
    bad = np.nonzero(U.bits(loss) != U.bits(want))[0]
    assert bad.size == 0, (spec, bad[:5], loss[bad[:5]], want[bad[:5]])


# ------------------------------------------------------------------------------------------------- parameters
def test_register_loss_refuses_a_parameter_outside_the_domain():
    ctx = sr_amd.get_context()
    out = ctypes.c_int(0)
    for kind in (2, 4, 5, 6, 7, 13, 18):
        for bad in (0.0, -0.0, -1.5, float("nan"), float("inf")):
            assert _lib.lib.sr_register_loss(ctx.handle, kind, bad, ctypes.byref(out)) == _lib.SR_ERR_INVALID_ARG, (kind, bad)
        assert _lib.lib.sr_register_loss(ctx.handle, kind, 0.125, ctypes.byref(out)) == _lib.SR_OK
    for tau in (0.0, -0.5, 0.25):
        assert _lib.lib.sr_register_loss(ctx.handle, 8, tau, ctypes.byref(out)) == _lib.SR_OK
