"""GPU: a scoring call leaves nothing behind for the next one, and the entry points refuse as they always did.

Each scoring call carries what it asks for — the view, the parameter side of a ParametricExpression batch,
the row views, whether the fold's internal passes may touch the last-call record — through the batch engine.
These tests pin what a slip there would change: plain and parametric calls interleaved on one context, a
parametric call that fails half way, the fold's fallback passes (which score a few trees of the batch with a
parameter side of their own, inside the call), and every entry point's refusals, in their order.
"""
import ctypes

import numpy as np
import pytest

import sr_amd
from sr_amd import (Dataset, Options, _lib, batch, eval_grad_batch, eval_grad_batch_views, eval_loss_batch,
                    eval_loss_batch_views, eval_tree_array_batch, flatten_trees, gen_random_population)
from sr_amd.device import get_lane_context
from sr_amd.node import TreeBatch
from parametric_util import data, population, to_parametric

pytestmark = pytest.mark.gpu

OPTS = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "log"])
NF, K, NC = 3, 2, 5
N, NT = 3000, 64


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    """Two results of one call (tuples of arrays): equal bit for bit."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(_bits(x) if x.dtype.kind == "f" else x, _bits(y) if y.dtype.kind == "f" else y)


def _pds(X, y, cls):
    return Dataset(X, y, extra={"class": cls}, n_classes=NC)


@pytest.fixture(scope="module")
def small():
    """64 plain trees and 64 parametric ones (distinct (2, 5) matrices) over 3,000 rows with classes."""
    opts = Options(**OPTS)
    X, y, cls = data(N, NF, NC, seed=71)
    plain = flatten_trees(gen_random_population(NT, opts, NF, max_size=30, seed=72), np.float32)
    ext = population(NT, opts, NF, K, seed=73)
    P = np.random.default_rng(74).standard_normal((NT, K, NC)).astype(np.float32)
    par = to_parametric(ext, NF, P)
    assert par.is_parameter.sum() >= 20
    return opts, _pds(X, y, cls), plain, par


def _plain_loss(small):
    opts, ds, plain, _ = small
    return eval_loss_batch(plain, ds, opts)


def _par_loss(small):
    opts, ds, _, par = small
    return eval_loss_batch(par, ds, opts)


# ------------------------------------------------------------------ a. plain and parametric calls interleaved
def _views(kind, ds):
    """The dataset (or its view) and the row views of one case: the full data, one 200-row view, two views."""
    rng = np.random.default_rng(75)
    if kind == "full":
        return ds, None
    if kind == "one":
        return batch(ds, rng.integers(0, N, size=200)), None
    return ds, (np.arange(NT) % 2, rng.integers(0, N, size=(2, 200)))


@pytest.mark.parametrize("kind", ["full", "one", "two"])
def test_plain_and_parametric_calls_interleave(small, kind):
    """plain, parametric, plain, parametric — eval_loss_batch, eval_grad_batch and (16 trees) eval_tree_array_batch:
    the two plain results are the same bits, and so are the two parametric ones."""
    opts, ds, plain, par = small
    view, vs = _views(kind, ds)
    first = np.arange(16)
    if vs is None:
        calls = [lambda tb: eval_loss_batch(tb, view, opts), lambda tb: eval_grad_batch(tb, view, opts),
                 lambda tb: eval_tree_array_batch(tb.take(first), view, opts)]
    else:  # (predictions have no several-views call)
        calls = [lambda tb: eval_loss_batch_views(tb, view, opts, vs[0], vs[1]),
                 lambda tb: eval_grad_batch_views(tb, view, opts, vs[0], vs[1])]
    for call in calls:
        a0, p0, a1, p1 = call(plain), call(par), call(plain), call(par)
        _same(a0, a1)
        _same(p0, p1)
        assert a0[-1].any() and p0[-1].any()  # (some complete trees on either side)
        assert not np.array_equal(_bits(a0[0]), _bits(p0[0]))


# ------------------------------------------------------------------ b. a failing parametric call leaves no trace
def test_failed_parametric_call_leaves_no_trace(small):
    opts, ds, plain, par = small
    ctx = sr_amd.get_context()
    a0, p0 = _plain_loss(small), _par_loss(small)
    out_l, out_c = np.empty(NT, dtype=np.float32), np.empty(NT, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def call(tb):
        s, ps = tb.to_struct(), tb.to_param_struct()
        return _lib.lib.sr_eval_loss_batch_parametric(ctx.handle, ds.device_handle(ctx), ctx.opset_id(opts.operators),
                                                      ctypes.byref(s), ctypes.byref(ps), None, 0, 0, p(out_l), p(out_c))

    # refused inside the engine, by the compiler, once the parameter side is in place: parameter index > K
    bad_par = par.parameter.copy()
    bad_par[par.is_parameter != 0] = K + 1
    bad = TreeBatch(par.offsets, par.degree, par.op, par.feature, par.constant, par.val, par.is_parameter, bad_par,
                    par.parameters)
    assert call(bad) == _lib.SR_ERR_BAD_TREE
    _same(_plain_loss(small), a0)
    _same(_par_loss(small), p0)
    # refused at the entry: a class count that is not the dataset's
    wrong = TreeBatch(par.offsets, par.degree, par.op, par.feature, par.constant, par.val, par.is_parameter,
                      par.parameter, np.ones((NT, K, NC + 1), dtype=np.float32))
    assert call(wrong) == _lib.SR_ERR_INVALID_ARG and "n_classes" in _lib.last_error()
    _same(_plain_loss(small), a0)
    _same(_par_loss(small), p0)


# ------------------------------------------------------------------ c. the fold's internal passes
def test_fold_fallback_passes_keep_the_call_record(small):
    """A parametric FOLD-mode call whose every third tree takes the fallback (the prediction pass over those
    trees alone, with their own parameter side, inside the call): the losses are those of the call without
    a fallback, and the last-call record — chunks, rows per lane, derived columns, the fold's path — is the
    call's own loss launches', not the internal passes'."""
    opts = Options(**OPTS)
    n, nt = 40_000, 400
    X, y, cls = data(n, NF, NC, seed=51)
    ext = population(nt, opts, NF, K, seed=52)
    P = np.random.default_rng(53).standard_normal((nt, K, NC)).astype(np.float32)
    par = to_parametric(ext, NF, P)
    d = _pds(X, y, cls)
    ctx = sr_amd.get_context()
    a0 = _plain_loss(small)

    def run(debug_fail):
        for k, v in dict(timing=1, fold_store_mb=0, fold_delta_log2=30, fold_debug_fail=debug_fail).items():
            ctx.set_tuning(k, v)
        try:
            loss, comp = eval_loss_batch(par, d, opts)
            info = ctx.last_ref_fold()
            rec = dict(chunks=ctx.last_launches(), rows=ctx.last_rows_per_lane(), derived=ctx.last_derived_columns(),
                       path=info["path"])
            kernel_ms = ctx.last_kernel_ms()[0]
        finally:
            ctx.set_tuning("fold_store_mb", 512)
            ctx.set_tuning("fold_delta_log2", 8)
            ctx.set_tuning("fold_debug_fail", 0)
        return loss, comp, info, rec, kernel_ms

    l0, c0, i0, r0, _ = run(0)
    l3, c3, i3, r3, ms3 = run(3)
    assert i0["path"] == 2 and i3["fallback"] > 0, (i0, i3)
    assert np.array_equal(c0, c3)
    fin = c0 & np.isfinite(l0)
    assert fin.sum() > 100
    assert np.array_equal(_bits(l0[fin]), _bits(l3[fin]))
    assert r0 == r3, (r0, r3)
    assert r3["chunks"] >= 1 and r3["rows"] > 0
    assert ms3 > 0.0  # (the call was timed although its internal passes were not)
    _same(_plain_loss(small), a0)


# ------------------------------------------------------------------ d. the entry points' refusals
EXPR_LOSS = 1 << 20  # the first expression-loss code (sr_register_loss_expr)
INVALID = _lib.SR_ERR_INVALID_ARG
ENTRIES = {  # name -> (parametric, views, kind)
    "sr_eval_loss_batch": (False, False, "loss"),
    "sr_eval_loss_batch_parametric": (True, False, "loss"),
    "sr_eval_loss_batch_views": (False, True, "loss"),
    "sr_eval_loss_batch_views_parametric": (True, True, "loss"),
    "sr_eval_grad_batch": (False, False, "grad"),
    "sr_eval_grad_batch_parametric": (True, False, "grad"),
    "sr_eval_grad_batch_views": (False, True, "grad"),
    "sr_eval_grad_batch_views_parametric": (True, True, "grad"),
    "sr_eval_tree_array": (False, False, "pred"),
    "sr_eval_tree_array_parametric": (True, False, "pred"),
}
# What the entry points have always answered, as (code, part of sr_last_error's text), written down from the
# checks' own source — not taken from a run.
NULL_TREES = (INVALID, "NULL tree batch")
BAD_OPSET = (INVALID, "unknown opset id 12345")
OTHER_CTX = (INVALID, "dataset is NULL or belongs to another context")
NULL_PARAMS = (INVALID, "NULL parameter batch")
CLASSES = (INVALID, "sr_param_batch n_classes 6 differs from the dataset's 5")
BAD_VIEWS = (INVALID, "bad row views")
NULL_OUT = (INVALID, "NULL output buffers")
NO_Y = (INVALID, "dataset has no y")
EXPR_ONLY = (INVALID, "an expression loss (sr_register_loss_expr) is taken by sr_eval_loss_batch(_views)")


class _Entry:
    """One entry point's argument list over a 64-row dataset and 8 trees, with single arguments replaced."""

    def __init__(self):
        self.opts = Options(**OPTS)
        self.ctx = sr_amd.get_context()
        self.other = get_lane_context(1)
        X, y, cls = data(64, NF, NC, seed=81)
        self.ds = _pds(X, y, cls)
        self.ds_no_y = Dataset(X, None, extra={"class": cls}, n_classes=NC)
        ext = population(8, self.opts, NF, K, seed=82)
        self.par = to_parametric(ext, NF, np.ones((K, NC), dtype=np.float32))
        self.par6 = to_parametric(ext, NF, np.ones((K, NC + 1), dtype=np.float32))
        self.plain = flatten_trees(gen_random_population(8, self.opts, NF, max_size=30, seed=83), np.float32)
        self.tv = np.zeros(8, dtype=np.int32)
        self.vr = np.arange(32, dtype=np.int64).reshape(2, 16)
        self.out = [np.zeros(8 * 64 + 256, dtype=np.float32) for _ in range(2)] + [np.zeros(8, dtype=np.uint8)]

    def __call__(self, name, **bad):
        parametric, views, kind = ENTRIES[name]
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        tb = self.par if parametric else self.plain
        s = tb.to_struct()
        ds = self.ds_no_y if bad.get("no_y") else self.ds
        args = [self.ctx.handle, ds.device_handle(self.other if bad.get("other_ctx") else self.ctx),
                12345 if bad.get("opset") else self.ctx.opset_id(self.opts.operators),
                None if bad.get("null_trees") else ctypes.byref(s)]
        if parametric:
            ps = (self.par6 if bad.get("classes") else tb).to_param_struct()
            args.append(None if bad.get("null_params") else ctypes.byref(ps))
        if views:
            args += [p(self.tv), 0 if bad.get("no_views") else 2, None if bad.get("null_rows") else p(self.vr), 16]
        else:
            args += [None, 0]
        if kind != "pred":
            args.append(EXPR_LOSS if bad.get("expr") else 0)
        outs = [p(self.out[0]), p(self.out[1]), p(self.out[2])] if kind == "grad" else [p(self.out[0]), p(self.out[2])]
        args += [None] * len(outs) if bad.get("null_out") else outs
        rc = getattr(_lib.lib, name)(*args)
        return rc, _lib.last_error()


@pytest.fixture(scope="module")
def entry():
    return _Entry()


def _refused(got, want):
    assert got[0] == want[0] and want[1] in got[1], (got, want)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entry_point_refusals(entry, name):
    parametric, views, kind = ENTRIES[name]
    assert entry(name)[0] == 0, _lib.last_error()  # (the valid call these cases spoil one argument of)
    _refused(entry(name, null_trees=True), NULL_TREES)
    _refused(entry(name, opset=True), BAD_OPSET)
    _refused(entry(name, other_ctx=True), OTHER_CTX)
    _refused(entry(name, null_out=True), NULL_OUT)
    if parametric:
        _refused(entry(name, null_params=True), NULL_PARAMS)
        _refused(entry(name, classes=True), CLASSES)
    if views:
        _refused(entry(name, no_views=True), BAD_VIEWS)
        _refused(entry(name, null_rows=True), BAD_VIEWS)
    if kind == "grad":
        _refused(entry(name, no_y=True), NO_Y)
    if parametric and kind != "pred":
        _refused(entry(name, expr=True), EXPR_ONLY)
    # two at once: which one is named is the order of the checks
    _refused(entry(name, other_ctx=True, opset=True), OTHER_CTX)
    _refused(entry(name, opset=True, null_trees=True), BAD_OPSET)
    _refused(entry(name, null_trees=True, null_out=True), NULL_TREES)
    if parametric:
        _refused(entry(name, null_trees=True, null_params=True), NULL_TREES)
        _refused(entry(name, null_params=True, null_out=True), NULL_PARAMS)
    if parametric and views:
        _refused(entry(name, classes=True, no_views=True), CLASSES)
    if parametric and kind != "pred":  # an expression loss is refused before the context is looked at
        _refused(entry(name, expr=True, null_trees=True), EXPR_ONLY)
        _refused(entry(name, expr=True, other_ctx=True), EXPR_ONLY)
    if views:
        _refused(entry(name, no_views=True, null_out=True), BAD_VIEWS)
    if kind == "grad":
        _refused(entry(name, null_out=True, no_y=True), NULL_OUT)
    assert entry(name)[0] == 0, _lib.last_error()
