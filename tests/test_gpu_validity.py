"""GPU: the `complete` flag per operator, check site and kernel build, against the two rules of validity_util.py.

Rule A: absorber(producer, other operand) under five wrappers; the producer is non-finite on one row, and the tree
is incomplete with loss +Inf whatever the absorber makes of it (`inv(exp(x1))`, `tanh(..)`, `x2 > ..`, `cond`, `min`,
`atan2(2.0, ..)`); on the control data, which lacks that row's value, every form is complete with a finite loss.
Rule B: an array of finite values whose sum overflows makes the tree incomplete exactly where DynamicExpressions
array-checks it.  The expectations come from the rules alone (tests/test_validity_host.py holds them against the
oracle on the CPU): no oracle call and no tolerance here, except for the controls' predictions.

All forms of an operator set and group go in one batch (a group shares its dataset: validity_util's "E", "L", "K"),
in Float32 and Float64, with the BASIC operator set and the whole catalog.  Sizes 1, 65, 1153 and 4161 rows
(2 x 2048 + 65: three row tiles at 32 rows per lane, the largest tile of any build; 9 to 33 at the default 8 and 4
rows per lane; the last one partly filled, its padding a replica of a real row); the bad row first or last, so at
4161 rows in the first or the last tile alone.  Every call is made twice and must repeat bit for bit, predictions
and gradients included.  Nothing is filtered: every test counts what it asserted.
"""
import ctypes
import functools

import numpy as np
import pytest

import sr_amd
import validity_util as V
from oracle import Oracle
from parametric_util import to_parametric
from parity_util import PERTURB_SEEDS
from sr_amd import _lib
from sr_amd import (Dataset, Options, SubDataset, eval_grad_batch, eval_loss_batch, eval_loss_batch_views,
                    eval_tree_array_batch, optimize_constants_batch)
from test_gpu_build_table import DEFAULTS, _knob_cases

pytestmark = pytest.mark.gpu

OPSETS = ("basic", "full")
N_TILES = 4161  # 2 x 64 x 32 + 65
SIZES = ((1, 0), (65, 0), (65, 64), (1153, 0), (1153, 1152), (N_TILES, 0), (N_TILES, N_TILES - 1))
both = pytest.mark.parametrize("dtype_name", list(V.DTYPES))
sets = pytest.mark.parametrize("opset", OPSETS)


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view({4: np.uint32, 8: np.uint64}[v.dtype.itemsize])


def _twice(call):
    """The call's (loss, complete[, further arrays: predictions, gradients]), made twice: every array bit-equal."""
    first, second = call(), call()
    assert len(first) == len(second)
    for k, (a, b) in enumerate(zip(first, second)):
        a, b = np.asarray(a), np.asarray(b)
        assert np.array_equal(a, b) if a.dtype == bool else np.array_equal(_bits(a), _bits(b)), ("not repeatable", k)
    return np.asarray(first[0]), np.asarray(first[1])


def _assert_flags(forms, loss, comp, complete, what):
    """Incomplete with +Inf, or complete with a finite loss, for every form."""
    if complete:
        wrong = [(forms[k].expr, bool(comp[k]), float(loss[k])) for k in np.nonzero(~comp | ~np.isfinite(loss))[0]]
    else:
        wrong = [(forms[k].expr, bool(comp[k]), float(loss[k])) for k in np.nonzero(comp | ~np.isposinf(loss))[0]]
    assert not wrong, (what, "complete" if complete else "incomplete", len(wrong), wrong[:6])
    return len(forms)


def _rule_a(opset, dtype_name, n, bad_row, score, what="", groups=V.GROUPS, make=None):
    """score(batch, dataset) -> (loss, complete) on each group's bad dataset and on the control; returns the number
    of (form, dataset) verdicts asserted.  `make(X, y)` builds the dataset (default: Dataset(X, y))."""
    T = V.DTYPES[dtype_name]
    data = V.rule_a_data(n, T, bad_row)
    y = np.zeros(n, dtype=T)
    make = make or (lambda X, y: Dataset(X, y))
    asserted = 0
    for group in groups:
        tb = V.rule_a_batch(opset, group, dtype_name)
        forms = V.rule_a_forms(opset, group)
        for which in (group, "control"):
            ds = make(data[which], y)
            try:
                loss, comp = _twice(lambda: score(tb, ds))
            finally:
                ds.free_device()
            complete = which == "control" and group != "K"
            asserted += _assert_flags(forms, loss, comp, complete, (what, opset, dtype_name, n, bad_row, group, which))
    return asserted


def _n_verdicts(opset, groups=V.GROUPS):
    return 2 * sum(len(V.rule_a_forms(opset, g)) for g in groups)


# ------------------------------------------------------------------------------------------- eval_loss_batch
@both
@sets
def test_loss_full_view_every_size_and_bad_row(opset, dtype_name):
    opts = V.options(opset)
    asserted = sum(_rule_a(opset, dtype_name, n, bad, lambda tb, ds: eval_loss_batch(tb, ds, opts)) for n, bad in SIZES)
    assert asserted == len(SIZES) * _n_verdicts(opset)


@both
@sets
@pytest.mark.parametrize("n", [1153, N_TILES])
def test_loss_row_view_with_and_without_the_bad_row(opset, dtype_name, n):
    """A SubDataset (the gather builds): a view that holds the bad row is incomplete; the same view with that row's
    index replaced by its neighbour's is complete, on the dataset that still holds the bad row."""
    opts = V.options(opset)
    T = V.DTYPES[dtype_name]
    bad_row = n - 2
    rng = np.random.default_rng(n)
    idx = rng.permutation(n)[: n - 64].astype(np.int64)
    idx = idx[idx != bad_row]
    with_bad = np.concatenate([idx, [bad_row]])  # in the view's last, partly filled tile
    without = np.concatenate([idx, [bad_row - 1]])
    data = V.rule_a_data(n, T, bad_row)
    y = np.zeros(n, dtype=T)
    asserted = 0
    for group in ("E", "L"):
        tb, forms = V.rule_a_batch(opset, group, dtype_name), V.rule_a_forms(opset, group)
        ds = Dataset(data[group], y)
        try:
            for view, complete in ((with_bad, False), (without, True), (with_bad[::-1].copy(), False)):
                sub = SubDataset(ds, view)
                loss, comp = _twice(lambda: eval_loss_batch(tb, sub, opts))
                asserted += _assert_flags(forms, loss, comp, complete, ("row view", opset, dtype_name, n, group, complete))
        finally:
            ds.free_device()
    assert asserted == 3 * _n_verdicts(opset, ("E", "L")) // 2


@both
@sets
def test_weighted_calls_and_a_loss_that_swallows_nan(opset, dtype_name):
    """Weighted calls, and two losses outside sr_loss_propagates_nan: the root's NaN test reads the root values, not
    the loss sum.  L1HingeLoss, and ZeroOneLoss (t p < 0 ? 1 : 0), which does map a NaN prediction to a number."""
    n, asserted = N_TILES, 0
    w = (0.5 + (np.arange(n) % 7) / 7.0).astype(V.DTYPES[dtype_name])
    cases = [("L2DistLoss()", True), ("L1HingeLoss()", False), ("L1HingeLoss()", True), ("ZeroOneLoss()", False)]
    for spec, weighted in cases:
        opts = Options(elementwise_loss=spec, **V.OPSETS[opset])
        make = (lambda X, y: Dataset(X, y, weights=w)) if weighted else None
        for bad in (0, n - 1):
            asserted += _rule_a(opset, dtype_name, n, bad, lambda tb, ds: eval_loss_batch(tb, ds, opts), (spec, weighted),
                                make=make)
    assert asserted == len(cases) * 2 * _n_verdicts(opset)


@both
@sets
def test_expression_loss(opset, dtype_name):
    opts = Options(elementwise_loss="loss(p, t) = abs(p - t) + 0.5 * square(p - t)", **V.OPSETS[opset])
    asserted = sum(_rule_a(opset, dtype_name, n, bad, lambda tb, ds: eval_loss_batch(tb, ds, opts), "expression loss")
                   for n, bad in ((65, 64), (N_TILES, N_TILES - 1)))
    assert asserted == 2 * _n_verdicts(opset)


# ------------------------------------------------------------------------------------------- builds and knobs
@pytest.mark.parametrize("view", ["full", "rows"])
@both
@sets
def test_every_reachable_build(opset, dtype_name, view):
    """Register-stack and LDS-stack builds and the rows-per-lane variants through the knob table, as
    test_gpu_build_table.py reaches them; "max_row_blocks" 1 (the launch writes the results) and 512 (a tile per row
    block, a reduce launch follows).  The deep wrapper's forms need the LDS stack at every setting."""
    T = V.DTYPES[dtype_name]
    opts = V.options(opset)
    n, bad = N_TILES, N_TILES - 1
    cases = _knob_cases("plain", T, opset == "basic", view == "full")
    idx = np.concatenate([np.random.default_rng(7).permutation(n - 1), [bad]]).astype(np.int64)
    make = (lambda X, y: SubDataset(Dataset(X, y), idx)) if view == "rows" else None
    ctx = sr_amd.get_context()
    asserted = 0
    try:
        for rpl, vstk, mrb in cases:
            ctx.set_tuning("rows_per_lane", rpl)
            ctx.set_tuning("vstk_rows", vstk)
            ctx.set_tuning("max_row_blocks", mrb)
            asserted += _rule_a(opset, dtype_name, n, bad, lambda tb, ds: eval_loss_batch(tb, ds, opts),
                                f"rows_per_lane={rpl} vstk_rows={vstk} max_row_blocks={mrb}", make=make)
    finally:
        for name, value in DEFAULTS.items():
            ctx.set_tuning(name, value)
    assert asserted == len(cases) * _n_verdicts(opset)


@both
@sets
def test_one_tile_per_row_block(monkeypatch, opset, dtype_name):
    """SR_AMD_MAX_ROW_BLOCKS above the tile count, in a fresh context: the flag of a row in the last tile alone
    comes through the per-row-block partials and their reduce."""
    opts = V.options(opset)
    monkeypatch.setenv("SR_AMD_MAX_ROW_BLOCKS", "65536")
    ctx = sr_amd.device.DeviceContext(0)  # reads the environment at creation
    try:
        score = lambda tb, ds: eval_loss_batch(tb, ds, opts, ctx=ctx)  # noqa: E731
        asserted = sum(_rule_a(opset, dtype_name, N_TILES, bad, score, "row blocks")
                       for bad in (0, N_TILES - 1))
    finally:
        ctx.close()
    assert asserted == 2 * _n_verdicts(opset)


def _listed_info(ctx):
    """sr_last_phase_ms out[16..18]: listed loss launches, their listed and their excluded positions."""
    out = (ctypes.c_double * 19)()
    _lib.check(_lib.lib.sr_last_phase_ms(ctx.handle, out, 19))
    return dict(listed=int(out[16]), live=int(out[17]), excl=int(out[18]), path=ctx.last_ref_fold()["path"])


@pytest.mark.parametrize("stress", [0, 1])
def test_dead_tree_probe_and_listed_launch(stress):
    """The dead-tree probe and the listed loss launch ("loss_compact") at test_gpu_loss_compact.py's shape, the
    smallest at which they run: Float32, the BASIC set, 2^18 rows, one chunk of more than 512 trees (group "L" four
    times), the bad row last.  Three settings: probe before every chunk with the list, the same without the list,
    and no probe (so no list).  With the stress rows off the probe runs the first row tiles only and cannot see the
    bad row: every register-stack tree is on the list (none excluded) and the verdict is the listed launch's own.
    With them on, x1 = 1000 / -1 is x1's extreme row: the probe marks the trees and the list leaves them out
    (excluded > 0, which also shows that the probe ran); on the control nothing is excluded."""
    T, dtype_name = np.float32, "float32"
    opts = V.options("basic")
    n = 1 << 18
    bad = n - 1
    data = V.rule_a_data(n, T, bad)
    ctx = sr_amd.get_context()
    asserted = 0
    try:
        ctx.set_tuning("stress_probe", stress)
        for group, copies in (("E", 1), ("L", 4)):
            forms = V.rule_a_forms("basic", group) * copies
            tb = V.rule_a_batch("basic", group, dtype_name)
            tb = tb.take(np.tile(np.arange(tb.n_trees), copies))
            n_deep = sum(f.wrapper == "deep" for f in forms)  # (the LDS-stack launch beside the list)
            assert tb.n_trees - n_deep >= 512
            for which in (group, "control"):
                ds = Dataset(data[which], np.zeros(n, dtype=T))
                try:
                    for probe, listed in ((1, 1), (1, 0), (0, 1)):
                        ctx.set_tuning("probe", probe)
                        ctx.set_tuning("loss_compact", listed)
                        loss, comp = _twice(lambda: eval_loss_batch(tb, ds, opts))
                        info = _listed_info(ctx)
                        what = ("probe / list", stress, group, which, probe, listed, info)
                        asserted += _assert_flags(forms, loss, comp, which == "control", what)
                        assert info["path"] == 2, what
                        if probe and listed:
                            assert info["listed"] >= 1 and info["live"] + info["excl"] == tb.n_trees - n_deep, what
                            if stress and which != "control":
                                assert info["excl"] > 0, what
                            else:
                                assert info["excl"] == 0, what
                        else:
                            assert info["listed"] == 0 and info["live"] == 0 and info["excl"] == 0, what
                finally:
                    ds.free_device()
    finally:
        ctx.set_tuning("probe", 2)
        ctx.set_tuning("loss_compact", 1)
        ctx.set_tuning("stress_probe", 1)
    assert asserted == 6 * (len(V.rule_a_forms("basic", "E")) + 4 * len(V.rule_a_forms("basic", "L")))


@pytest.mark.parametrize("probe", [0, 1])
def test_dead_tree_probe_float64(probe):
    """Float64 has no listed launch and no counter that says the probe ran; 40,000 rows are 156 row blocks of the 16
    the probe asks for (test_dead_tree_probe_is_invisible's size).  The flags with the probe off and on."""
    opts = V.options("basic")
    n = 40000
    ctx = sr_amd.get_context()
    try:
        ctx.set_tuning("probe", probe)
        asserted = sum(_rule_a("basic", "float64", n, bad, lambda tb, ds: eval_loss_batch(tb, ds, opts), ("probe", probe))
                       for bad in (0, n - 1))
    finally:
        ctx.set_tuning("probe", 2)
    assert asserted == 2 * _n_verdicts("basic")


@both
@pytest.mark.parametrize("view", ["full", "rows"])
def test_derived_columns_on_and_off(dtype_name, view):
    """exp(x1) and log(x1) from the call's derived columns (LOAD_DERIVED) and evaluated in every tree: the producer
    itself is the derived column.  A call chooses columns from 16,384 rows and 2^25 trees x rows on (sr_plan.h):
    32,833 rows, group "L" repeated 8 times."""
    T = V.DTYPES[dtype_name]
    opts = V.options("basic")
    n = 32768 + 65
    bad = n - 1
    idx = np.concatenate([np.random.default_rng(9).permutation(n - 1), [bad]]).astype(np.int64)
    data = V.rule_a_data(n, T, bad)
    ctx = sr_amd.get_context()
    asserted = 0
    try:
        for group, copies in (("E", 1), ("L", 8)):
            forms = V.rule_a_forms("basic", group) * copies
            tb = V.rule_a_batch("basic", group, dtype_name)
            tb = tb.take(np.tile(np.arange(tb.n_trees), copies))
            assert tb.n_trees * n >= 1 << 25
            for which in (group, "control"):
                ds = Dataset(data[which], np.zeros(n, dtype=T))
                target = SubDataset(ds, idx) if view == "rows" else ds
                try:
                    for on in (1, 0):
                        ctx.set_tuning("derived", on)
                        loss, comp = _twice(lambda: eval_loss_batch(tb, target, opts))
                        used = ctx.last_derived_columns()
                        assert (used >= 1) if on else (used == 0), (group, which, on, used)
                        what = ("derived", on, view, dtype_name, group, which)
                        asserted += _assert_flags(forms, loss, comp, which == "control", what)
                finally:
                    ds.free_device()
    finally:
        ctx.set_tuning("derived", 1)
    assert asserted == 4 * (len(V.rule_a_forms("basic", "E")) + 8 * len(V.rule_a_forms("basic", "L")))


# ------------------------------------------------------------------------------------------- the other entry points
@both
@sets
def test_views_each_get_their_own_verdict(opset, dtype_name):
    """eval_loss_batch_views: every form twice, once on a view that holds the bad row and once on one that does not."""
    opts = V.options(opset)
    T = V.DTYPES[dtype_name]
    n, bad = N_TILES, N_TILES - 1
    rows = np.random.default_rng(3).permutation(n - 1)[:2047].astype(np.int64)
    view_rows = np.stack([np.concatenate([rows, [bad]]), np.concatenate([rows, [bad - 1]])])
    data = V.rule_a_data(n, T, bad)
    asserted = 0
    for group in ("E", "L"):
        tb, forms = V.rule_a_batch(opset, group, dtype_name), V.rule_a_forms(opset, group)
        nt = tb.n_trees
        two = tb.take(np.concatenate([np.arange(nt), np.arange(nt)]))
        tree_view = np.concatenate([np.zeros(nt, dtype=np.int32), np.ones(nt, dtype=np.int32)])
        ds = Dataset(data[group], np.zeros(n, dtype=T))
        try:
            loss, comp = _twice(lambda: eval_loss_batch_views(two, ds, opts, tree_view, view_rows))
        finally:
            ds.free_device()
        asserted += _assert_flags(forms, loss[:nt], comp[:nt], False, ("views", opset, dtype_name, group, "bad"))
        asserted += _assert_flags(forms, loss[nt:], comp[nt:], True, ("views", opset, dtype_name, group, "clean"))
    assert asserted == _n_verdicts(opset, ("E", "L"))


@functools.lru_cache(maxsize=None)
def _oracle_predictions(opset, group, dtype_name, n):
    """The oracle's control predictions and their spread under +-1 ulp libm perturbations: computed once."""
    T = V.DTYPES[dtype_name]
    X = V.rule_a_data(n, T, 0)["control"]
    tb = V.rule_a_batch(opset, group, dtype_name)
    orc = Oracle.from_options(V.options(opset))
    out, spread = np.empty((tb.n_trees, n)), np.zeros((tb.n_trees, n))
    for k in range(tb.n_trees):
        o, c = orc.eval_tree_array(tb, k, X)
        assert c, V.rule_a_forms(opset, group)[k]
        out[k] = o
        for seed in PERTURB_SEEDS:
            p, _ = orc.eval_tree_array(tb, k, X, perturb=seed)
            with np.errstate(invalid="ignore"):
                d = np.abs(p.astype(np.float64) - out[k])
            spread[k] = np.maximum(spread[k], np.where(np.isfinite(d), d, np.inf))  # (sqrt(e - e) under a perturbed e)
    return out, spread


@both
@sets
def test_predictions_early_exit(opset, dtype_name):
    """eval_tree_array_batch (PRED: per-node checks, early exit): the flags at every size; the controls' predictions
    at 65 rows within test_predictions_vs_oracle's bar (1e-4 relative + 1e-6, or 4 x the row's libm spread)."""
    opts = V.options(opset)

    def score(tb, ds):
        out, comp = eval_tree_array_batch(tb, ds, opts)
        # the flag's companion here is the prediction, not a loss: +Inf stands for "incomplete" in _assert_flags; the
        # complete trees' predictions are the third array _twice compares (an early exit leaves the rest unwritten)
        return np.where(comp, 0.0, np.inf), comp, np.where(comp[:, None], out, 0)

    asserted = sum(_rule_a(opset, dtype_name, n, bad, score, "PRED") for n, bad in SIZES)
    assert asserted == len(SIZES) * _n_verdicts(opset)
    T = V.DTYPES[dtype_name]
    X = V.rule_a_data(65, T, 0)["control"]
    compared = 0
    for group in ("E", "L"):
        want, spread = _oracle_predictions(opset, group, dtype_name, 65)
        ds = Dataset(X)
        try:
            out, comp = eval_tree_array_batch(V.rule_a_batch(opset, group, dtype_name), ds, opts)
        finally:
            ds.free_device()
        assert comp.all()
        tol = np.maximum(1e-4 * np.abs(want) + 1e-6, 4 * spread)
        assert np.isfinite(out).all()
        bad = np.nonzero(~(np.abs(out.astype(np.float64) - want) <= tol).all(axis=1))[0]
        assert len(bad) == 0, [(V.rule_a_forms(opset, group)[k].expr) for k in bad[:6]]
        compared += len(want)
    assert compared == _n_verdicts(opset, ("E", "L")) // 2


@both
def test_parametric_trees(dtype_name):
    """p1 stands for x1 and p2 for x3; class 2 holds the trigger and is present on exactly one row (control: on
    none)."""
    T = V.DTYPES[dtype_name]
    opts = V.options("full")
    asserted = 0
    for n, bad in ((65, 64), (N_TILES, 0), (N_TILES, N_TILES - 1)):
        X = V.rule_a_data(n, T, bad)["control"]
        y = np.zeros(n, dtype=T)
        for group in V.GROUPS:
            ext, forms = V.rule_a_batch("full", group, dtype_name, parametric=True), V.rule_a_forms("full", group)
            tb = to_parametric(ext, V.NF, V.rule_a_params(group, T))
            for with_bad in (True, False):
                cls = np.ones(n, dtype=np.int32)
                if with_bad:
                    cls[bad] = 2
                ds = Dataset(X, y, extra={"class": cls}, n_classes=2)
                try:
                    loss, comp = _twice(lambda: eval_loss_batch(tb, ds, opts))
                    pcomp = eval_tree_array_batch(tb, ds, opts)[1]
                finally:
                    ds.free_device()
                complete = not with_bad and group != "K"
                asserted += _assert_flags(forms, loss, comp, complete, ("parametric", dtype_name, n, bad, group, with_bad))
                assert np.array_equal(pcomp, comp), ("parametric PRED", dtype_name, n, group, with_bad)
    assert asserted == 3 * _n_verdicts("full")


# forms whose control has no finite gradient under dual arithmetic (validity_util.singular_controls): sqrt(0 * P) and
# sqrt(P - P) (sqrt' at 0), (0 * P) ^ y and (P - P) ^ y with a fractional y (y 0^(y - 1)), where a constant is present
N_SINGULAR = {"basic": 6, "grad": 22}


@both
@pytest.mark.parametrize("opset", ["basic", "grad"])
def test_gradients(opset, dtype_name):
    """eval_grad_batch: an incomplete tree has loss +Inf and an all-zero gradient; a control a finite gradient, but for
    the N_SINGULAR forms whose derivative is infinite at the producer's benign value 0.  The catalog less gamma, which
    has no gradient rule."""
    opts = V.options(opset)
    grads = {}

    def score(tb, ds):
        loss, g, comp = eval_grad_batch(tb, ds, opts)
        grads["last"] = (np.asarray(g), tb.constant_offsets())
        return loss, comp, g

    T = V.DTYPES[dtype_name]
    asserted = 0
    assert sum(int(V.singular_controls(opset, g).sum()) for g in ("E", "L")) == N_SINGULAR[opset]
    for n, bad in ((65, 64), (N_TILES, N_TILES - 1)):
        data = V.rule_a_data(n, T, bad)
        for group in V.GROUPS:
            tb, forms = V.rule_a_batch(opset, group, dtype_name), V.rule_a_forms(opset, group)
            singular = V.singular_controls(opset, group)
            for which in (group, "control"):
                ds = Dataset(data[which], np.zeros(n, dtype=T))
                try:
                    loss, comp = _twice(lambda: score(tb, ds))
                finally:
                    ds.free_device()
                complete = which == "control" and group != "K"
                asserted += _assert_flags(forms, loss, comp, complete, ("grad", opset, dtype_name, n, group, which))
                g, offs = grads["last"]
                assert offs[-1] > 0
                per_tree = [g[offs[k]:offs[k + 1]] for k in range(tb.n_trees)]
                if complete:
                    wrong = [forms[k].expr for k, v in enumerate(per_tree) if not np.isfinite(v).all() and not singular[k]]
                else:
                    wrong = [forms[k].expr for k, v in enumerate(per_tree) if v.any()]
                assert not wrong, ("grad", opset, dtype_name, n, group, which, len(wrong), wrong[:6])
    assert asserted == 2 * _n_verdicts(opset)


@both
def test_constant_optimisation_leaves_incomplete_trees_alone(dtype_name):
    """optimize_constants_batch: an incomplete tree keeps its constants bit for bit and is not "improved".  Groups "E"
    and "L", where the data makes the tree incomplete; a restart can move group "K"'s constant producer (exp(1000.0))
    into range, which is an improvement."""
    T = V.DTYPES[dtype_name]
    opts = V.options("grad")
    n, bad = 65, 64
    data = V.rule_a_data(n, T, bad)
    kept = 0
    for group in ("E", "L"):
        tb = V.rule_a_batch("grad", group, dtype_name)
        ds = Dataset(data[group], np.zeros(n, dtype=T))
        try:
            runs = [optimize_constants_batch(tb, ds, opts, np.random.default_rng(0), iterations=2, nrestarts=1)
                    for _ in range(2)]
            new, loss, improved, _ = runs[0]
            assert np.array_equal(_bits(new.get_constants()), _bits(runs[1][0].get_constants()))
            assert np.array_equal(_bits(loss), _bits(runs[1][1])) and np.array_equal(improved, runs[1][2])
        finally:
            ds.free_device()
        assert not improved.any() and np.all(np.isposinf(loss)), (group, int(improved.sum()))
        assert np.array_equal(_bits(new.get_constants()), _bits(tb.get_constants())), group
        kept += tb.n_trees
    assert kept == len(V.rule_a_forms("grad", "E")) + len(V.rule_a_forms("grad", "L"))


# ------------------------------------------------------------------------------------------- rule B
@pytest.mark.parametrize("view", ["full", "rows"])
@pytest.mark.parametrize("n", [1153, N_TILES])
@both
@sets
def test_rule_b_checked_arrays(opset, dtype_name, n, view):
    """Sums that overflow, in every role DynamicExpressions gives an array: the flag alone (such a tree's loss may
    itself overflow).  With the BASIC set the verdicts come from the deferred checks and the exact-sum pass; with the
    catalog, from the per-node checks.  Both ends of "max_row_blocks"."""
    T = V.DTYPES[dtype_name]
    opts = V.options(opset)
    tb, want = V.rule_b_batch(opset, dtype_name, n)
    forms = V.rule_b_forms(opset, dtype_name, n)
    ds = Dataset(V.rule_b_data(n, T), np.zeros(n, dtype=T))
    target = ds if view == "full" else SubDataset(ds, np.random.default_rng(n).permutation(n).astype(np.int64))
    ctx = sr_amd.get_context()
    calls = 0
    try:
        for mrb in (1, 512):
            ctx.set_tuning("max_row_blocks", mrb)
            loss, comp = _twice(lambda: eval_loss_batch(tb, target, opts))
            wrong = [(forms[k][0], bool(comp[k])) for k in np.nonzero(comp != want)[0]]
            assert not wrong, (opset, dtype_name, n, view, mrb, wrong)
            assert np.all(np.isposinf(loss[~comp]))
            if opset == "basic":
                assert ctx.last_exact_trees() > 0  # (the exact-sum pass decided some of them)
            pcomp = eval_tree_array_batch(tb, target, opts)[1]
            assert np.array_equal(pcomp, want), [(forms[k][0], bool(pcomp[k])) for k in np.nonzero(pcomp != want)[0]]
            calls += 1
    finally:
        ctx.set_tuning("max_row_blocks", DEFAULTS["max_row_blocks"])
        ds.free_device()
    assert calls == 2 and len(want) == len(forms) >= 40
