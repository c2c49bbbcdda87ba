"""GPU: every build of the tile kernel a scoring call's knobs can reach, against the oracle.

Which build of ``sr_tile_kernel`` a launch runs follows from the call's family (plain, parametric, expression
loss), element type, operator tier, loss, view and the "rows_per_lane" / "vstk_rows" knobs (csrc/sr_builds.h:
the table of builds and sr_resolve_build).  This walks that space at the smallest shape with two full tiles and
a ragged one for every rows-per-lane count: 4,097 rows (2 x 64 x 32 + 1), 3 features, six trees — one that
fits the register stack, one that needs the LDS stack, one that is non-finite on the ragged tile's only row,
three ordinary ones.  Each call: complete flags equal to the oracle's, incomplete trees Inf, every complete
tree within the parity tests' bar for its dtype and family.

The library before the build table fails three of the 72 cases, plain Float32 BASIC over the row view (L2, L1,
Logit), at "rows_per_lane" 4 with one row block: it planned the launch and the stored-loss layout at 4 rows per
lane and ran the one gathered build at 8, whose last tile of a position wrote its 256 padding zeros over the
next position's first rows.  Four of the five complete trees came out 7-8 % low (L2, tree 0: 4.8609 against the
oracle's 5.2457, bar 5.2e-4).  sr_launch_shape now plans a row view at the build's rows per lane (DESIGN.md
§4.8); every other case passes on that library unchanged.
"""
import numpy as np
import pytest

import sr_amd
from loss_expr_util import loss_tolerance_f64
from oracle import Oracle
from parametric_util import compile_info, to_parametric, x_ext
from parity_util import assert_losses_within, loss_tolerance
from sr_amd import Dataset, Options, batch, eval_loss_batch, flatten_trees, parse_expression
from test_gpu_parity import C2_OPTS, FULL_OPTS

pytestmark = pytest.mark.gpu

N, NF, K, NC = 4097, 3, 2, 2
DEEP = ("((cos(x1 * x2) + cos(x2 * x3)) * (cos(x3 * x1) - cos(x1 + x2))) + "
        "((cos(x2 - x3) + cos(x3 + x1)) * (cos(x1 - x3) * cos(x2 + {b})))")
# shallow (<= 2 operand-stack slots), deep (more), non-finite at row 4096 (x3 = -11 there), three ordinary;
# {a}, {b}: a constant in a plain tree, parameters p1 / p2 (leaves x4 / x5 before to_parametric) in a parametric one
TREES = ["(x1 * {a}) + x2", DEEP, "log(x3 + 10.0) * {b}", "cos(x2) * {a} - 0.5", "exp(x3 * 0.3) + {b} * x1",
         "x2 / (x3 * x3 + 1.0) + {a}"]
SHALLOW, DEEP_AT, NONFINITE = 0, 1, 2
# the loss axis: the catalog spec, and the expression that restates it (loss_expr_util.RESTATED)
LOSSES = {"L2": ("L2DistLoss()", "square(p - t)"), "L1": ("L1DistLoss()", "abs(p - t)"),
          "Logit": ("LogitDistLoss()", "-log(4.0) - (p - t) + 2.0*log(1.0 + exp(p - t))")}
DEFAULTS = {"rows_per_lane": 0, "vstk_rows": 0, "max_row_blocks": 512}


def _data(dtype):
    rng = np.random.default_rng(4097)
    X = rng.standard_normal((NF, N)).astype(dtype)
    X[2, N - 1] = -11.0  # log(x3 + 10) is NaN on the ragged tile's row alone
    cls = rng.integers(1, NC + 1, size=N).astype(np.int32)
    y = (2 * np.cos(X[2].astype(np.float64)) + X[0].astype(np.float64) ** 2 - 2 + 0.1 * rng.standard_normal(N)).astype(dtype)
    idx = rng.integers(0, N, size=N)
    idx[-1] = N - 1  # the view keeps the shape and the bad row on its ragged tile
    P = rng.standard_normal((K, NC)).astype(dtype)
    return X, y, cls, idx, P


def _knob_cases(family, dtype, basic, full_view):
    """(rows_per_lane, vstk_rows, max_row_blocks) settings that reach distinct builds or launch sequences; the
    rest of the cross resolves to a build already in the list (sr_resolve_build) and is left out."""
    f32 = dtype == np.float32
    rpls = (0, 4, 8, 16, 32) if f32 else (0, 4, 8)  # (Float64 reads 16 and 32 as 0)
    vstks = (0, 16, 32) if f32 else (0, 8)
    if not basic:  # the FULL tier: one build per view, whatever the knobs
        rpls, vstks = (0, 16), (0,)
    elif family != "plain":  # the classic kernel at its default rows; parametric: one register-stack build
        rpls, vstks = (0, 16) if f32 else (0, 8), (0, vstks[1])
    if not full_view:  # a row view has no register-stack build
        vstks = (0,)
    return [(r, v, m) for r in rpls for v in vstks for m in (1, 512)]


@pytest.mark.parametrize("view", ["full", "rows"])
@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("opset", ["basic", "full"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("family", ["plain", "parametric", "expr"])
def test_every_reachable_build_vs_oracle(family, dtype, opset, loss, view):
    ops = C2_OPTS if opset == "basic" else FULL_OPTS
    catalog = Options(elementwise_loss=LOSSES[loss][0], **ops)
    opts = Options(elementwise_loss=f"loss(p, t) = {LOSSES[loss][1]}", **ops) if family == "expr" else catalog
    X, y, cls, idx, P = _data(dtype)
    sub = {"a": "x4", "b": "x5"} if family == "parametric" else {"a": "1.5", "b": "0.7"}
    ext = flatten_trees([parse_expression(e.format(**sub), catalog) for e in TREES], dtype)
    if family == "parametric":
        tb, Xo, nf_o = to_parametric(ext, NF, P), x_ext(X, P, cls), NF + K
        ds = Dataset(X, y, extra={"class": cls}, n_classes=NC)
    else:
        tb, Xo, nf_o = ext, X, NF
        ds = Dataset(X, y)
    # the trees keep their roles: register stack (<= 2 slots) and LDS stack (more)
    assert compile_info(tb.take([SHALLOW]), catalog, N, NF)[3] <= 2
    assert compile_info(tb.take([DEEP_AT]), catalog, N, NF)[3] > 2
    target = ds if view == "full" else batch(ds, idx)
    Xv, yv = (Xo, y) if view == "full" else (np.ascontiguousarray(Xo[:, idx]), y[idx])
    assert nf_o == Xv.shape[0]
    # the oracle, once per case: the parity tests' bars (an expression-loss call accumulates in f64)
    bar = dict(loss_kind=catalog.loss_kind, loss_param=catalog.loss_param, rel_bar=1e-4 if dtype == np.float32 else 1e-10)
    tol, o_loss, o_comp, _ = (loss_tolerance_f64 if family == "expr" else loss_tolerance)(Oracle.from_options(catalog), ext, Xv, yv, **bar)
    assert not o_comp[NONFINITE] and o_comp[[SHALLOW, DEEP_AT]].all() and o_comp.sum() == len(TREES) - 1
    ctx = sr_amd.get_context()
    try:
        for rpl, vstk, mrb in _knob_cases(family, dtype, opset == "basic", view == "full"):
            what = f"rows_per_lane={rpl} vstk_rows={vstk} max_row_blocks={mrb}"
            ctx.set_tuning("rows_per_lane", rpl)
            ctx.set_tuning("vstk_rows", vstk)
            ctx.set_tuning("max_row_blocks", mrb)  # 1: the launch writes the results; 512: a reduce launch follows
            got, comp = eval_loss_batch(tb, target, opts)
            assert np.array_equal(comp, o_comp), (what, comp, o_comp)
            assert np.all(np.isinf(got[~comp])), what
            assert_losses_within(got, o_loss, comp, tol, what)
    finally:
        for name, value in DEFAULTS.items():
            ctx.set_tuning(name, value)
        ds.free_device()
