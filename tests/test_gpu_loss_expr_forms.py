"""GPU: every instruction form of the expression-loss program (csrc/sr_loss_expr.h) per element, on every
expression-loss tile build and gradient width.

test_loss_expr_forms_host.py's table (loss_expr_points.py: the fixed bodies, whose coverage of the instruction
kinds, DX / DY flags, leaf sources and 1-4 live values is asserted there, and 60 seeded random ones) against the same
exact reference (fractions.Fraction, central-difference derivative), in both dtypes and both tiers:

  * ``device_elements``: L and dL/dp per point through one-row views (the gathered builds) equal the reference bit
    for bit — values with the sign of a zero, a zero derivative by value;
  * ``device_mean``: the same points as one plain 1153-row dataset (the non-gathered builds; two full tiles of the
    widest build and a ragged tail, the point list rotated so every row slot of a lane holds distinct values) within
    tolerances derived from the documented accumulation (loss_expr_points.mean_tolerances), not measured;
  * ``last_rows_per_lane`` after those calls: 8 / 4 (Float32 BASIC / FULL) and 4 / 2 (Float64), gathered and full —
    all eight tile builds ran;
  * ``t ^ p`` at t = 0 (and its weighted twin): value 0, derivative exactly 0;
  * ``square(p - t)`` under trees with 1, 2, 3, 5, 9 and 17 constants: every gradient entry equals the one-constant
    tree's bit for bit, on one-row views and on the full dataset, and all five tangent buckets had items.
"""
import numpy as np
import pytest

import loss_expr_points as lp
from op_values_util import bits
from sr_amd import Dataset, Options, eval_grad_batch, eval_grad_batch_views, flatten_trees, get_context, parse_expression
from test_loss_expr_forms_host import POW_CASES, assert_elements

pytestmark = pytest.mark.gpu

DTYPES = {"float32": np.float32, "float64": np.float64}
ROWS_PER_LANE = {("float32", "BASIC"): 8, ("float32", "FULL"): 4, ("float64", "BASIC"): 4, ("float64", "FULL"): 2}
N_CHUNKS = 4


def _chunk(c):
    return lp.table()[c::N_CHUNKS]


@pytest.fixture(scope="module")
def refs():
    pts = lp.points()
    return {body: lp.reference(body, pts) for body in lp.table()}


@pytest.fixture(scope="module")
def elements():
    """device_elements per (body, dtype, tier), computed once and shared by the two tests that need it."""
    cache = {}

    def get(body, dname, tier):
        if (body, dname, tier) not in cache:
            p, t, w = lp.arrays(lp.points(), DTYPES[dname])
            cache[body, dname, tier] = lp.device_elements(body, p, t, w, DTYPES[dname], tier)
        return cache[body, dname, tier]

    return get


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("tier", lp.TIERS)
@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_device_elements_equal_the_exact_reference(chunk, tier, dname, refs, elements):
    for body in _chunk(chunk):
        val, der, comp = elements(body, dname, tier)
        assert comp.all(), (body, comp)
        assert_elements(body, DTYPES[dname], val, der, *refs[body])


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("tier", lp.TIERS)
@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_full_view_equals_the_mean_of_the_elements(chunk, tier, dname, elements):
    dtype = DTYPES[dname]
    p, t, w = lp.arrays(lp.points(), dtype)
    idx = lp.full_rows(len(p))
    worst = (0.0, 0.0)
    for body in _chunk(chunk):
        val, der, _ = elements(body, dname, tier)
        weighted = lp.uses_w(lp.parse(body))
        mean, tol_l, gmean, tol_g = lp.mean_tolerances(val.astype(np.float64)[idx], der.astype(np.float64)[idx], w[idx],
                                                       weighted, dtype)
        loss, g, rows = lp.device_mean(body, p, t, w, dtype, tier)
        assert rows == ROWS_PER_LANE[dname, tier], (body, rows)
        el, eg = abs(float(loss) - mean), abs(float(g) - gmean)
        worst = (max(worst[0], el / tol_l), max(worst[1], eg / tol_g if tol_g else 0.0))
        assert el <= tol_l, (body, dname, tier, "loss", float(loss), mean, el, tol_l)
        assert eg <= tol_g, (body, dname, tier, "gradient", float(g), gmean, eg, tol_g)
    print(f"chunk {chunk} {tier} {dname}: worst |loss - mean| / tol {worst[0]:.3g}, |g - mean| / tol {worst[1]:.3g}")


@pytest.mark.parametrize("dname", list(DTYPES))
def test_all_eight_tile_builds_run(dname):
    """BASIC and FULL, gathered (one-row views) and full view: the rows per lane of each build."""
    dtype = DTYPES[dname]
    p, t, w = lp.arrays(lp.points(), dtype)
    ctx = get_context()
    body = "abs(p) - (abs(p - t) * abs(p + t))"
    for tier in lp.TIERS:
        ds, _ = lp._dataset(body, p, t, w)
        try:
            lp._one_row_values(body, ds, len(p), dtype, tier)
            assert ctx.last_rows_per_lane() == ROWS_PER_LANE[dname, tier], ("gathered", tier)
        finally:
            ds.free_device()
        assert lp.device_mean(body, p, t, w, dtype, tier, deriv=False)[2] == ROWS_PER_LANE[dname, tier], ("full", tier)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("tier", lp.TIERS)
@pytest.mark.parametrize("body,weighted", POW_CASES)
def test_zero_base_power_has_a_zero_derivative(body, weighted, tier, dname):
    """pa = +Inf at a zero base; DX is clear, so it never meets the zero tangent (test_loss_expr_forms_host.py)."""
    dtype = DTYPES[dname]
    val, der, comp = lp.device_elements(body, np.array([0.5]), np.array([0.0]), np.array([2.0]), dtype, tier)
    assert comp.all() and val[0] == 0 and not np.signbit(val[0]) and der[0] == 0, (body, val, der, comp)


WIDTHS = (1, 2, 3, 5, 9, 17)  # constants per tree: the 1, 2, 4, 8 and 16-tangent buckets and the second window


@pytest.mark.parametrize("dname", list(DTYPES))
def test_tangent_widths_agree_bit_for_bit(dname):
    dtype = DTYPES[dname]
    opts = Options(elementwise_loss="loss(p, t) = square(p - t)", **lp.tier_operators("BASIC"))
    trees = [parse_expression(" + ".join(["x1"] + ["0.0"] * k), opts) for k in WIDTHS]
    p, t, w = lp.arrays(lp.points(), dtype)
    n = len(p)
    ctx = get_context()

    def check(g, so, n_sets, what):
        for s in range(n_sets):
            first = g[so[s * len(WIDTHS)]]
            assert np.isfinite(first) and first != 0
            for j, k in enumerate(WIDTHS):
                e = g[so[s * len(WIDTHS) + j]:so[s * len(WIDTHS) + j + 1]]
                assert e.shape == (k,) and np.all(bits(e) == bits(np.array([first], dtype=dtype))[0]), (what, s, k, e, first)
        info = ctx.last_grad_info()
        assert [b["kt"] for b in info] == [1, 2, 4, 8, 16] and all(b["items"] > 0 for b in info), (what, info)

    # one-row views: the six trees on every point
    ds = Dataset(np.ascontiguousarray(p[None, :]), t)
    try:
        tb = flatten_trees(trees * n, dtype)
        _, g, comp = eval_grad_batch_views(tb, ds, opts, np.repeat(np.arange(n, dtype=np.int32), len(WIDTHS)),
                                           np.arange(n, dtype=np.int64)[:, None])
        assert comp.all()
        check(g, tb.scalar_offsets(), n, "one-row views")
        want = (2 * (p.astype(np.float64) - t.astype(np.float64))).astype(dtype)  # exact in T
        assert np.array_equal(g[tb.scalar_offsets()[:-1:len(WIDTHS)]], want)
    finally:
        ds.free_device()
    # the full dataset
    idx = lp.full_rows(n)
    ds = Dataset(np.ascontiguousarray(p[idx][None, :]), np.ascontiguousarray(t[idx]))
    try:
        tb = flatten_trees(trees, dtype)
        _, g, comp = eval_grad_batch(tb, ds, opts)
        assert comp.all()
        check(g, tb.scalar_offsets(), 1, "full view")
    finally:
        ds.free_device()
