"""Per-row derivatives on the device: eval_grad_tree_array / eval_diff_tree_array.

Known answers: the reference derivative test's equations (test/integration/ad/zygote/test_derivatives.jl) against
tests/golden/diff_tree_array.json under that test's own criterion, isapprox(a, b; rtol = 0.1).  The tight pins are
identities: the evaluation is eval_tree_array_batch's; the constants' tangents are the existing gradient kernel's
(one-row views under L1DistLoss with y = -2^100: d loss / d pred = 1, n = 1); a feature's tangent is that of a zero
constant added to it (up to the sign of a zero); eval_diff is a row of eval_grad(variable=True); rows do not depend on the call's shape.

Random trees: the C2 generator (node_count ~ U{1..30}) over the operator catalog less gamma, the one operator
without a derivative rule (validity_util.OPSETS["grad"]).
"""
import json
import os

import numpy as np
import pytest

import sr_amd
from sr_amd import (Dataset, Node, Options, ParametricExpression, SubDataset, UnsupportedOperatorError,
                    eval_diff_tree_array, eval_diff_tree_array_batch, eval_grad_batch_views, eval_grad_tree_array,
                    eval_grad_tree_array_batch, eval_tree_array, eval_tree_array_batch, flatten_trees,
                    gen_random_population, parse_expression)
from validity_util import OPSETS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = [np.float32, np.float64]
ULP_LOG = os.path.join(os.path.dirname(HERE), "profiles", "diff_tree_array_ulp.txt")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def isapprox(a, b, rtol=0.1):
    """Julia's isapprox for arrays: the 2-norm of the difference against rtol times the larger 2-norm."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.linalg.norm(a - b) <= rtol * max(np.linalg.norm(a), np.linalg.norm(b)))


# ------------------------------------------------------------------ known answers
@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(HERE, "golden", "diff_tree_array.json")) as f:
        g = json.load(f)
    g["opts"] = Options(binary_operators=g["binary_operators"], unary_operators=g["unary_operators"])
    g["Xf"] = np.array(g["X"], dtype=np.float64) / g["scale"]
    return g


_ulp_lines = {}


def _record_ulp(name, dtype, got, want):
    want = np.asarray(want, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(want == 0, np.abs(got), np.abs(got.astype(np.float64) - want) / np.abs(want))
    _ulp_lines[(name, np.dtype(dtype).name)] = float(rel.max())
    if os.environ.get("SR_WRITE_PROFILES"):  # (the recorded figures: profiles/diff_tree_array_ulp.txt)
        with open(ULP_LOG, "w") as f:
            f.write("# max elementwise relative error of the device derivatives against the 60-digit fixture\n")
            f.write("# (tests/test_gpu_diff_tree_array.py; no bar is set on these)\n")
            for (n, d), v in sorted(_ulp_lines.items()):
                f.write(f"{n} {d} {v:.3e}\n")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["equation1", "equation2", "equation3"])
def test_known_answers_features(fixture, name, dtype):
    case = next(c for c in fixture["cases"] if c["name"] == name)
    opts = fixture["opts"]
    X = fixture["Xf"].astype(dtype)
    tree = parse_expression(case["expr"], opts)
    want = np.array(case["d_feature"])
    out, grad, comp = eval_grad_tree_array(tree, X, opts, variable=True)
    assert comp and grad.shape == (3, X.shape[1]) and grad.dtype == dtype
    stacked = np.stack([eval_diff_tree_array(tree, X, opts, i)[1] for i in (1, 2, 3)])
    _record_ulp(name, dtype, grad, want)
    print(name, np.dtype(dtype).name, "max rel err", _ulp_lines[(name, np.dtype(dtype).name)])
    assert isapprox(out, case["value"])
    assert isapprox(grad, want)
    assert isapprox(stacked, want)
    assert not isapprox(grad * 0, want)
    assert not isapprox(stacked * 0, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["equation4", "equation5"])
def test_known_answers_constants(fixture, name, dtype):
    case = next(c for c in fixture["cases"] if c["name"] == name)
    opts = fixture["opts"]
    X = fixture["Xf"].astype(dtype)
    tree = parse_expression(case["expr"], opts)
    want = np.array(case["d_constant"])
    _, grad, comp = eval_grad_tree_array(tree, X, opts, variable=False)
    assert comp and grad.shape == want.shape
    _record_ulp(name, dtype, grad, want)
    print(name, np.dtype(dtype).name, "max rel err", _ulp_lines[(name, np.dtype(dtype).name)])
    assert isapprox(grad, want)
    assert not isapprox(grad * 0, want)
    if name == "equation4":  # (C * x1: the derivative with respect to C is x1)
        assert isapprox(grad[0], X[0])


# ------------------------------------------------------------------ random trees, shared
GRAD_OPTS = Options(**OPSETS["grad"])
NF = 3


def _x(nf, n, dtype, seed=3):
    """Positive multiples of 2^-8 (no -0.0 anywhere)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(16, 1024, (nf, n)) / 256.0).astype(dtype)


def _chain(n_consts, nf=NF):
    """A fixed tree with n_consts constants (every tangent width must run)."""
    terms = [f"({0.25 + 0.125 * k} * cos(x{1 + k % nf}))" for k in range(n_consts)]
    return " + ".join(terms)


@pytest.fixture(scope="module", params=[1, 2])
def random_trees(request):
    trees = gen_random_population(300, GRAD_OPTS, NF, seed=request.param)
    trees += [parse_expression(_chain(k), GRAD_OPTS) for k in (1, 2, 3, 5, 9, 17)]
    return trees


@pytest.mark.parametrize("dtype", DTYPES)
def test_evaluation_is_eval_tree_array(random_trees, dtype):
    """`evaluation` and the value part of `complete` are eval_tree_array_batch's, bit for bit: 300 random trees
    x 333 rows (+ the fixed trees)."""
    ds = Dataset(_x(NF, 333, dtype))
    tb = flatten_trees(random_trees, dtype)
    ref, rcomp = eval_tree_array_batch(tb, ds, GRAD_OPTS)
    for variable in (False, True):
        out, grads, comp = eval_grad_tree_array_batch(tb, ds, GRAD_OPTS, variable=variable)
        assert same_bits(out, ref)
        # the value part of the flag: never complete where the value is not, and with no constants (nothing
        # that could be non-finite) exactly eval_tree_array's
        assert not np.any(comp & ~rcomp)
        if not variable:
            none = np.diff(tb.constant_offsets()) == 0
            assert np.array_equal(comp[none], rcomp[none])
        for t in np.flatnonzero(~comp):
            assert not grads[t].any()
        for t in np.flatnonzero(comp):
            assert np.isfinite(grads[t]).all()
    out, diff, comp = eval_diff_tree_array_batch(tb, ds, GRAD_OPTS, np.ones(tb.n_trees, np.int32))
    assert same_bits(out, ref) and not np.any(comp & ~rcomp)


@pytest.mark.parametrize("dtype", DTYPES)
def test_constants_equal_the_gradient_kernel(random_trees, dtype):
    """variable=False against sr_eval_grad_batch_views: one-row views, L1DistLoss, y = -2^100 (d loss / d pred = 1,
    n = 1), so that call's gradient entries are d pred / d c of the row.  Bit for bit, except that the gradient
    kernel's f64 accumulator starts at +0.0 and so returns +0.0 for a tangent of -0.0."""
    n = 64
    X = _x(NF, n, dtype)
    ds = Dataset(X, np.full(n, -2.0 ** 100, dtype=dtype))
    opts = Options(**OPSETS["grad"], elementwise_loss="L1DistLoss")
    tb = flatten_trees(random_trees, dtype)
    _, grads, comp = eval_grad_tree_array_batch(tb, ds, opts, variable=False)
    nc = np.diff(tb.constant_offsets())
    pick = [t for t in range(tb.n_trees) if comp[t] and nc[t] > 0]
    for k in (1, 2, 3, 5, 9, 17):
        assert any(nc[t] == k for t in pick), k
    sub = tb.take(np.repeat(pick, n))
    tree_view = np.tile(np.arange(n, dtype=np.int32), len(pick))
    view_rows = np.arange(n, dtype=np.int64).reshape(n, 1)
    _, g, c = eval_grad_batch_views(sub, ds, opts, tree_view, view_rows)
    off = sub.constant_offsets()
    for i, t in enumerate(pick):
        # a tree complete over the 64 rows is complete on each of them (a one-row view's checks see that row's
        # finite values only, and |pred + 2^100| is finite), so every picked tree is compared
        assert c[i * n:(i + 1) * n].all(), t
        got = grads[t]
        want = np.stack([g[off[i * n + r]:off[i * n + r + 1]] for r in range(n)], axis=1)
        zero = (got == 0) & (want == 0)
        assert np.array_equal(bits(np.where(zero, 0, got).astype(dtype)), bits(np.where(zero, 0, want).astype(dtype))), t
    print(np.dtype(dtype).name, "trees with constants and complete, all compared:", len(pick))


def _count_feature(tree, f):
    return sum(1 for nd in tree.preorder() if nd.degree == 0 and not nd.constant and nd.feature == f)


def _shift_feature(tree, f, add_op):
    """tree with every x_f replaced by (x_f + 0.0); returns it and the new constants' pre-order slots."""
    t = tree.copy()
    added = []
    for nd in t.preorder():
        if nd.degree == 0 and not nd.constant and not nd.is_parameter and nd.feature == f:
            c = Node(val=0.0)
            added.append(c)
            nd.set_node(Node(op=add_op, l=Node(feature=f), r=c))
    consts = [nd for nd in t.preorder() if nd.degree == 0 and nd.constant]
    return t, [k for k, nd in enumerate(consts) if any(nd is c for c in added)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nf", [1, 3, 17, 33])
def test_features_equal_zero_constants(nf, dtype):
    """d/dx_f against d/dc of the tree with every x_f replaced by (x_f + c), c = 0.0 (X holds no -0.0, so the values
    are unchanged).  One occurrence: bit for bit up to the sign of a zero (x_g + x_f leaves the other slots' -0.0 as it
    is, while the stack form adds the shifted operand's +0.0 to it).  m > 1 occurrences: the sum of the m constants' derivatives, within
    m eps_T sum|terms| — only the order of m additions differs.  nfeatures 17 and 33 take two and three windows."""
    n = 70
    eps = np.finfo(dtype).eps
    ds = Dataset(_x(nf, n, dtype, seed=nf))
    trees = gen_random_population(80, GRAD_OPTS, nf, seed=10 + nf)
    trees.append(parse_expression(" + ".join(f"(x{f} * x{f})" for f in range(1, nf + 1)), GRAD_OPTS))
    trees.append(parse_expression(" * ".join(f"cos(x{f})" for f in range(nf, 0, -1)), GRAD_OPTS))
    # (the last feature once, as a leaf, as either operand of a basic and of a general binary, beside constants)
    trees += [parse_expression(e.format(f=nf), GRAD_OPTS) for e in (
        "x{f}", "1.5 / x{f}", "x{f} / 1.5", "x{f} ^ 1.5", "1.5 ^ x{f}", "atan2(0.5, x{f})", "cos(0.5 - x{f}) * 2.0",
        "max(x{f}, 1.25) - 0.75")]
    add_op = GRAD_OPTS.operators.binary_index("+")
    _, gfeat, comp = eval_grad_tree_array_batch(trees, ds, GRAD_OPTS, variable=True)
    shifted, where = [], []
    for t, tree in enumerate(trees):
        if not comp[t]:
            continue
        for f in range(1, nf + 1):
            m = _count_feature(tree, f)
            if m == 0:
                assert not gfeat[t][f - 1].any(), (t, f)  # an unused feature: exactly 0 in every row
                continue
            st, slots = _shift_feature(tree, f, add_op)
            assert len(slots) == m
            if st.count_constants() > 128:
                continue
            shifted.append(st)
            where.append((t, f, slots))
    _, gc, comp2 = eval_grad_tree_array_batch(shifted, ds, GRAD_OPTS, variable=False)
    n_single = n_multi = 0
    for k, (t, f, slots) in enumerate(where):
        assert comp2[k], (t, f)
        got = gfeat[t][f - 1]
        terms = gc[k][slots]
        if len(slots) == 1:
            zero = (got == 0) & (terms[0] == 0)
            assert np.array_equal(bits(np.where(zero, 0, got).astype(dtype)),
                                  bits(np.where(zero, 0, terms[0]).astype(dtype))), (t, f)
            n_single += 1
        else:
            tol = len(slots) * eps * np.abs(terms.astype(np.float64)).sum(axis=0)
            err = np.abs(got.astype(np.float64) - terms.astype(np.float64).sum(axis=0))
            assert np.all(err <= tol), (t, f, float((err - tol).max()))
            n_multi += 1
    print("nf", nf, np.dtype(dtype).name, "single", n_single, "multi", n_multi)
    assert n_single >= 8 and n_multi >= 2  # (coverage guards of the draw, the fixed trees included)


@pytest.mark.parametrize("dtype", DTYPES)
def test_diff_is_a_row_of_grad(random_trees, dtype):
    nf = 5  # (the trees use x1..x3: directions 4 and 5 are unused features)
    ds = Dataset(_x(nf, 200, dtype))
    tb = flatten_trees(random_trees, dtype)
    out, grads, comp = eval_grad_tree_array_batch(tb, ds, GRAD_OPTS, variable=True)
    directions = 1 + np.arange(tb.n_trees) % nf
    out2, diff, comp2 = eval_diff_tree_array_batch(tb, ds, GRAD_OPTS, directions)
    assert same_bits(out, out2)
    assert diff.shape == (tb.n_trees, 200)
    n_checked = 0
    for t in range(tb.n_trees):
        if comp[t]:
            assert comp2[t]
            assert same_bits(diff[t], grads[t][directions[t] - 1]), t
            if directions[t] > 3:
                assert not diff[t].any()
            n_checked += 1
    assert n_checked > 100


# ------------------------------------------------------------------ row shapes
@pytest.fixture(scope="module", params=DTYPES, ids=lambda d: np.dtype(d).name)
def big_call(request):
    dtype = request.param
    opts = Options(**OPSETS["grad"])
    trees = gen_random_population(40, opts, NF, seed=21)
    trees += [parse_expression(_chain(k), opts) for k in (1, 2, 4, 8, 17)]
    X = _x(NF, 2100, dtype, seed=5)
    ds = Dataset(X)
    tb = flatten_trees(trees, dtype)
    res = {v: eval_grad_tree_array_batch(tb, ds, opts, variable=v) for v in (False, True)}
    # (trees complete over all 2,100 rows are complete over any of them)
    return dict(dtype=dtype, opts=opts, tb=tb, X=X, ds=ds, res=res)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513, 2049])
def test_row_counts(big_call, n):
    """The first n rows alone give the bits the larger call gives for them: padding rows leak nothing."""
    b = big_call
    ds = Dataset(np.ascontiguousarray(b["X"][:, :n]))
    for v in (False, True):
        out, grads, comp = eval_grad_tree_array_batch(b["tb"], ds, b["opts"], variable=v)
        rout, rgrads, rcomp = b["res"][v]
        assert comp[rcomp].all()
        for t in np.flatnonzero(rcomp):
            assert same_bits(out[t], rout[t, :n])
            assert same_bits(grads[t], np.ascontiguousarray(rgrads[t][:, :n])), (t, v)
    ds.free_device()


def test_gathered_rows(big_call):
    b = big_call
    idx = np.concatenate([np.arange(700, 300, -1), [5, 5, 5, 2099, 0], np.arange(0, 2100, 7)]).astype(np.int64)
    sub = SubDataset(b["ds"], idx)
    for v in (False, True):
        out, grads, comp = eval_grad_tree_array_batch(b["tb"], sub, b["opts"], variable=v)
        rout, rgrads, rcomp = b["res"][v]
        assert comp[rcomp].all()
        for t in np.flatnonzero(rcomp):
            assert same_bits(out[t], np.ascontiguousarray(rout[t, idx]))
            assert same_bits(grads[t], np.ascontiguousarray(rgrads[t][:, idx])), (t, v)


def test_forced_rows_per_lane(big_call):
    b = big_call
    ctx = sr_amd.get_context()
    try:
        for rows in (1, 2, 4, 8):
            ctx.set_tuning("grad_rows", rows)
            for v in (False, True):
                out, grads, comp = eval_grad_tree_array_batch(b["tb"], b["ds"], b["opts"], variable=v)
                rout, rgrads, rcomp = b["res"][v]
                assert np.array_equal(comp, rcomp)
                for t in range(b["tb"].n_trees):
                    assert same_bits(grads[t], rgrads[t]), (rows, t, v)
    finally:
        ctx.set_tuning("grad_rows", 0)


def test_staging_chunks(big_call):
    """The device staging bound ("grad_stage_bytes") splits the work items into chunks; the results do not depend
    on it: one item per chunk (1 byte), a bound that cuts trees between their windows and packs a few items per
    chunk, and the default give the same bits, flags and work-item counts."""
    b = big_call
    ctx = sr_amd.get_context()
    nt = b["tb"].n_trees
    directions = 1 + np.arange(nt) % NF
    ref_diff = eval_diff_tree_array_batch(b["tb"], b["ds"], b["opts"], directions)
    ref_items = {}
    for v in (False, True):
        eval_grad_tree_array_batch(b["tb"], b["ds"], b["opts"], variable=v)
        ref_items[v] = [x["items"] for x in ctx.last_grad_info()]
    item = 2100 * np.dtype(b["dtype"]).itemsize  # one tangent of one tree
    try:
        for stage in (1, 5 * item + 1, 40 * item):
            ctx.set_tuning("grad_stage_bytes", stage)
            for v in (False, True):
                out, grads, comp = eval_grad_tree_array_batch(b["tb"], b["ds"], b["opts"], variable=v)
                rout, rgrads, rcomp = b["res"][v]
                assert same_bits(out, rout) and np.array_equal(comp, rcomp)
                assert [x["items"] for x in ctx.last_grad_info()] == ref_items[v]
                for t in range(nt):
                    assert same_bits(grads[t], rgrads[t]), (stage, t, v)
            out, diff, comp = eval_diff_tree_array_batch(b["tb"], b["ds"], b["opts"], directions)
            assert same_bits(diff, ref_diff[1]) and np.array_equal(comp, ref_diff[2])
    finally:
        ctx.set_tuning("grad_stage_bytes", 256 << 20)


# ------------------------------------------------------------------ completeness
BASIC = Options(binary_operators=["+", "-", "*", "/"], unary_operators=["sqrt", "cos", "exp", "gamma"])
BASIC_NOGAMMA = Options(binary_operators=["+", "-", "*", "/"], unary_operators=["sqrt", "cos", "exp"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_completeness(dtype):
    opts = BASIC_NOGAMMA
    X = _x(2, 130, dtype)
    X0 = X.copy()
    X0[0, 77] = 0.0
    sq = parse_expression("sqrt(x1)", opts)
    # sqrt(x1) with a row at 0: finite values, an infinite derivative
    out, comp = eval_tree_array(sq, X0, opts)
    assert comp
    out2, grad, comp2 = eval_grad_tree_array(sq, X0, opts, variable=True)
    assert not comp2 and not grad.any() and same_bits(out, out2)
    _, d, comp3 = eval_diff_tree_array(sq, X0, opts, 1)
    assert not comp3 and not d.any()
    # (the other direction's tangent at that row is the rule's Inf x 0 = NaN: incomplete as well)
    _, d, comp3 = eval_diff_tree_array(sq, X0, opts, 2)
    assert not comp3 and not d.any()
    _, d, comp3 = eval_diff_tree_array(sq, X, opts, 2)
    assert comp3 and not d.any()
    # ... and without that row
    _, grad, comp2 = eval_grad_tree_array(sq, X, opts, variable=True)
    assert comp2 and np.array_equal(grad[0], (0.5 / np.sqrt(X[0])).astype(dtype)) and not grad[1].any()
    # x1 / x2 with x2 = 0 on a row: incomplete in value already
    Xz = X.copy()
    Xz[1, 3] = 0.0
    div = parse_expression("x1 / x2", opts)
    assert not eval_tree_array(div, Xz, opts)[1]
    _, grad, comp2 = eval_grad_tree_array(div, Xz, opts, variable=True)
    assert not comp2 and not grad.any()
    # a batch mixing them leaves the complete trees' bits unchanged
    good = [parse_expression(e, opts) for e in ("cos(x1) * 1.5 + x2", "exp(x2 * 0.25) / (x1 + 2.0)")]
    ds = Dataset(Xz)
    ds0 = Dataset(X0)
    for v in (False, True):
        _, alone, c_alone = eval_grad_tree_array_batch(good, ds, opts, variable=v)
        _, mixed, c_mixed = eval_grad_tree_array_batch([div, good[0], div, good[1]], ds, opts, variable=v)
        assert c_alone.all() and list(c_mixed) == [False, True, False, True]
        assert same_bits(mixed[1], alone[0]) and same_bits(mixed[3], alone[1])
        assert not mixed[0].any() and not mixed[2].any()
        _, alone, c_alone = eval_grad_tree_array_batch(good, ds0, opts, variable=v)
        _, mixed, c_mixed = eval_grad_tree_array_batch([good[0], sq, good[1]], ds0, opts, variable=v)
        assert list(c_mixed) == [True, not v, True]  # (sqrt(x1) has no constants: nothing to be non-finite)
        assert same_bits(mixed[0], alone[0]) and same_bits(mixed[2], alone[1])


def test_padding_rows_do_not_count():
    """65 rows, the last valid row fine, the tile's padding replicates row 0: a bad derivative at row 0 counts once
    and a view without it is complete."""
    opts = BASIC_NOGAMMA
    X = _x(1, 65, np.float32)
    X[0, 0] = 0.0
    sq = parse_expression("sqrt(x1)", opts)
    ds = Dataset(X)
    assert not eval_grad_tree_array_batch([sq], ds, opts, variable=True)[2][0]
    sub = SubDataset(ds, np.arange(1, 65, dtype=np.int64))
    _, grad, comp = eval_grad_tree_array_batch([sq], sub, opts, variable=True)
    assert comp[0] and np.isfinite(grad[0]).all()


# ------------------------------------------------------------------ refusals
def test_refusals():
    X = _x(2, 10, np.float32)
    with pytest.raises(UnsupportedOperatorError):
        eval_grad_tree_array(parse_expression("gamma(x1)", BASIC), X, BASIC, variable=True)
    with pytest.raises(UnsupportedOperatorError):
        eval_diff_tree_array(parse_expression("gamma(x1)", BASIC), X, BASIC, 1)
    t = parse_expression("cos(x1) + x2", BASIC_NOGAMMA)
    for bad in (0, 3):
        with pytest.raises(ValueError):
            eval_diff_tree_array(t, X, BASIC_NOGAMMA, bad)
        with pytest.raises(ValueError):
            eval_diff_tree_array_batch([t, t], Dataset(X), BASIC_NOGAMMA, [1, bad])
    pe = ParametricExpression(parse_expression("p1 * x1", BASIC_NOGAMMA), np.ones((1, 2)))
    with pytest.raises(NotImplementedError, match="§15"):
        eval_grad_tree_array(pe, X, BASIC_NOGAMMA)
    with pytest.raises(NotImplementedError, match="§15"):
        eval_diff_tree_array(pe, X, BASIC_NOGAMMA, 1)
    # no constants under variable=False: an empty [0, n] gradient, complete as eval_tree_array
    out, grad, comp = eval_grad_tree_array(t, X, BASIC_NOGAMMA, variable=False)
    assert grad.shape == (0, 10) and comp == eval_tree_array(t, X, BASIC_NOGAMMA)[1]
    assert same_bits(out, eval_tree_array(t, X, BASIC_NOGAMMA)[0])


def test_last_grad_info_reports_the_launches():
    ctx = sr_amd.get_context()
    opts = BASIC_NOGAMMA
    trees = [parse_expression(e, opts) for e in ("x1 * 1.5", "cos(x1 * 0.5) + 2.0 * x2", "x1")]
    eval_grad_tree_array_batch(trees, Dataset(_x(2, 100, np.float32)), opts, variable=False)
    info = ctx.last_grad_info()
    items = [b["items"] for b in info]
    assert items == [1, 1, 0, 0, 0]
