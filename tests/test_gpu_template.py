"""GPU: TemplateExpression candidates on the device: the reference's known answers, identity
with the hand-composed tree through the existing calls, guards, tied gradients against the untied sum, frozen
literals, tied optimisation against its closed form, category-indexed parameters, and the refusals.
"""

import numpy as np
import pytest

import sr_amd
import sr_amd.distributed
from oracle import Oracle
from parity_util import assert_losses_within, loss_tolerance
from sr_amd import (Dataset, Options, ParametricExpression, SubDataset, TemplateExpression, TemplateExpressionSpec,
                    TemplateStructure, compose, eval_grad_batch, eval_grad_tree_array_batch, eval_loss, eval_loss_batch,
                    eval_tree_array_batch, flatten_trees, get_scalar_constants, optimize_constants_batch,
                    parse_expression, string_tree)
from template_util import SUB_OPS, build_case, load_cases, random_template, staged_eval

pytestmark = pytest.mark.gpu

OPTS = Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos"])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _tmpl(expressions, combine, trees, opts=OPTS, values=None, **kw):
    st = TemplateStructure(expressions, combine, **kw)
    return TemplateExpression({k: parse_expression(v, opts) for k, v in trees.items()}, structure=st, parameters=values)


def _union(opts, ex):
    """The options a hand-composed tree is scored with: the union operator set."""
    return Options(operators=ex.structure.union_operators(opts.operators))


def _isapprox(a, b, dtype):
    """Julia's isapprox with its default rtol = sqrt(eps(T)), atol = 0 (vectors: 2-norms)."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return np.linalg.norm(a - b) <= np.sqrt(np.finfo(dtype).eps) * max(np.linalg.norm(a), np.linalg.norm(b))


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("case", load_cases(), ids=lambda c: c["name"])
def test_reference_known_answers(case):
    opts, ex, X, y, rows = build_case(case)
    e = case["expect"]
    ds = Dataset(X, y)
    view = ds if rows is None else SubDataset(ds, rows)
    out, comp = eval_tree_array_batch([ex], view, opts)
    assert bool(comp[0]) == e["complete"]
    if e["complete"]:
        assert out.dtype == X.dtype and _isapprox(out[0], e["predictions"], X.dtype)
    if y is not None:
        loss, comp = eval_loss_batch([ex], view, opts)
        assert bool(comp[0]) == e["complete"] and loss.dtype == X.dtype
        assert _isapprox(loss[0], e["loss"], X.dtype)
        assert _isapprox(eval_loss(ex, ds, opts, idx=rows), e["loss"], X.dtype)


# ------------------------------------------------------------------ identity with the hand-composed tree
def _data(n, dtype, seed, weights=False):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((3, n)).astype(dtype)
    y = (np.sin(X[0] * X[1]) + X[2]).astype(dtype)
    w = rng.random(n).astype(dtype) + dtype(0.5) if weights else None
    return X, y, w


IDENTITY = [
    (("f", "g"), "sin(f(x1, x2)) + g(x3)^2", {"f": "x1 * x2 + 0.5", "g": "cos(x1) - 1.25"},
     "sin(((x1 * x2) + 0.5)) + ((cos(x3) - 1.25) * (cos(x3) - 1.25))"),
    (("f",), "f(f(x1)) - 0.5 * f(x2 / x3)", {"f": "1.5 * x1 + 0.25"},
     "((1.5 * ((1.5 * x1) + 0.25)) + 0.25) - (0.5 * ((1.5 * (x2 / x3)) + 0.25))"),
    (("f", "g"), "max(f(), g(x1, exp(x2)))", {"f": "0.75", "g": "x1 * x2"}, "max(0.75, x1 * exp(x2))"),
]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("view", ["full", "sub", "weighted"])
def test_template_equals_the_hand_composed_tree_bit_for_bit(dtype, view):
    X, y, w = _data(333, dtype, 7, weights=view == "weighted")
    ds = Dataset(X, y, weights=w)
    dv = SubDataset(ds, np.random.default_rng(3).integers(0, 333, 130)) if view == "sub" else ds
    for keys, combine, trees, by_hand in IDENTITY:
        ex = _tmpl(keys, combine, trees)
        uo = _union(OPTS, ex)
        hand = parse_expression(by_hand, uo)
        assert string_tree(compose(ex, OPTS).tree, uo) == string_tree(hand, uo)
        l0, c0 = eval_loss_batch([hand], dv, uo)
        l1, c1 = eval_loss_batch([ex], dv, OPTS)
        p0, pc0 = eval_tree_array_batch([hand], dv, uo)
        p1, pc1 = eval_tree_array_batch([ex], dv, OPTS)
        assert c0[0] and c1[0] and pc0[0] and pc1[0]
        assert np.array_equal(_bits(l0), _bits(l1)) and np.array_equal(_bits(p0), _bits(p1))
        # eval_cost(_batch): this loss, and the SUM of the sub-expressions' complexities (not the composed tree's)
        po = Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos"], parsimony=0.01)
        size = sum(t.count_nodes() for t in ex.trees.values())
        assert sr_amd.compute_complexity(ex, po) == size != compose(ex, OPTS).tree.count_nodes()
        cost, loss = sr_amd.eval_cost(dv, ex, po)
        costs, losses = sr_amd.eval_cost_batch([ex], dv, po)
        assert np.array_equal(_bits(np.asarray([loss])), _bits(l1)) and np.array_equal(_bits(losses), _bits(l1))
        want = sr_amd.loss_to_cost(loss, ds.use_baseline, ds.baseline_loss, None, po, complexity=size)
        assert cost == want and costs[0] == want


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_random_templates_against_the_oracle(dtype):
    """100 random templates, ten structures of ten candidates, one device call each: the flags are the restatement's (composition plus guards), the
    losses within parity_util's bars of the oracle's on the composed tree."""
    rng = np.random.default_rng(99)
    opts = Options(**SUB_OPS)
    X = rng.standard_normal((3, 333)).astype(dtype)
    y = rng.standard_normal(333).astype(dtype)
    # one structure per device call: 10 structures x 10 candidates
    n_bad = 0
    for s in range(10):
        first = random_template(rng, opts, dtype)
        batch = [first]
        for _ in range(9):
            trees = {k: sr_amd.gen_random_tree_fixed_size(int(rng.integers(1, 10)), opts,
                                                          max(1, first.structure.num_features[k]), dtype, rng)
                     for k in first.structure.expressions if first.structure.num_features[k] > 0}
            trees.update({k: first.trees[k].copy() for k in first.structure.expressions if k not in trees})
            batch.append(TemplateExpression(trees, structure=first.structure))
        loss, comp = eval_loss_batch(batch, Dataset(X, y), opts)
        cs = [compose(ex, opts) for ex in batch]
        orc = Oracle(cs[0].operators.unaops, cs[0].operators.binops)
        want = np.array([staged_eval(ex, X, opts)[1] for ex in batch])
        assert np.array_equal(comp, want), first.structure.combine
        n_bad += int((~want).sum())
        tb = flatten_trees([c.tree for c in cs], dtype)
        tol, ol, oc, _ = loss_tolerance(orc, tb, X, y)
        assert np.all(np.isinf(loss[~comp]))
        assert_losses_within(loss[comp], ol[comp], np.ones(int(comp.sum()), bool), tol[comp], first.structure.combine)
    assert 5 <= n_bad <= 95


# ------------------------------------------------------------------ guards
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_dropped_argument_still_decides_the_flag(dtype):
    """f(x1, x2 / x3), f = #1 composes to x1: the division by zero is seen only through the guard."""
    X, y, _ = _data(200, dtype, 5)
    X[2, 150] = 0
    ds = Dataset(X, y)
    ex = _tmpl(("f",), "f(x1, x2 / x3)", {"f": "x1"})
    assert string_tree(compose(ex, OPTS).tree, OPTS) == "x1"
    loss, comp = eval_loss_batch([ex], ds, OPTS)
    assert not comp[0] and np.isinf(loss[0])
    assert not eval_tree_array_batch([ex], ds, OPTS)[1][0]
    l, g, c = eval_grad_batch([ex], ds, OPTS)
    assert not c[0] and np.isinf(l[0])
    rows = np.r_[0:150, 151:200]
    loss, comp = eval_loss_batch([ex], SubDataset(ds, rows), OPTS)
    ref, rc = eval_loss_batch([parse_expression("x1", OPTS)], SubDataset(ds, rows), OPTS)
    assert comp[0] and rc[0] and np.array_equal(_bits(loss), _bits(ref))
    # has_invalid_variables: incomplete without evaluation, gradient zero
    bad = _tmpl(("f", "g"), "f(x1, x2) + g(x3)", {"f": "x1 + x3 * 2.0", "g": "x1"})
    good = _tmpl(("f", "g"), "f(x1, x2) + g(x3)", {"f": "x1 + x2 * 2.0", "g": "x1"})
    l, g, c = eval_grad_batch([bad, good], SubDataset(ds, rows), OPTS)
    assert not c[0] and np.isinf(l[0]) and c[1] and np.isfinite(l[1]) and g[0] == 0 and g[1] != 0 and g.shape == (2,)
    out, c = eval_tree_array_batch([bad, good], SubDataset(ds, rows), OPTS)
    assert not c[0] and c[1] and not out[0].any()  # (the invalid candidate's predictions are left untouched)


# ------------------------------------------------------------------ tied gradient against the untied sum
def _chain(n):
    """c_n * cos(c_(n-1) * cos(... cos(c_1 * #1))): n scalars around ONE occurrence of #1, so f(f(x1)) holds 2 n
    constants (the untied reference takes 128 at the most)."""
    s = "x1"
    for i in range(n):
        s = f"{0.9 + 0.05 * i:.2f} * {s}" if i == 0 else f"{0.9 + 0.05 * i:.2f} * cos({s})"
    return s


TIED_SUBS = {
    # every operand form a constant takes in a gradient program (csrc/sr_compile.cpp emit, with_const_index)
    "whole_tree": "0.75",                               # LOAD_CONST as the whole tree
    "load_const": "1.5 - x1",                           # LOAD_CONST, then the feature as the operand
    "add_cr": "cos(x1) + 0.5", "sub_cl": "0.5 - cos(x1)", "sub_cr": "cos(x1) - 0.5",
    "mul_c": "1.5 * cos(x1)", "div_cl": "1.5 / (cos(x1) + 2.0)", "div_cr": "cos(x1) / 1.5",
    "pow_general": "(cos(x1) + 2.0) ^ 1.5", "pow_left": "1.5 ^ cos(x1)",
    "max_general": "max(cos(x1), 0.25)",
    "under_unary": "cos(0.75) * x1",
    "three": "1.5 * cos(x1 * 0.75) + 0.25",
    "seventeen": _chain(17),
}
TIED_STRUCTS = ["f(x1) - f(x2)", "f(f(x1))", "f(x1) * f(x2) / f(x3)"]
TIED_OPTS = Options(binary_operators=["+", "-", "*", "/", "^", "max"], unary_operators=["cos"])
_RATIOS = {}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("combine", TIED_STRUCTS)
def test_tied_gradient_equals_the_sum_over_copies(dtype, combine):
    """Each tied scalar's derivative against the SUM of its copies' derivatives from the untied gradient call on
    the same composed tree, within m eps_T A + 64 eps_f64 A (m copies; A = sum over rows and copies of
    |d pred / d c_copy * d loss / d pred|, formed here in f64)."""
    rng = np.random.default_rng(11)
    n = 257
    X = rng.uniform(-0.8, 0.8, (3, n)).astype(dtype)
    y = rng.standard_normal(n).astype(dtype)
    ds = Dataset(X, y)
    batch = [_tmpl(("f",), combine, {"f": sub}, opts=TIED_OPTS) for sub in TIED_SUBS.values()]
    cs = [compose(ex, TIED_OPTS) for ex in batch]
    uo = Options(operators=cs[0].operators)
    plain = flatten_trees([c.tree for c in cs], dtype)
    lt, gt, ct = eval_grad_batch(batch, ds, TIED_OPTS)
    lu, gu, cu = eval_grad_batch(plain, ds, uo)
    pred, rowg, cr = eval_grad_tree_array_batch(plain, ds, uo, variable=False)
    assert ct.all() and cu.all() and cr.all() and np.array_equal(_bits(lt), _bits(lu))
    co = plain.constant_offsets()
    eps_t, eps64 = float(np.finfo(dtype).eps), float(np.finfo(np.float64).eps)
    at, worst = 0, 0.0
    for name, c, t in zip(TIED_SUBS, cs, range(len(cs))):
        slots = np.asarray(c.slots)
        assert c.n_scalars == {"three": 3, "seventeen": 17}.get(name, 2 if name in ("div_cl", "pow_general") else 1)
        untied = gu[co[t]:co[t + 1]].astype(np.float64)
        dldp = 2.0 * (pred[t].astype(np.float64) - y.astype(np.float64)) / n
        for s in range(c.n_scalars):
            copies = np.flatnonzero(slots == s)
            m = len(copies)
            # (f = a constant under f(f(x1)): the inner call is dropped, its copy lives in the guard tree)
            assert m == (1 if (name, combine) == ("whole_tree", "f(f(x1))") else 3 if "x3" in combine else 2)
            A = float(np.sum(np.abs(rowg[t][copies].astype(np.float64) * dldp)))
            bar = m * eps_t * A + 64 * eps64 * A
            err = abs(float(gt[at + s]) - float(np.sum(untied[copies])))
            assert err <= bar, (name, combine, s, err, bar)
            worst = max(worst, err / bar if bar > 0 else 0.0)
        at += c.n_scalars
    assert at == gt.size
    _RATIOS[(combine, np.dtype(dtype).name)] = worst
    print(f"template_grad_ties {combine!r} {np.dtype(dtype).name}: max |tied - sum untied| / bar = {worst:.3f}")


# ------------------------------------------------------------------ frozen literals
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_structure_literals_are_frozen(dtype):
    X, y, _ = _data(129, dtype, 2)
    y = (2.0 * 3.0 * X[0] + 1.5).astype(dtype)
    ds = Dataset(X, y)
    ex = _tmpl(("f",), "2.0 * f(x1) + 1.5", {"f": "1.0 * x1"})
    l, g, c = eval_grad_batch([ex], ds, OPTS)
    assert c[0] and g.shape == (1,)
    want = np.mean(2.0 * (2.0 * X[0].astype(np.float64) + 1.5 - y) * 2.0 * X[0])
    assert abs(g[0] - want) <= 1e-4 * abs(want)
    new, loss, imp, _ = optimize_constants_batch([ex], ds, OPTS, np.random.default_rng(0))
    # (the fit itself is not the subject: one Newton path on an exact quadratic, far inside these margins)
    assert imp[0] and loss[0] < 1e-4 and abs(get_scalar_constants(new[0])[0] - 3.0) < 1e-2
    tree = compose(new[0], OPTS).tree
    vals = [n.val for n in tree.preorder() if n.degree == 0 and n.constant]
    assert vals[0] == 2.0 and vals[-1] == 1.5 and len(vals) == 3
    assert new[0].structure is ex.structure and get_scalar_constants(ex).tolist() == [1.0]


# ------------------------------------------------------------------ scalars without a constant node
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_scalars_the_composed_tree_does_not_hold(dtype):
    """An unread entry of a parameter vector (f(x) + p[1] with two parameters) and a sub-expression called only
    inside a dropped argument (f(x1, g(x2)), f = c * #1): the derivative is exactly 0 and the optimiser leaves
    the value as it is, while the other scalars are fitted — alone and beside a candidate of the usual kind."""
    X, _, _ = _data(129, dtype, 9)
    ds = Dataset(X, (3.0 * X[0] + 0.5).astype(dtype))
    unread = _tmpl(("f",), "f(x) + p[1]", {"f": "1.5 * x1"}, values={"p": [1.0, 2.0]}, arguments=("x",),
                   parameters={"p": 2})
    l, g, c = eval_grad_batch([unread, unread.copy()], ds, OPTS)
    assert c.all() and g.shape == (6,) and g[0] != 0 and g[1] != 0 and g[2] == 0 and np.array_equal(g[:3], g[3:])
    new, loss, imp, _ = optimize_constants_batch([unread], ds, OPTS, np.random.default_rng(0))
    v = get_scalar_constants(new[0])
    assert imp[0] and loss[0] < 1e-4 and abs(v[0] - 3.0) < 1e-2 and abs(v[1] - 0.5) < 1e-2 and v[2] == 2.0
    dropped = _tmpl(("f", "g"), "f(x1, g(x2))", {"f": "1.5 * x1", "g": "0.75 * x1 + 0.25"})
    plain = _tmpl(("f", "g"), "f(x1, g(x2))", {"f": "1.5 * x1 + 0.125 * x2", "g": "0.75 * x1 + 0.25"})
    assert len(compose(dropped, OPTS).guards) == 1 and not compose(plain, OPTS).guards
    l, g, c = eval_grad_batch([dropped, plain], ds, OPTS)
    assert c.all() and g.shape == (7,) and g[0] != 0 and g[1] == 0 and g[2] == 0 and np.all(g[3:] != 0)
    new, loss, imp, _ = optimize_constants_batch([dropped, plain], ds, OPTS, np.random.default_rng(0))
    v = get_scalar_constants(new[0])
    x1, yy = X[0].astype(np.float64), 3.0 * X[0].astype(np.float64) + 0.5
    c_star = float(np.sum(yy * x1) / np.sum(x1 * x1))
    assert imp.all() and abs(v[0] - c_star) < 1e-2 and v[1] == 0.75 and v[2] == 0.25
    assert not np.array_equal(get_scalar_constants(new[1])[2:], [0.75, 0.25])


def test_optimised_scalars_that_break_a_guard_are_not_adopted():
    """f(x1, sqrt(f(x2, x3))), f = c * #1 on positive x2: the main tree c * x1 fits y = -2 x1 at c = -2, where the
    guard sqrt(c * x2) is NaN.  The candidate keeps its start and its starting loss."""
    rng = np.random.default_rng(3)
    X = rng.uniform(0.5, 2.0, (3, 129))
    ds = Dataset(X, -2.0 * X[0])
    ex = _tmpl(("f",), "f(x1, sqrt(f(x2, x3)))", {"f": "1.0 * x1"})
    l0, c0 = eval_loss_batch([ex], ds, OPTS)
    new, loss, imp, _ = optimize_constants_batch([ex], ds, OPTS, np.random.default_rng(0))
    assert c0[0] and not imp[0] and get_scalar_constants(new[0]).tolist() == [1.0] and loss[0] == l0[0]


# ------------------------------------------------------------------ tied optimisation: a closed form
def test_tied_optimisation_lands_on_the_constrained_minimum():
    """f(x1) + f(x2), f = c * #1, y = 2 x1 + 3 x2: the objective is exactly quadratic in the ONE scalar c, so the
    Newton path lands on c* = sum y (x1 + x2) / sum (x1 + x2)^2.  An optimiser that lets the copies drift apart
    reaches c = (2, 3) and loss 0."""
    rng = np.random.default_rng(17)
    X = rng.standard_normal((2, 129))
    y = 2.0 * X[0] + 3.0 * X[1]
    ds = Dataset(X, y)
    ex = _tmpl(("f",), "f(x1) + f(x2)", {"f": "1.0 * x1"})
    new, loss, imp, _ = optimize_constants_batch([ex], ds, OPTS, np.random.default_rng(0))
    s = X[0] + X[1]
    c_star = float(np.sum(y * s) / np.sum(s * s))
    l_star = float(np.mean((c_star * s - y) ** 2))
    c = float(get_scalar_constants(new[0])[0])
    assert imp[0] and abs(c - c_star) <= 1e-6 * abs(c_star), (c, c_star)
    assert loss[0] >= l_star * (1 - 1e-12), (loss[0], l_star)
    vals = [n.val for n in compose(new[0], OPTS).tree.preorder() if n.degree == 0 and n.constant]
    assert vals == [c, c]


# ------------------------------------------------------------------ category-indexed parameters
def _category_case(dtype, n_literals=0):
    """n_literals: that many literals of the structure in front (2.0 * p1[category] ..., then + 0.01 * x1 terms):
    frozen constants beside the scalars and the parameter tangents (33: a window of frozen entries only)."""
    rng = np.random.default_rng(23)
    n = 300
    cls = rng.integers(1, 4, n)
    X = np.stack([rng.standard_normal(n), rng.standard_normal(n), cls.astype(np.float64)]).astype(dtype)
    y = (cls * np.cos(X[0]) + X[0] * cls - 0.5).astype(dtype)
    ds = Dataset(X, y, extra={"class": cls}, n_classes=3)
    rows = np.flatnonzero(cls != 2)[:200]  # class 2 has no row in the view
    values = {"p1": [1.0, 2.0, 3.0], "p2": [0.5, -0.25, 0.75], "p3": [7.0]}
    lead = "2.0 * " if n_literals else ""
    tail = "".join(f" + {0.01 * (i + 1):.2f} * x1" for i in range(max(0, n_literals - 1)))
    ex = _tmpl(("f", "g"), f"{lead}p1[category] * g(x1) + f(x1, p2[category]) - p3[1]{tail}",
               {"f": "x1 * x2 + 0.5", "g": "cos(x1)"},
               values=values, arguments=("x1", "x2", "category"), parameters={"p1": 3, "p2": 3, "p3": 1})
    popts = Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos"],
                    expression_spec=sr_amd.ParametricExpressionSpec(max_parameters=2))
    by_hand = f"(({lead}p1 * cos(x1)) + ((x1 * p2) + 0.5)) - 7.0{tail}"
    hand = ParametricExpression(parse_expression(by_hand, popts), np.array([values["p1"], values["p2"]], dtype=dtype))
    return ds, SubDataset(ds, rows), ex, hand, popts


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_category_parameters_equal_the_hand_built_parametric_expression(dtype):
    ds, sub, ex, hand, popts = _category_case(dtype)
    assert get_scalar_constants(ex).tolist() == [0.5, 1.0, 2.0, 3.0, 0.5, -0.25, 0.75, 7.0]
    for view in (ds, sub):
        l0, c0 = eval_loss_batch([hand], view, popts)
        l1, c1 = eval_loss_batch([ex], view, OPTS)
        assert c0[0] and c1[0] and np.array_equal(_bits(l0), _bits(l1))
        p0, _ = eval_tree_array_batch([hand], view, popts)
        p1, _ = eval_tree_array_batch([ex], view, OPTS)
        assert np.array_equal(_bits(p0), _bits(p1))
        # gradient: the hand-built call gives [0.5, 7.0 | K x C column-major]
        _, g0, _ = eval_grad_batch([hand], view, popts)
        _, g1, gc = eval_grad_batch([ex], view, OPTS)
        mapped = np.concatenate([g0[:1], g0[2::2], g0[3::2], g0[1:2]])  # f's constant, p1, p2, p3[1]
        assert gc[0] and np.array_equal(_bits(mapped), _bits(g1))
        assert np.all(g1[[1, 3, 4, 6, 0, 7]] != 0)
        if view is sub:
            assert g1[2] == 0 and g1[5] == 0  # the absent class
    # the optimised result
    tb0, lo0, i0, _ = optimize_constants_batch([hand], sub, popts, np.random.default_rng(5))
    new, lo1, i1, _ = optimize_constants_batch([ex], sub, OPTS, np.random.default_rng(5))
    assert i0[0] and i1[0] and np.array_equal(_bits(lo0), _bits(lo1))
    v = get_scalar_constants(new[0]).astype(dtype)
    c0 = tb0.get_constants()
    assert np.array_equal(_bits(np.array([v[0], v[7]])), _bits(c0))
    assert np.array_equal(_bits(v[1:4]), _bits(tb0.parameters[0, 0])) and np.array_equal(_bits(v[4:7]), _bits(tb0.parameters[0, 1]))
    assert new[0].structure is ex.structure


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_literals", [1, 33])
def test_category_parameters_beside_frozen_literals(dtype, n_literals):
    """The constant table [scalars | frozen | used parameters]: loss and gradient equal the hand-built
    ParametricExpression's (whose literals are constants of their own), entry for entry and bit for bit; with 33
    literals the tangent window [16, 32) holds frozen entries only and is left out."""
    ds, sub, ex, hand, popts = _category_case(dtype, n_literals)
    c = compose(ex, OPTS)
    assert string_tree(c.tree, OPTS) == string_tree(hand.tree, OPTS) and c.slots.count(-1) == n_literals
    assert get_scalar_constants(ex).tolist() == [0.5, 1.0, 2.0, 3.0, 0.5, -0.25, 0.75, 7.0]
    where = [j for j, s in enumerate(c.slots) if s >= 0]  # the hand-built tree's constants that are scalars
    nc = len(c.slots)
    for view in (ds, sub):
        l0, c0 = eval_loss_batch([hand], view, popts)
        l1, c1 = eval_loss_batch([ex], view, OPTS)
        assert c0[0] and c1[0] and np.array_equal(_bits(l0), _bits(l1))
        _, g0, _ = eval_grad_batch([hand], view, popts)
        _, g1, gc = eval_grad_batch([ex], view, OPTS)
        mapped = np.concatenate([g0[where[:1]], g0[nc::2], g0[nc + 1::2], g0[where[1:]]])
        assert gc[0] and g1.shape == (8,) and np.array_equal(_bits(mapped), _bits(g1))
    new, loss, imp, _ = optimize_constants_batch([ex], sub, OPTS, np.random.default_rng(5))
    assert imp[0] and loss[0] < eval_loss_batch([ex], sub, OPTS)[0][0]
    lits = lambda e: [n.val for n, s in zip([n for n in compose(e, OPTS).tree.preorder() if n.degree == 0 and n.constant],  # noqa: E731
                                            c.slots) if s < 0]
    assert lits(new[0]) == lits(ex) and len(lits(ex)) == n_literals


def test_category_parameters_refuse_mismatched_data():
    ds, sub, ex, hand, popts = _category_case(np.float32)
    X = ds.X.copy()
    X[2, 5] = 1 + X[2, 5] % 3
    with pytest.raises(ValueError, match="category"):
        eval_loss_batch([ex], Dataset(X, ds.y, extra={"class": ds.classes}, n_classes=3), OPTS)
    with pytest.raises(ValueError, match="classes"):
        eval_loss_batch([ex], Dataset(ds.X, ds.y), OPTS)
    short = ex.copy()
    short.parameters["p2"] = np.array([1.0, 2.0])
    with pytest.raises(ValueError, match="entries"):
        eval_loss_batch([short], ds, OPTS)
    with pytest.raises(NotImplementedError, match="§16"):
        eval_loss_batch([ex], ds, Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos"],
                                          elementwise_loss="loss(p, t) = abs(p - t)"))


def test_expression_loss_on_a_parameter_free_template():
    X, y, _ = _data(130, np.float32, 4)
    ds = Dataset(X, y)
    lopts = Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos"], elementwise_loss="loss(p, t) = abs(p - t)")
    ex = _tmpl(("f",), "f(x1) - f(x2)", {"f": "1.5 * x1 + 0.25"})
    l1, c1 = eval_loss_batch([ex], ds, lopts)
    l0, c0 = eval_loss_batch([parse_expression("((1.5 * x1) + 0.25) - ((1.5 * x2) + 0.25)", lopts)], ds, lopts)
    assert c0[0] and c1[0] and np.array_equal(_bits(l0), _bits(l1))


# ------------------------------------------------------------------ refusals
def test_calls_that_do_not_take_templates_say_so():
    X, y, _ = _data(64, np.float32, 1)
    ds = Dataset(X, y)
    ex = _tmpl(("f",), "f(x1) - f(x2)", {"f": "1.5 * x1 + 0.25"})
    views = np.arange(64, dtype=np.int64).reshape(2, 32)
    for call in (lambda: sr_amd.eval_loss_batch_views([ex], ds, OPTS, [0], views),
                 lambda: sr_amd.eval_grad_batch_views([ex], ds, OPTS, [0], views),
                 lambda: sr_amd.distributed.eval_loss_sharded([ex], ds, OPTS),
                 lambda: sr_amd.distributed.eval_loss_tree_sharded([ex], ds, OPTS),
                 lambda: sr_amd.distributed.gpu_partials_packed([ex], ds, OPTS, 64),
                 lambda: sr_amd.eval_grad_tree_array_batch([ex], ds, OPTS),
                 lambda: sr_amd.eval_diff_tree_array_batch([ex], ds, OPTS, 1),
                 lambda: sr_amd.equation_search(X, y, niterations=1, options=Options(
                     binary_operators=["+", "*"], expression_spec=TemplateExpressionSpec(structure=ex.structure)))):
        with pytest.raises(NotImplementedError, match="DESIGN.md §16"):
            call()
    with pytest.raises(ValueError, match="one structure"):
        eval_loss_batch([ex, _tmpl(("f",), "f(x1)", {"f": "x1"})], ds, OPTS)
    with pytest.raises(ValueError, match="all templates"):
        eval_loss_batch([ex, parse_expression("x1", OPTS)], ds, OPTS)
