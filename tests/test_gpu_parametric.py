"""GPU: ParametricExpression trees scored on the device (LOAD_PARAM / P operands, the SR_TIER_PARAM builds of csrc/sr_builds.h).

A parameter leaf p_k reads parameters[k, class[row]] of its own tree's matrix; DynamicExpressions evaluates
it as feature leaf nfeatures + k of vstack(X, parameters[:, class]).  So every parametric result has a
twin: the plain tree (parametric_util: the same population before its leaves were converted) on the
materialised columns X_ext — scored by the plain device path (bit for bit) and by the CPU oracle.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import sr_amd
from oracle import Oracle
from sr_amd import (Dataset, Options, ParametricExpression, ParametricExpressionSpec, _lib, batch, eval_loss,
                    eval_loss_batch, eval_loss_batch_views, eval_tree_array, eval_tree_array_batch, flatten_trees,
                    parse_expression)
from parity_util import assert_losses_within, loss_tolerance
from parametric_util import data, population, to_parametric, x_ext

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2_OPTS = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "log"])
NF, K, NC = 3, 2, 5


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _pds(X, y, cls, n_classes=NC, **kw):
    return Dataset(X, y, extra={"class": cls}, n_classes=n_classes, **kw)


# ------------------------------------------------------------------ 1. the reference's known answers
def test_golden_batched_parametric_mse():
    with open(os.path.join(ROOT, "tests", "golden", "parametric_known_answers.json")) as f:
        g = json.load(f)["batched_parametric_mse"]
    opts = Options(binary_operators=g["binary_operators"], unary_operators=g["unary_operators"],
                   expression_spec=ParametricExpressionSpec(max_parameters=g["max_parameters"]))
    d = Dataset(np.array(g["X"]), np.array(g["y"]), extra={"class": g["class"]})
    ex = ParametricExpression(parse_expression(g["expr"], opts), np.array(g["parameters"]))
    assert len(g["cases"]) == 5
    for case in g["cases"]:
        view = d if case["indices"] is None else batch(d, np.array(case["indices"]) - g["index_base"])
        assert float(eval_loss(ex, view, opts)) == pytest.approx(case["loss"], rel=1e-12), case
    out, comp = eval_tree_array(ex, np.array(g["X"]), g["class"], opts)
    assert comp and out.tolist() == [1.0, 2.0, 3.0]


# ------------------------------------------------------------------ 2. device vs device, bit for bit
@pytest.mark.parametrize("dtype,builds", [(np.float32, (0, 16, 8)), (np.float64, (0, 8, 4))])
def test_parametric_equals_plain_tree_on_materialised_columns(dtype, builds):
    """48 trees with distinct (2, 5) matrices over 2,500 rows (ragged across three 1,024-row tiles of the
    16-rows-per-lane kernel): loss bits, complete and predictions equal the plain tree's on
    Dataset(vstack(X, P_t[:, class - 1]), y), under every rows_per_lane setting."""
    opts = Options(**C2_OPTS)
    n, nt = 2500, 48
    X, y, cls = data(n, NF, NC, dtype=dtype, seed=3)
    ext = population(nt, opts, NF, K, dtype=dtype, seed=12)
    P = np.random.default_rng(5).standard_normal((nt, K, NC)).astype(dtype)
    par = to_parametric(ext, NF, P)
    assert par.is_parameter.sum() >= 20
    pds = _pds(X, y, cls)
    plain = [Dataset(x_ext(X, P[t], cls), y) for t in range(nt)]
    ctx = sr_amd.get_context()
    try:
        for rpl in builds:
            ctx.set_tuning("rows_per_lane", rpl)
            loss, comp = eval_loss_batch(par, pds, opts)
            pred, pcomp = eval_tree_array_batch(par, pds, opts)
            assert comp.any()
            for t in range(nt):
                one = ext.take([t])
                l1, c1 = eval_loss_batch(one, plain[t], opts)
                p1, pc1 = eval_tree_array_batch(one, plain[t], opts)
                assert (bool(comp[t]), bool(pcomp[t])) == (bool(c1[0]), bool(pc1[0])), (rpl, t)
                assert _bits(loss[t:t + 1])[0] == _bits(l1)[0], (rpl, t, loss[t], l1[0])
                assert np.array_equal(_bits(pred[t]), _bits(p1[0])), (rpl, t)
    finally:
        ctx.set_tuning("rows_per_lane", 0)
        for d in plain:
            d.free_device()


# ------------------------------------------------------------------ 3. / 4. populations vs the oracle
def _assert_population(loss, comp, o_loss, o_comp, tol, ref_loss, tb, what):
    mism = np.nonzero(comp != o_comp)[0]
    assert len(mism) == 0, (what, mism[:5])
    assert np.all(np.isinf(loss[~comp]))
    assert_losses_within(loss, o_loss, comp, tol, what)
    # trees without a transcendental: the reference's in-order fold, bit for bit
    n_unary = np.add.reduceat((tb.degree == 1).astype(np.int64), tb.offsets[:-1])
    arith = comp & (n_unary == 0)
    assert arith.sum() >= 5, what
    assert np.array_equal(_bits(loss[arith]), _bits(ref_loss[arith])), what


@pytest.mark.parametrize("n", [5000, 97])
def test_population_shared_parameters_vs_oracle(n):
    opts = Options(**C2_OPTS)
    X, y, cls = data(n, NF, NC, seed=n)
    ext = population(1500, opts, NF, K, seed=7)
    P = np.random.default_rng(8).standard_normal((K, NC)).astype(np.float32)
    par = to_parametric(ext, NF, P)
    loss, comp = eval_loss_batch(par, _pds(X, y, cls), opts)
    Xe = x_ext(X, P, cls)
    orc = Oracle.from_options(opts)
    tol, o_loss, o_comp, _ = loss_tolerance(orc, ext, Xe, y)
    ref_loss, _ = orc.eval_loss_batch(ext, Xe, y, accum="ref", n_threads=8)
    _assert_population(loss, comp, o_loss, o_comp, tol, ref_loss, ext, f"shared n={n}")


def test_population_distinct_parameters_vs_oracle():
    """300 trees (several tree groups, launched in cost order dealt over the groups), each with its own
    matrix: the table is read at the caller's tree index."""
    opts = Options(**C2_OPTS)
    n, nt = 3000, 300
    X, y, cls = data(n, NF, NC, seed=21)
    ext = population(nt, opts, NF, K, seed=22)
    P = (1.5 * np.random.default_rng(23).standard_normal((nt, K, NC))).astype(np.float32)
    par = to_parametric(ext, NF, P)
    loss, comp = eval_loss_batch(par, _pds(X, y, cls), opts)
    orc = Oracle.from_options(opts)
    tol = np.zeros(nt)
    o_loss = np.zeros(nt, dtype=np.float32)
    ref_loss = np.zeros(nt, dtype=np.float32)
    o_comp = np.zeros(nt, dtype=bool)
    for t in range(nt):
        one, Xe = ext.take([t]), x_ext(X, P[t], cls)
        tl, ol, oc, _ = loss_tolerance(orc, one, Xe, y)
        tol[t], o_loss[t], o_comp[t] = tl[0], ol[0], oc[0]
        ref_loss[t] = orc.eval_loss_batch(one, Xe, y, accum="ref")[0][0]
    _assert_population(loss, comp, o_loss, o_comp, tol, ref_loss, ext, "distinct")
    # two trees' matrices swapped: their results change (and only theirs)
    # (a pair whose losses the oracle says depend on the matrix: p1 - p1 would not)
    uses = np.add.reduceat(par.is_parameter.astype(np.int64), par.offsets[:-1])
    cand = np.nonzero(comp & (uses > 0) & np.isfinite(loss))[0]

    def swapped(t, u):
        return orc.eval_loss_batch(ext.take([t]), x_ext(X, P[u], cls), y, accum="ref")

    a = b = -1
    for i in range(min(20, cand.size // 2)):
        t, u = int(cand[i]), int(cand[-1 - i])
        (lt, ct), (lu, cu) = swapped(t, u), swapped(u, t)
        if ct[0] and cu[0] and lt[0] != o_loss[t] and lu[0] != o_loss[u]:
            a, b = t, u
            break
    assert a >= 0
    P2 = P.copy()
    P2[[a, b]] = P[[b, a]]
    loss2, comp2 = eval_loss_batch(to_parametric(ext, NF, P2), _pds(X, y, cls), opts)
    assert loss2[a] != loss[a] and loss2[b] != loss[b]
    assert loss2[a] == pytest.approx(float(swapped(a, b)[0][0]), rel=1e-4)
    assert loss2[b] == pytest.approx(float(swapped(b, a)[0][0]), rel=1e-4)
    keep = np.ones(nt, dtype=bool)
    keep[[a, b]] = False
    assert np.array_equal(_bits(loss2[keep]), _bits(loss[keep])) and np.array_equal(comp2[keep], comp[keep])


# ------------------------------------------------------------------ 5. views and gather
def test_views_equal_single_view_calls():
    opts = Options(**C2_OPTS)
    n, nt = 600, 64
    X, y, cls = data(n, NF, NC, seed=31)
    ext = population(nt, opts, NF, K, seed=32)
    P = np.random.default_rng(33).standard_normal((nt, K, NC)).astype(np.float32)
    par = to_parametric(ext, NF, P)
    d = _pds(X, y, cls)
    rng = np.random.default_rng(34)
    rows = rng.integers(0, n, size=(4, 50))  # drawn with replacement
    tree_view = rng.integers(0, 4, size=nt)
    loss, comp = eval_loss_batch_views(par, d, opts, tree_view, rows)
    assert comp.any()
    for v in range(4):
        sel = np.nonzero(tree_view == v)[0]
        l1, c1 = eval_loss_batch(par.take(sel), batch(d, rows[v]), opts)
        assert np.array_equal(c1, comp[sel]), v
        assert np.array_equal(_bits(l1), _bits(loss[sel])), v


# ------------------------------------------------------------------ 6. finiteness edges
def _edge(expr, X, cls, P, n_classes):
    """(device complete, oracle complete, device loss, oracle loss) of one Float32 parametric tree."""
    opts = Options(**C2_OPTS)
    y = np.zeros(X.shape[1], dtype=np.float32)
    t = parse_expression(expr, opts)
    ex = ParametricExpression(t, P)
    loss, comp = eval_loss_batch([ex], _pds(X, y, cls, n_classes), opts)
    pred, pcomp = eval_tree_array_batch([ex], _pds(X, y, cls, n_classes), opts)
    assert bool(pcomp[0]) == bool(comp[0])
    sub = parse_expression(expr.replace("p1", f"x{X.shape[0] + 1}"), opts)
    orc = Oracle.from_options(opts)
    ol, oc = orc.eval_loss_batch(flatten_trees([sub], np.float32), x_ext(X, P, cls), y, accum="ref")
    return bool(comp[0]), bool(oc[0]), loss[0], ol[0]


def test_edge_array_sum_overflows():
    """x1 * p1 over 4,096 rows, one class at 3e38 / 100: every value is finite, DynamicExpressions' sum of
    the output array is not."""
    n = 4096
    rng = np.random.default_rng(41)
    X = (0.5 + rng.random((1, n))).astype(np.float32)
    cls = rng.integers(1, 4, size=n).astype(np.int32)
    P = np.array([[1.0, np.float32(3e38) / 100, -2.0]], dtype=np.float32)
    comp, o_comp, loss, _ = _edge("x1 * p1", X, cls, P, 3)
    assert np.all(np.isfinite(X[0] * P[0, cls - 1]))
    assert comp is False and o_comp is False and np.isinf(loss)


def test_edge_inf_parameter_in_last_tile():
    """cos(p1): Inf in a class whose only row sits in the last row tile."""
    n = 2500
    X = np.random.default_rng(42).standard_normal((1, n)).astype(np.float32)
    cls = np.ones(n, dtype=np.int32)
    cls[:1000] = 2
    cls[n - 3] = 3
    P = np.array([[0.5, 1.5, np.inf]], dtype=np.float32)
    comp, o_comp, loss, _ = _edge("cos(p1)", X, cls, P, 3)
    assert comp is False and o_comp is False and np.isinf(loss)
    cls[n - 3] = 1  # the same matrix, the Inf class now unused: complete
    comp, o_comp, loss, o_loss = _edge("cos(p1)", X, cls, P, 3)
    assert comp is True and o_comp is True and _bits(np.float32([loss]))[0] == _bits(np.float32([o_loss]))[0]


def test_edge_nan_in_unused_class():
    """p1 + x1 with NaN in a class no row uses: no row reads it, the tree is complete."""
    n = 1500
    X = np.random.default_rng(43).standard_normal((1, n)).astype(np.float32)
    cls = np.where(np.arange(n) % 2 == 0, 1, 3).astype(np.int32)
    P = np.array([[0.25, np.nan, -1.0]], dtype=np.float32)
    comp, o_comp, loss, o_loss = _edge("p1 + x1", X, cls, P, 3)
    assert comp is True and o_comp is True
    assert _bits(np.float32([loss]))[0] == _bits(np.float32([o_loss]))[0]


# ------------------------------------------------------------------ 7. both paths of the in-order fold
def test_both_fold_paths_give_the_sequential_fold():
    opts = Options(**C2_OPTS)
    n, nt = 40_000, 400
    X, y, cls = data(n, NF, NC, seed=51)
    ext = population(nt, opts, NF, K, seed=52)
    P = np.random.default_rng(53).standard_normal((nt, K, NC)).astype(np.float32)
    par = to_parametric(ext, NF, P)
    d = _pds(X, y, cls)
    ctx = sr_amd.get_context()
    try:
        l1, c1 = eval_loss_batch(par, d, opts)
        i1 = ctx.last_ref_fold()
        ctx.set_tuning("fold_store_mb", 0)
        l2, c2 = eval_loss_batch(par, d, opts)
        i2 = ctx.last_ref_fold()
    finally:
        ctx.set_tuning("fold_store_mb", 512)
    assert i1["path"] == 1 and i2["path"] == 2, (i1, i2)
    assert i1["folded"] > 100 and i2["folded"] > 100, (i1, i2)
    assert np.array_equal(c1, c2)
    fin = c1 & np.isfinite(l1)
    assert np.array_equal(_bits(l1[fin]), _bits(l2[fin]))
    pred, pcomp = eval_tree_array_batch(par, d, opts)
    assert np.array_equal(pcomp, c1)
    idx = np.nonzero(fin)[0]
    want = np.empty(idx.size, dtype=np.float32)
    for q, t in enumerate(idx):  # LossFunctions' L2 mean of the device's own predictions: a left fold in Float32
        e = (pred[t] - y).astype(np.float32)
        want[q] = np.float32(np.add.accumulate(e * e, dtype=np.float32)[-1] / np.float32(n))
    bad = idx[_bits(l1[idx]) != _bits(want)]
    assert bad.size == 0, (bad[:5], l1[bad[:5]])


# ------------------------------------------------------------------ 8. invariance and errors
def test_plain_calls_ignore_the_class_row_and_errors():
    opts = Options(**C2_OPTS)
    n = 3000
    X, y, cls = data(n, NF, NC, seed=61)
    plain = flatten_trees(sr_amd.gen_random_population(400, opts, NF, max_size=30, seed=62), np.float32)
    with_cls, without = _pds(X, y, cls), Dataset(X, y)
    la, ca = eval_loss_batch(plain, with_cls, opts)
    lb, cb = eval_loss_batch(plain, without, opts)
    assert np.array_equal(ca, cb) and np.array_equal(_bits(la), _bits(lb))
    pa, _ = eval_tree_array_batch(plain.take(np.arange(40)), with_cls, opts)
    pb, _ = eval_tree_array_batch(plain.take(np.arange(40)), without, opts)
    assert np.array_equal(_bits(pa), _bits(pb))
    idx = np.random.default_rng(63).integers(0, n, size=200)
    assert np.array_equal(_bits(eval_loss_batch(plain, batch(with_cls, idx), opts)[0]),
                          _bits(eval_loss_batch(plain, batch(without, idx), opts)[0]))
    ctx = sr_amd.get_context()
    nf_out, n_out = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.lib.sr_dataset_info(with_cls.device_handle(ctx), None, ctypes.byref(nf_out), ctypes.byref(n_out)))
    assert (nf_out.value, n_out.value) == (NF, n)

    # a parametric call needs classes, and as many as the parameters have columns
    ext = population(8, opts, NF, K, seed=64)
    par = to_parametric(ext, NF, np.ones((K, NC), dtype=np.float32))
    with pytest.raises(ValueError):
        eval_loss_batch(par, without, opts)  # the Python mirror refuses first
    s, ps = par.to_struct(), par.to_param_struct()
    out_l, out_c = np.empty(8, dtype=np.float32), np.empty(8, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def call(ds, ps_):
        return _lib.lib.sr_eval_loss_batch_parametric(ctx.handle, ds.device_handle(ctx), ctx.opset_id(opts.operators),
                                                      ctypes.byref(s), ctypes.byref(ps_), None, 0, 0, p(out_l), p(out_c))

    assert call(without, ps) == _lib.SR_ERR_INVALID_ARG and "classes" in _lib.last_error()
    assert call(with_cls, ps) == 0
    ps6 = to_parametric(ext, NF, np.ones((K, NC + 1), dtype=np.float32))
    assert call(with_cls, ps6.to_param_struct()) == _lib.SR_ERR_INVALID_ARG and "n_classes" in _lib.last_error()
    bad_par = par.parameter.copy()
    bad_par[par.is_parameter != 0] = K + 1
    bad = sr_amd.node.TreeBatch(par.offsets, par.degree, par.op, par.feature, par.constant, par.val, par.is_parameter,
                                bad_par, par.parameters)
    s = bad.to_struct()
    assert call(with_cls, bad.to_param_struct()) == _lib.SR_ERR_BAD_TREE
    # the upload refuses a class outside 1..n_classes
    Xj = np.ascontiguousarray(X.T)
    out = ctypes.c_void_p()
    for wrong in (0, NC + 1):
        c2 = cls.copy()
        c2[17] = wrong
        rc = _lib.lib.sr_dataset_upload_classes(ctx.handle, _lib.SR_DTYPE_F32, p(Xj), NF, n, p(y), None, p(c2), NC,
                                                ctypes.byref(out))
        assert rc == _lib.SR_ERR_INVALID_ARG and "row 17" in _lib.last_error()
