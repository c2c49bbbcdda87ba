"""TEST HELPER: the loss-value fixture (tests/golden/loss_values.json, make_loss_value_fixtures.py), the catalog
table, the bars and the device harness of test_loss_values_host.py, test_gpu_loss_values.py and
tools/loss_values_ulp.py.

The harness is loss_expr_points.device_elements' (its one-row-view helpers are shared, not copied): row k of one
dataset is point k (X[0] = pred, y = target), tree k runs on the one-row view [k]; the tree x1 gives the loss value,
x1 + 0.0 the derivative d loss / d pred as its single gradient entry.  A one-row view's loss is L_k w_k / w_k: with
a power-of-two weight the value's own bits, but for the sign of a zero (the tile's padding rows add +0.0), which no
test here compares.
"""
import functools
import importlib.util
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = {"float32": np.float32, "float64": np.float64}
EXACT, INEXACT, OVERFLOW = 0, 1, 2

# spec string -> (SrLossKind, class, parameter): include/sr_amd.h's SR_LOSS_* codes
CATALOG = {
    "L2DistLoss()": (0, "exact", 0.0), "L1DistLoss()": (1, "exact", 0.0),
    "LPDistLoss{3}()": (2, "inexact", 3.0), "LPDistLoss(1.5)": (2, "inexact", 1.5), "LPDistLoss{2}()": (2, "inexact", 2.0),
    "LPDistLoss{1}()": (2, "inexact", 1.0), "LogitDistLoss()": (3, "inexact", 0.0),
    "HuberLoss()": (4, "exact", 1.0), "HuberLoss(0.5)": (4, "exact", 0.5),
    "L1EpsilonInsLoss(0.25)": (5, "exact", 0.25), "L1EpsilonInsLoss(2.0)": (5, "exact", 2.0),
    "L2EpsilonInsLoss(0.25)": (6, "exact", 0.25), "L2EpsilonInsLoss(2.0)": (6, "exact", 2.0),
    "PeriodicLoss(4.0)": (7, "inexact", 4.0), "PeriodicLoss(0.5)": (7, "inexact", 0.5),
    "QuantileLoss(0.25)": (8, "exact", 0.25), "QuantileLoss(0.75)": (8, "exact", 0.75),
    "ZeroOneLoss()": (9, "exact", 0.0), "PerceptronLoss()": (10, "exact", 0.0), "L1HingeLoss()": (11, "exact", 0.0),
    "L2HingeLoss()": (12, "exact", 0.0), "SmoothedL1HingeLoss(0.5)": (13, "exact", 0.5),
    "SmoothedL1HingeLoss(2.0)": (13, "exact", 2.0), "ModifiedHuberLoss()": (14, "exact", 0.0),
    "L2MarginLoss()": (15, "exact", 0.0), "ExpLoss()": (16, "inexact", 0.0), "SigmoidLoss()": (17, "inexact", 0.0),
    "DWDMarginLoss(1)": (18, "inexact", 1.0), "DWDMarginLoss(2)": (18, "inexact", 2.0), "DWDMarginLoss(0.5)": (18, "inexact", 0.5),
}
# Float32 only: a parameter that T rounds (LossFunctions keeps it in Float64), held to the inexact bar
F32_ONLY = {"HuberLoss(0.3)": (4, "inexact", 0.3)}
NAMES = {0: "L2", 1: "L1", 2: "LP", 3: "Logit", 4: "Huber", 5: "L1EpsIns", 6: "L2EpsIns", 7: "Periodic", 8: "Quantile",
         9: "ZeroOne", 10: "Perceptron", 11: "L1Hinge", 12: "L2Hinge", 13: "SmoothedL1Hinge", 14: "ModifiedHuber",
         15: "L2Margin", 16: "Exp", 17: "Sigmoid", 18: "DWD"}
WEIGHTS = (0.5, 2.0, 4.0)

# The bars, in ulp_T(scale), per inexact loss: (value, derivative) per dtype, "host" (sr_host_elem_loss and the
# oracle: the CPU's libm) and "device" (MI355X).  They quote profiles/loss_values_ulp.txt (tools/loss_values_ulp.py),
# which holds the measured maxima: each bar is twice the maximum rounded up to a whole unit (the rule of
# profiles/op_values_ulp.txt; the factor covers a libm release changing a last bit).  No device maximum exceeds 2.
BARS = {
    "host": {
        "float32": {"DWD": (2, 2), "Exp": (0, 2), "Huber": (2, 0), "LP": (0, 2), "Logit": (2, 2), "Periodic": (2, 2), "Sigmoid": (1, 1)},
        "float64": {"DWD": (2, 2), "Exp": (0, 0), "LP": (0, 2), "Logit": (2, 2), "Periodic": (1, 2), "Sigmoid": (2, 2)},
    },
    "device": {
        "float32": {"DWD": (2, 2), "Exp": (2, 2), "Huber": (2, 0), "LP": (2, 2), "Logit": (2, 0), "Periodic": (2, 2), "Sigmoid": (1, 1)},
        "float64": {"DWD": (2, 4), "Exp": (0, 0), "LP": (2, 4), "Logit": (2, 2), "Periodic": (1, 2), "Sigmoid": (1, 1)},
    },
}


def bar_of(maximum):
    """Twice the measured maximum, rounded up to a whole unit."""
    return int(np.ceil(2.0 * maximum - 1e-12))


def specs(dtype_name):
    out = dict(CATALOG)
    if dtype_name == "float32":
        out.update(F32_ONLY)
    return out


@functools.lru_cache(maxsize=None)
def maker():
    """tests/golden/make_loss_value_fixtures.py as a module."""
    spec = importlib.util.spec_from_file_location("make_loss_value_fixtures", os.path.join(HERE, "golden", "make_loss_value_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture_text():
    with open(os.path.join(HERE, "golden", "loss_values.json")) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def fixture():
    return json.loads(fixture_text())


def from_bits(b, T):
    return np.array(b, dtype=np.uint32 if T == np.float32 else np.uint64).view(T)


def bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


class Points:
    """One (loss, dtype) entry of the fixture as arrays."""

    def __init__(self, dtype_name, spec):
        T = DTYPES[dtype_name]
        e = fixture()[dtype_name][spec]
        rows = e["points"]
        self.spec, self.dtype_name, self.T = spec, dtype_name, T
        self.kind, self.cls_name, self.param = specs(dtype_name)[spec]
        self.kinks = e["kinks"]
        self.pred, self.target, self.value, self.deriv = (from_bits([r[i] for r in rows], T) for i in range(4))
        self.scale_v = np.array([r[4] for r in rows], dtype=np.float64)
        self.scale_d = np.array([r[5] for r in rows], dtype=np.float64)
        self.cls = np.array([r[6] for r in rows], dtype=np.int64)
        self.dyadic = np.array([r[7] for r in rows], dtype=bool)
        self.n = len(rows)
        self.margin = self.kind >= 9
        self.bar_name = NAMES[self.kind]


def ulp_of(scale, T):
    """ulp_T(scale): T's spacing at the magnitude `scale` (the subnormal spacing at least)."""
    with np.errstate(all="ignore"):
        s = np.minimum(np.abs(np.asarray(scale, dtype=np.float64)), float(np.finfo(T).max)).astype(T)
    return np.maximum(np.spacing(s).astype(np.float64), float(np.finfo(T).smallest_subnormal))


def errors(pts, got_v, got_d):
    """(value error, derivative error) in ulp_T(scale) at every point; an exact-class or overflow point has the
    scale of its own expected value (only its zero / nonzero matters to the callers: they compare bits there)."""
    out = []
    for got, want, scale in ((got_v, pts.value, pts.scale_v), (got_d, pts.deriv, pts.scale_d)):
        with np.errstate(all="ignore"):
            sc = np.where(scale > 0, scale, np.abs(want.astype(np.float64)))
            sc = np.where(np.isfinite(sc), sc, 1.0)
            g, w = np.asarray(got, dtype=np.float64), want.astype(np.float64)
            err = np.where(g == w, 0.0, np.abs(g - w) / ulp_of(sc, pts.T))
        out.append(np.where(np.isnan(err), np.inf, err))
    return out


def same_but_zero_sign(got, want):
    """Bit-equal, a zero's sign apart."""
    got, want = np.asarray(got), np.asarray(want)
    return (bits(got) == bits(want)) | ((got == 0) & (want == 0))


def assert_meets(pts, got_v, got_d, where, what, counts=None):
    """Exact points bit-equal (a zero's sign apart), inexact points within BARS[where], overflow points by isinf (and
    the sign) where the fixture's value is infinite, else as their loss's class.  `counts`: incremented per point."""
    got_v, got_d = np.asarray(got_v, dtype=pts.T), np.asarray(got_d, dtype=pts.T)
    bar_v, bar_d = BARS[where][pts.dtype_name].get(pts.bar_name, (0, 0))
    err_v, err_d = errors(pts, got_v, got_d)
    for got, want, err, bar, which in ((got_v, pts.value, err_v, bar_v, "value"), (got_d, pts.deriv, err_d, bar_d, "derivative")):
        inf = np.isinf(want)
        exact = ~inf & ((pts.cls == EXACT) | ((pts.cls == OVERFLOW) & (pts.cls_name == "exact")))
        inexact = ~inf & ~exact
        bad = np.nonzero(inf & ~(np.isinf(got) & (np.signbit(got) == np.signbit(want))))[0]
        assert bad.size == 0, (what, which, "overflow", pts.pred[bad[:4]], pts.target[bad[:4]], got[bad[:4]])
        bad = np.nonzero(exact & ~same_but_zero_sign(got, want))[0]
        assert bad.size == 0, (what, which, "exact", pts.pred[bad[:4]], pts.target[bad[:4]], got[bad[:4]], want[bad[:4]])
        bad = np.nonzero(inexact & ~(err <= bar))[0]
        assert bad.size == 0, (what, which, f"bar {bar}", pts.pred[bad[:4]], pts.target[bad[:4]], got[bad[:4]], want[bad[:4]], err[bad[:4]])
    if counts is not None:
        counts[(pts.dtype_name, pts.spec)] = counts.get((pts.dtype_name, pts.spec), 0) + pts.n


def host_elements(pts):
    """(value, derivative) of sr_host_elem_loss at the points."""
    import ctypes

    from sr_amd import _lib

    v, d = np.empty(pts.n, dtype=pts.T), np.empty(pts.n, dtype=pts.T)
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    pred, target = np.ascontiguousarray(pts.pred), np.ascontiguousarray(pts.target)
    _lib.check(_lib.lib.sr_host_elem_loss(_lib.SR_DTYPE_F32 if pts.T == np.float32 else _lib.SR_DTYPE_F64, pts.kind, float(pts.param),
                                          pts.n, p(pred), p(target), p(v), p(d)))
    return v, d


def oracle_values(pts, accum):
    """The oracle's loss per point: one-row datasets (one per target), constant trees (one per prediction)."""
    from oracle import Oracle
    from sr_amd import Node, Options, flatten_trees

    orc = Oracle.from_options(Options(elementwise_loss=pts.spec, binary_operators=["+"], unary_operators=[]))
    got = np.full(pts.n, np.nan, dtype=pts.T)
    for t in np.unique(pts.target):
        idx = np.nonzero(pts.target == t)[0]
        tb = flatten_trees([Node(val=float(pts.pred[k])) for k in idx], pts.T)
        with np.errstate(all="ignore"):
            loss, comp = orc.eval_loss_batch(tb, np.zeros((1, 1), dtype=pts.T), np.array([t], dtype=pts.T), loss_kind=pts.kind,
                                             loss_param=pts.param, accum=accum)
        assert comp.all(), (pts.spec, t)
        got[idx] = loss
    return got


# ------------------------------------------------------------------------------------------------- the device harness
def options(spec, tier, gradient=False):
    from loss_expr_points import tier_operators
    from sr_amd import Options

    return Options(elementwise_loss=spec, **tier_operators(tier, gradient))


def dataset(pts, weights=None, rows=None):
    from sr_amd import Dataset

    idx = np.arange(pts.n) if rows is None else rows
    X = np.ascontiguousarray(pts.pred[idx][None, :])
    with np.errstate(over="ignore"):  # (1e20: the dataset's own statistics may overflow)
        return Dataset(X, np.ascontiguousarray(pts.target[idx]), **({} if weights is None else dict(weights=np.ascontiguousarray(weights))))


def point_weights(pts):
    """Power-of-two weights 0.5, 2, 4 dealt over the points."""
    return np.array([WEIGHTS[k % 3] for k in range(pts.n)], dtype=pts.T)


def device_elements(pts, tier, weighted=False, deriv=True):
    """(value [n], derivative [n] or None, complete [n]) of the device per point, each call made twice and
    required to repeat bit for bit."""
    from loss_expr_points import one_row_gradients, one_row_losses

    ds = dataset(pts, point_weights(pts) if weighted else None)
    try:
        val, comp = one_row_losses(options(pts.spec, tier), ds, pts.n, pts.T)
        val2, comp2 = one_row_losses(options(pts.spec, tier), ds, pts.n, pts.T)
        assert np.array_equal(bits(val), bits(val2)) and np.array_equal(comp, comp2), (pts.spec, tier, "the loss call does not repeat")
        der = None
        if deriv:
            der, gc = one_row_gradients(options(pts.spec, tier, gradient=True), ds, pts.n, pts.T)
            der2, gc2 = one_row_gradients(options(pts.spec, tier, gradient=True), ds, pts.n, pts.T)
            assert np.array_equal(bits(der), bits(der2)) and np.array_equal(gc, gc2), (pts.spec, tier, "the gradient call does not repeat")
            assert np.array_equal(gc, comp), (pts.spec, tier, gc, comp)
    finally:
        ds.free_device()
    return val, der, comp.astype(bool)
