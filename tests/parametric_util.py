"""TEST HELPER: parametric populations from the plain generator, and their materialised-column twins.

DynamicExpressions evaluates a ParametricExpression as the plain tree in which parameter leaf p_k is
feature leaf nfeatures + k, on ``vstack(X, parameters[:, class - 1])``.  So a plain population generated
over nf + K features IS the oracle's (and the plain device path's) input for the parametric population
obtained by turning every feature leaf above nf into parameter leaf ``feature - nf``.
"""
import ctypes

import numpy as np

from sr_amd import _lib, flatten_trees, gen_random_population
from sr_amd.node import TreeBatch


def to_parametric(tb_ext: TreeBatch, nf: int, parameters) -> TreeBatch:
    """tb_ext: a plain batch over nf + K features; parameters: [K, n_classes] (shared by every tree) or
    [n_trees, K, n_classes].  The parametric batch: the same trees with leaves x_(nf + k) -> p_k (their
    `feature` field zeroed: a parameter leaf's feature is not read)."""
    P = np.asarray(parameters, dtype=tb_ext.val.dtype)
    if P.ndim == 2:
        P = np.broadcast_to(P, (tb_ext.n_trees,) + P.shape)
    isp = (tb_ext.degree == 0) & (tb_ext.constant == 0) & (tb_ext.feature > nf)
    par = np.where(isp, tb_ext.feature.astype(np.int64) - nf, 0)
    assert par.max(initial=0) <= P.shape[1]
    feat = np.where(isp, 0, tb_ext.feature)
    return TreeBatch(tb_ext.offsets, tb_ext.degree, tb_ext.op, feat, tb_ext.constant, tb_ext.val, isp, par, P)


def x_ext(X, P, cls):
    """vstack(X, P[:, class - 1]) for one [K, n_classes] matrix and 1-based classes."""
    P = np.asarray(P, dtype=X.dtype)
    return np.ascontiguousarray(np.vstack([X, P[:, np.asarray(cls) - 1]]))


def population(n_trees, opts, nf, K, dtype=np.float32, seed=0, max_size=30):
    """A plain random population over nf + K features (the oracle's input), as a TreeBatch."""
    return flatten_trees(gen_random_population(n_trees, opts, nf + K, max_size=max_size, dtype=dtype, seed=seed), dtype)


def data(n, nf=3, n_classes=5, dtype=np.float32, seed=2):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((nf, n)).astype(dtype)
    cls = rng.integers(1, n_classes + 1, size=n).astype(np.int32)
    cls[:n_classes] = np.arange(1, n_classes + 1)[: min(n, n_classes)]  # every class present (n >= n_classes)
    y = (2 * np.cos(X[nf - 1].astype(np.float64)) + X[0].astype(np.float64) ** 2 * (1 + 0.1 * cls) - 2).astype(dtype)
    return X, y, cls


def compile_info(tb: TreeBatch, opts, n_rows, nfeatures):
    """(rc, out_len, out_static_bad, max_depth) of sr_compile_info / sr_compile_info_parametric."""
    una = [s.encode() for s in opts.operators.unaops]
    bina = [s.encode() for s in opts.operators.binops]
    ua = (ctypes.c_char_p * max(len(una), 1))(*una)
    ba = (ctypes.c_char_p * max(len(bina), 1))(*bina)
    s = tb.to_struct()
    out_len = np.zeros(tb.n_trees, dtype=np.int32)
    bad = np.zeros(tb.n_trees, dtype=np.uint8)
    depth = ctypes.c_int(0)
    dt = _lib.SR_DTYPE_F32 if tb.val.dtype == np.float32 else _lib.SR_DTYPE_F64
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    if tb.parametric:
        ps = tb.to_param_struct()
        rc = _lib.lib.sr_compile_info_parametric(dt, len(una), ua, len(bina), ba, ctypes.byref(s), ctypes.byref(ps),
                                                 n_rows, nfeatures, p(out_len), p(bad), ctypes.byref(depth), None, 0)
    else:
        rc = _lib.lib.sr_compile_info(dt, len(una), ua, len(bina), ba, ctypes.byref(s), n_rows, nfeatures, p(out_len),
                                      p(bad), ctypes.byref(depth), None, 0)
    return rc, out_len, bad.astype(bool), int(depth.value)
