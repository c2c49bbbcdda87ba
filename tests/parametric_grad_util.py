"""TEST HELPER: reference gradients of parametric trees with respect to their parameter matrix.

A parametric population's CPU twin is the plain population on ``x_ext(X, P, cls)`` (parametric_util), so
d loss / d P[k, c] is a central difference of the oracle's Float64 loss on ``x_ext(X, P +- h e_kc, cls)``,
Richardson-extrapolated over h and h / 2 with |D(h) - D(h/2)| as the error estimate — the scheme of
``Oracle.loss_grad_fd`` for constants.  One matrix is shared by every tree, so each (entry, sign, step)
is one oracle call over the whole batch.
"""
import numpy as np

from parametric_util import x_ext


def _central(orc, ext, X, y, cls, P, rel, w, loss_kind):
    K, C = P.shape
    g = np.zeros((ext.n_trees, K, C))
    for k in range(K):
        for c in range(C):
            h = rel * max(1.0, abs(P[k, c]))
            lp = []
            for sgn in (1.0, -1.0):
                Q = P.copy()
                Q[k, c] += sgn * h
                lp.append(orc.eval_loss_batch(ext, x_ext(X, Q, cls), y, w, loss_kind, accum="f64", n_threads=8)[0])
            with np.errstate(invalid="ignore"):
                g[:, k, c] = (lp[0] - lp[1]) / (2 * h)
    return g


def param_grad_fd(orc, ext, X, y, cls, P, w=None, loss_kind=0):
    """(g[n_trees, K, C], err[n_trees, K, C]) for the plain twins `ext` (Float64 data)."""
    X, y, P = np.asarray(X, np.float64), np.asarray(y, np.float64), np.asarray(P, np.float64)
    g1 = _central(orc, ext, X, y, cls, P, 1e-5, w, loss_kind)
    g2 = _central(orc, ext, X, y, cls, P, 5e-6, w, loss_kind)
    return (4 * g2 - g1) / 3, np.abs(g2 - g1)


def uses_parameter(par):
    """[n_trees] bool: the tree has a parameter leaf."""
    return np.add.reduceat(par.is_parameter.astype(np.int64), par.offsets[:-1]) > 0
