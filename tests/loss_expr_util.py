"""TEST HELPER: the per-tree loss tolerance for calls that accumulate in f64 (expression losses).

``parity_util.loss_tolerance``'s recipe — the oracle's loss as is and under four one-ulp libm
perturbations; every tree held to max(rel_bar |loss|, spread_factor x its measured spread) — with the
oracle's ``accum="f64"``: an expression-loss call returns the f64 sum of the element losses divided once
(DESIGN.md §14), not the reference's in-order fold in T.
"""
import numpy as np

from parity_util import PERTURB_SEEDS, REL_BAR

# the issue's restated catalog losses: body over (p, t) -> the catalog spec it restates
RESTATED = {
    "square(p - t)": "L2DistLoss()",
    "abs(p - t)": "L1DistLoss()",
    "abs(p - t)^3": "LPDistLoss{3}()",
    "-log(4.0) - (p - t) + 2.0*log(1.0 + exp(p - t))": "LogitDistLoss()",
    "(p - t) * (((p - t) > 0.0) - 0.3)": "QuantileLoss(0.3)",
    "square(max(0.0, 1.0 - t*p))": "L2HingeLoss()",
    "square(1.0 - t*p)": "L2MarginLoss()",
    "exp(-(t*p))": "ExpLoss()",
    "1.0 - tanh(t*p)": "SigmoidLoss()",
}
OPS = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "log"])


def data(n, seed, dtype, margin=False):
    """tests/test_gpu_losses.py's inputs."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((4, n)).astype(dtype)
    y = 2 * np.cos(X[3]) + X[0] ** 2 - 2 + 0.1 * rng.standard_normal(n)
    if margin:  # classification targets for the margin-based losses
        y = np.sign(y) + (y == 0)
    return X, y.astype(dtype)


def loss_tolerance_f64(orc, tb, X, y, w=None, loss_kind=0, loss_param=0.0, rel_bar=REL_BAR, spread_factor=4.0):
    """(tol, loss, complete, n_widened) of the unperturbed oracle under f64 accumulation."""
    kw = dict(w=w, loss_kind=loss_kind, accum="f64", n_threads=8, loss_param=loss_param)
    l0, c0 = orc.eval_loss_batch(tb, X, y, **kw)
    spread = np.zeros(len(l0))
    for seed in PERTURB_SEEDS:
        lp, cp = orc.eval_loss_batch(tb, X, y, perturb=seed, **kw)
        with np.errstate(invalid="ignore"):
            d = np.abs(lp.astype(np.float64) - l0.astype(np.float64))
        spread = np.maximum(spread, np.where(cp & c0 & np.isfinite(d), d, 0.0))
    base = rel_bar * np.abs(l0.astype(np.float64))
    tol = np.maximum(base, spread_factor * spread)
    return tol, l0, c0, int(np.sum(c0 & (tol > base)))
