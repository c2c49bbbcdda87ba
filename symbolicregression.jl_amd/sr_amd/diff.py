"""Per-row derivatives mirrored from reference src/InterfaceDynamicExpressions.jl:118-165
(``eval_diff_tree_array``, ``eval_grad_tree_array``), computed on the device by the per-row build of the
forward-mode gradient kernel.

The single-tree functions keep the reference's names and argument meanings; the batched ones
(``eval_grad_tree_array_batch`` / ``eval_diff_tree_array_batch``) differentiate a whole batch in one call.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .dataset import Dataset, SubDataset
from .device import get_context
from .loss import _as_batch
from .node import ParametricExpression

_PARAMETRIC = ("per-row derivatives of ParametricExpression trees are not on the device: DESIGN.md §15 "
               "(plain trees only)")


def grad_layout(n_grad, n_rows: int) -> np.ndarray:
    """[n_trees + 1] element offsets of the trees' ``[n_grad_t, n_rows]`` blocks in the flat derivative array
    of ``sr_eval_grad_tree_array`` (rows fastest; tree t starts at the running sum of ``n_grad_u * n_rows``)."""
    n_grad = np.asarray(n_grad, dtype=np.int64)
    if n_grad.ndim != 1 or (n_grad < 0).any() or n_rows < 0:
        raise ValueError("n_grad must be a vector of non-negative counts and n_rows non-negative")
    return np.concatenate([[0], np.cumsum(n_grad * np.int64(n_rows))]).astype(np.int64)


def n_grad_of(tb, nfeatures: int, variable: bool) -> np.ndarray:
    """Derivative arrays per tree: its constants (``variable=False``) or ``nfeatures`` (``variable=True``)."""
    if variable:
        return np.full(tb.n_trees, int(nfeatures), dtype=np.int64)
    return np.diff(tb.constant_offsets()).astype(np.int64)


def _refuse_parametric(trees):
    if isinstance(trees, ParametricExpression) or getattr(trees, "parametric", False):
        raise NotImplementedError(_PARAMETRIC)
    if isinstance(trees, (list, tuple)) and any(isinstance(t, ParametricExpression) for t in trees):
        raise NotImplementedError(_PARAMETRIC)


def _prepare(trees, dataset):
    from .template import refuse

    refuse(trees, "the per-row derivative calls (eval_grad_tree_array / eval_diff_tree_array)")
    _refuse_parametric(trees)
    if not isinstance(dataset, (Dataset, SubDataset)):
        raise TypeError("dataset must be a Dataset or a SubDataset")
    full = dataset.full
    tb = _as_batch(trees, full.dtype)
    if tb.parametric:
        raise NotImplementedError(_PARAMETRIC)
    idx = dataset.indices
    n_rows = full.n if idx is None else int(idx.size)
    return full, tb, idx, n_rows


def check_directions(directions, n_trees: int, nfeatures: int) -> np.ndarray:
    """``directions`` (one 1-based feature per tree, or one for all) as int32 [n_trees]; ``ValueError`` outside
    1..nfeatures."""
    d = np.asarray(directions)
    if d.ndim == 0:
        d = np.full(n_trees, d)
    if d.shape != (n_trees,):
        raise ValueError(f"directions must be one feature index per tree ({n_trees}), got shape {d.shape}")
    if d.size and not np.issubdtype(d.dtype, np.integer):
        if not np.all(d == np.floor(d)):
            raise ValueError("directions must be integers")
    d = d.astype(np.int64)
    if d.size and (d.min() < 1 or d.max() > nfeatures):
        raise ValueError(f"direction outside 1..{nfeatures}")
    return np.ascontiguousarray(d, dtype=np.int32)


def eval_grad_tree_array_batch(trees, dataset, options, *, variable: bool = False, ctx=None):
    """``(evaluation[n_trees, n_rows], gradients, complete[n_trees])``: ``gradients[t]`` is tree t's
    ``[n_grad_t, n_rows]`` array — one row per constant in pre-order (``variable=False``) or per feature
    (``variable=True``; exactly 0 for a feature the tree does not use).  ``evaluation`` is
    ``eval_tree_array_batch``'s; ``complete`` is its flag and no returned derivative being NaN or ±Inf; an
    incomplete tree's derivatives are all 0."""
    full, tb, idx, n_rows = _prepare(trees, dataset)
    ctx = ctx or get_context()
    ng = n_grad_of(tb, full.nfeatures, bool(variable))
    off = grad_layout(ng, n_rows)
    out = np.empty((tb.n_trees, n_rows), dtype=full.dtype)
    grads = np.zeros(int(off[-1]) + 1, dtype=full.dtype)
    complete = np.empty(tb.n_trees, dtype=np.uint8)
    s = tb.to_struct()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    _lib.check(_lib.lib.sr_eval_grad_tree_array(
        ctx.handle, full.device_handle(ctx), ctx.opset_id(options.operators), ctypes.byref(s),
        None if idx is None else p(idx), 0 if idx is None else int(idx.size), 1 if variable else 0,
        p(out), p(grads), p(complete)))
    per_tree = [grads[off[t]:off[t + 1]].reshape(int(ng[t]), n_rows) for t in range(tb.n_trees)]
    return out, per_tree, complete.astype(bool)


def eval_diff_tree_array_batch(trees, dataset, options, directions, *, ctx=None):
    """``(evaluation[n_trees, n_rows], derivative[n_trees, n_rows], complete[n_trees])``: tree t's derivative
    with respect to feature ``directions[t]`` (1-based) — that row of the ``variable=True`` gradient, bit for
    bit, computed with one tangent."""
    full, tb, idx, n_rows = _prepare(trees, dataset)
    d = check_directions(directions, tb.n_trees, full.nfeatures)
    ctx = ctx or get_context()
    out = np.empty((tb.n_trees, n_rows), dtype=full.dtype)
    diff = np.zeros((tb.n_trees, n_rows), dtype=full.dtype)
    complete = np.empty(tb.n_trees, dtype=np.uint8)
    s = tb.to_struct()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    _lib.check(_lib.lib.sr_eval_diff_tree_array(
        ctx.handle, full.device_handle(ctx), ctx.opset_id(options.operators), ctypes.byref(s),
        None if idx is None else p(idx), 0 if idx is None else int(idx.size), p(d), p(out), p(diff), p(complete)))
    return out, diff, complete.astype(bool)


def _with_dataset(X, fn):
    if isinstance(X, (Dataset, SubDataset)):
        return fn(X)
    ds = Dataset(np.asarray(X))
    try:
        return fn(ds)
    finally:
        ds.free_device()


def eval_diff_tree_array(tree, X, options, direction):
    """``eval_diff_tree_array(tree, X, options, direction) -> (evaluation, derivative, complete)``
    (src/InterfaceDynamicExpressions.jl:118-130): the derivative with respect to feature ``direction``
    (1-based) at every row.  ``X`` is ``[nfeatures, n]`` or a Dataset / SubDataset."""
    _refuse_parametric(tree)
    if int(direction) != direction:
        raise ValueError("direction must be an integer")
    nf = X.full.nfeatures if isinstance(X, (Dataset, SubDataset)) else np.asarray(X).shape[0]
    check_directions([int(direction)], 1, nf)  # (before any upload)
    out, diff, comp = _with_dataset(X, lambda ds: eval_diff_tree_array_batch([tree], ds, options, [int(direction)]))
    return out[0], diff[0], bool(comp[0])


def eval_grad_tree_array(tree, X, options, *, variable: bool = False):
    """``eval_grad_tree_array(tree, X, options; variable) -> (evaluation, gradient[n_grad, n], complete)``
    (src/InterfaceDynamicExpressions.jl:153-165): with ``variable=True`` the derivative with respect to every
    feature, else with respect to every constant (pre-order)."""
    _refuse_parametric(tree)
    out, grads, comp = _with_dataset(X, lambda ds: eval_grad_tree_array_batch([tree], ds, options, variable=variable))
    return out[0], grads[0], bool(comp[0])
