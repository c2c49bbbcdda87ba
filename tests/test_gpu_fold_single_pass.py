"""GPU: the in-order fold's steps composed in the loss launch under candidate binades ("fold_single_pass").

A large call (path 2 of the in-order loss fold, csrc/sr_fold_dev.h) used to run every complete tree twice:
the loss launch, then the FOLD-mode pass, because the binade of the running sum at each row block is only
known from the f64 prefix.  The loss launch now guesses that binade per (tree, row block) from the
block's first tile and composes the block's steps under the binades nearest the guess; the plan takes
a block's pair from there when its binade is among them and no tile has an exact half-ulp tie, and
the FOLD pass runs only what is left.  Every composition is exact, so nothing may change in any bit:

* knob 1 = knob 0 = numpy's sequential Float32 fold of the device's own predictions;
* exact half-ulp ties, heavy-tailed trees (the guess misses), a shortage of slow-segment slots, views that
  are no multiple of the tile and one-row-block calls all give the same bits.

Shapes: 40,000 rows with "fold_store_mb" 0 (path 2), "fold_seg_max" 2048, "max_row_blocks" 20 and
"vstk_rows" 16: 20 row blocks of two 1,024-row tiles on the register-stack launch (the build that composes
candidates; below 2^17 rows a call takes the 512-row-tile LDS-stack build unless told otherwise, and a
small batch more, shorter row blocks), so a block's steps accumulate over more than one tile.
"""
import numpy as np
import pytest

import sr_amd
from sr_amd import (Dataset, Options, eval_loss_batch, eval_tree_array_batch, flatten_trees, gen_random_population,
                    parse_expression)

pytestmark = pytest.mark.gpu

OPTS = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "log"])
N = 40_000
DEFAULTS = dict(fold_single_pass=1, fold_store_mb=512, fold_seg_max=16384, vstk_rows=0, fold_slot_mb=24576,
                max_row_blocks=512)


def _data(n, seed=2, weighted=False):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((5, n)).astype(np.float32)
    y = (2 * np.cos(X[3]) + X[0] ** 2 - 2 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    w = (0.25 + rng.random(n)).astype(np.float32) if weighted else None
    return X, y, w


def _jl_sum32(v):
    """Base.sum of a Float32 vector: mapreduce_impl's pairwise recursion, leaves of < 1024 folded in order."""
    def rec(lo, hi):
        if hi - lo < 1024:
            return np.add.accumulate(v[lo:hi + 1], dtype=np.float32)[-1]
        mid = lo + ((hi - lo) >> 1)
        return np.float32(rec(lo, mid) + rec(mid + 1, hi))
    return np.float32(rec(0, len(v) - 1))


def _np_fold_losses(pred, y, w=None):
    """LossFunctions' L2 mean (or weighted sum / sum(w)) of the given predictions, in Float32 and in row
    order: numpy's add.accumulate is a sequential left fold."""
    d = (pred - y).astype(np.float32)
    lo = d * d
    if w is not None:
        lo = (lo * w).astype(np.float32)
    total = np.add.accumulate(lo, dtype=np.float32)[-1]
    den = _jl_sum32(w) if w is not None else np.float32(len(y))
    return np.float32(total / den)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _run(tb, ds, opts, single_pass, **knobs):
    """One path-2 call at the module's shapes; every knob back to its default afterwards."""
    ctx = sr_amd.get_context()
    setup = dict(fold_store_mb=0, fold_seg_max=2048, vstk_rows=16, max_row_blocks=20, fold_single_pass=single_pass)
    setup.update(knobs)
    try:
        for k, v in setup.items():
            ctx.set_tuning(k, v)
        loss, comp = eval_loss_batch(tb, ds, opts)
        info = ctx.last_ref_fold()
        info.update(ctx.last_fold_cand())
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_tuning(k, v)
    return loss, comp, info


@pytest.fixture(scope="module")
def population():
    opts = Options(**OPTS)
    return opts, flatten_trees(gen_random_population(1200, opts, 5, max_size=30, seed=7), np.float32)


@pytest.mark.parametrize("weighted", [False, True])
def test_on_equals_off_equals_sequential_fold(population, weighted):
    opts, tb = population
    X, y, w = _data(N, weighted=weighted)
    ds = Dataset(X, y, weights=w)
    l1, c1, i1 = _run(tb, ds, opts, 1)
    l0, c0, i0 = _run(tb, ds, opts, 0)
    print("single pass on:", i1, "off:", i0)
    assert i1["path"] == 2 and i0["path"] == 2, (i1, i0)
    assert np.array_equal(c1, c0)
    fin = c1 & np.isfinite(l1)
    assert fin.sum() > 300
    assert np.array_equal(np.isfinite(l1), np.isfinite(l0))
    assert np.array_equal(_bits(l1[fin]), _bits(l0[fin]))
    pred, _ = eval_tree_array_batch(tb, ds, opts)
    idx = np.nonzero(fin)[0]
    want = np.array([_np_fold_losses(pred[t], y, w) for t in idx], dtype=np.float32)
    bad = idx[_bits(l1[idx]) != _bits(want)]
    assert bad.size == 0, (bad[:5], l1[bad[:5]], want[:5])
    assert i0["taken"] == 0 and i0["rerun"] > 0, i0
    assert i1["taken"] > 0 and i1["rerun"] < i0["rerun"], (i1, i0)
    assert i1["taken"] + i1["rerun"] == i0["rerun"], (i1, i0)  # (the same blocks, split between the passes)


@pytest.mark.parametrize("single_pass", [1, 0])
def test_exact_half_ulp_ties(single_pass):
    """Losses that are exact multiples of 2^-12 under running sums near 2^17 (ulp 2^-6... 2^-7): about one
    row in 64 is an exact half-ulp tie, which poisons a candidate (the FOLD pass's ordered composition
    takes the block).  The reference needs no device."""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((5, N)).astype(np.float32)
    X[0] = (rng.integers(0, 256, N) / 64.0).astype(np.float32)
    y = np.zeros(N, dtype=np.float32)
    opts = Options(**OPTS)
    tb = flatten_trees([parse_expression(e, opts) for e in ("x1", "x1 * 1.0", "x1 + 0.0")], np.float32)
    loss, comp, info = _run(tb, Dataset(X, y), opts, single_pass)
    print("ties, single pass", single_pass, info)
    assert info["path"] == 2 and comp.all(), info
    want = np.float32(np.add.accumulate((X[0] * X[0]).astype(np.float32), dtype=np.float32)[-1] / np.float32(N))
    assert np.array_equal(_bits(loss), _bits(np.full(3, want, dtype=np.float32))), (loss, want, info)


def test_heavy_tail_takes_the_rerun():
    """A tree whose loss sits in a few rows: the first tile's sum says little about the running sum, the
    guess misses by many binades and the blocks take the FOLD pass.  (exp(1.5 x^2) over these 40,000
    N(0,1) rows, max |x| = 4.75, stays below 5e14: the CPU oracle scores the tree complete with a finite
    Float32 loss, 5.56e24, of which five rows hold all but 1e-11.)"""
    X, y, _ = _data(N, seed=6)
    opts = Options(**OPTS)
    tb = flatten_trees([parse_expression("exp(x1 * x1 * 1.5)", opts)], np.float32)
    ds = Dataset(X, y)
    l1, c1, i1 = _run(tb, ds, opts, 1)
    l0, c0, i0 = _run(tb, ds, opts, 0)
    print("heavy tail, on:", i1, "off:", i0)
    assert c1.all() and c0.all() and np.isfinite(l1).all()
    assert np.array_equal(_bits(l1), _bits(l0))
    assert i1["path"] == 2 and i1["rerun"] > 0, i1
    pred, _ = eval_tree_array_batch(tb, ds, opts)
    assert _bits(l1[0]) == _bits(_np_fold_losses(pred[0], y))


def test_slot_shortage_is_counted(population):
    """128 slow-segment slots for 1,200 trees: a tree that finds no slot — for its first block too — takes
    the fallback and is counted; no tree silently keeps the f64 sum."""
    opts, tb = population
    X, y, _ = _data(N)
    ds = Dataset(X, y)
    l_d, c_d, i_d = _run(tb, ds, opts, 1)
    l_s, c_s, i_s = _run(tb, ds, opts, 1, fold_slot_mb=1)
    print("slots default:", i_d, "1 MB:", i_s)
    assert np.array_equal(c_d, c_s)
    fin = c_d & np.isfinite(l_d)
    assert i_s["folded"] + i_s["fallback"] == int(fin.sum()), (i_s, int(fin.sum()))
    assert i_s["fallback"] > 0, i_s
    assert np.array_equal(_bits(l_d[fin]), _bits(l_s[fin]))


@pytest.mark.parametrize("n", [40_001, 1_000])
def test_odd_edges(n):
    """A view that is no multiple of the tile, and a call of one row block (nothing to take there)."""
    X, y, _ = _data(n, seed=8)
    opts = Options(**OPTS)
    tb = flatten_trees(gen_random_population(300, opts, 5, max_size=30, seed=13), np.float32)
    ds = Dataset(X, y)
    l1, c1, i1 = _run(tb, ds, opts, 1)
    l0, c0, i0 = _run(tb, ds, opts, 0)
    print("n", n, "on:", i1, "off:", i0)
    assert i1["path"] == 2 and i0["path"] == 2
    assert np.array_equal(c1, c0)
    fin = c1 & np.isfinite(l1)
    assert np.array_equal(_bits(l1[fin]), _bits(l0[fin]))
    if n <= 1024:  # (one tile, one row block: no candidates, the first block is always the plan's)
        assert i1["taken"] == 0 and i1["rerun"] == i0["rerun"], (i1, i0)
    idx = np.nonzero(fin)[0][:60]
    pred, _ = eval_tree_array_batch(tb.take(idx), ds, opts)
    want = np.array([_np_fold_losses(pred[k], y) for k in range(len(idx))], dtype=np.float32)
    assert np.array_equal(_bits(l1[idx]), _bits(want))
