"""GPU: the schedule of a large call's fold chains and exact-sum pass (csrc/sr_capi.cpp):
"tail_chunk" (a plain path-2 call with the candidate launch runs three chunks, so that the last two chunks'
chains — plan, compact, scan, FOLD re-run, walk — run side by side) and "exact_early" (the BIG trees'
exact-sum pass enqueued as soon as the flags are final, beside the last chains).

The two only move launches between streams and chunks: no kernel's arithmetic changes, so no bit of any
result may change, whatever runs beside what.  With the two at 0 the launch sequence is the two-chunk one.

Shapes: tests/test_gpu_fold_compact.py's (1,200 trees of seed 7 x 40,000 rows, "fold_store_mb" 0,
"fold_seg_max" 2048, "vstk_rows" 16, "max_row_blocks" 20: path 2 over 20 row blocks), "chunk_min" 64 so that
the call runs several chunks, and planted trees whose values pass the deferred checks' bound at this row
count (FLT_MAX / (2 x 40,000 x nodes) ~ 1e32), which the exact-sum pass decides.
"""
import numpy as np
import pytest

import sr_amd
from bytecode_vm import compile_info
from sr_amd import (Dataset, Options, eval_loss_batch, eval_tree_array_batch, flatten_trees, gen_random_population,
                    parse_expression)
from sr_amd.dataset import SubDataset

pytestmark = pytest.mark.gpu

OPTS = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "log"])
N = 40_000
ON = dict(tail_chunk=4, exact_early=1)  # the library's defaults
OFF = dict(tail_chunk=0, exact_early=0)
DEFAULTS = dict(fold_store_mb=512, fold_seg_max=16384, vstk_rows=0, max_row_blocks=512, chunk_min=1024, **ON)
BIG = ("x1 * 5.0e34", "(x2 * 4.0e34) + x3", "cos(x1) * 2.0e33", "x4 * 1.0e33", "(x1 * 3.0e34) - (x5 * 2.0e34)",
       "x2 * 6.0e33")


def _data(n, seed=2):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((5, n)).astype(np.float32)
    y = (2 * np.cos(X[3]) + X[0] ** 2 - 2 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    w = (0.25 + rng.random(n)).astype(np.float32)
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


def _run(tb, ds, opts, **knobs):
    """One call at the module's shapes; every knob back to its default afterwards."""
    ctx = sr_amd.get_context()
    setup = dict(fold_store_mb=0, fold_seg_max=2048, vstk_rows=16, max_row_blocks=20, chunk_min=64)
    setup.update(knobs)
    try:
        for k, v in setup.items():
            ctx.set_tuning(k, v)
        loss, comp = eval_loss_batch(tb, ds, opts)
        info = ctx.last_ref_fold()
        info.update(chunks=ctx.last_launches(), exact=ctx.last_exact_trees())
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_tuning(k, v)
    return loss, comp, info


def _same(a, b):
    """Two calls' (loss, complete): the same flags and the same bits."""
    (la, ca, _), (lb, cb, _) = a, b
    return (np.array_equal(ca, cb) and np.array_equal(np.isfinite(la), np.isfinite(lb)) and
            np.array_equal(_bits(la[np.isfinite(la)]), _bits(lb[np.isfinite(lb)])))


@pytest.fixture(scope="module")
def opts():
    return Options(**OPTS)


@pytest.fixture(scope="module")
def trees(opts):
    """The population with the BIG trees planted in its first, middle and last sixth."""
    pop = gen_random_population(1200, opts, 5, max_size=30, seed=7)
    big = [parse_expression(e, opts) for e in BIG]
    return pop[:100] + big[:2] + pop[100:700] + big[2:4] + pop[700:] + big[4:]


@pytest.fixture(scope="module")
def population(opts, trees):
    return flatten_trees(trees, np.float32)


@pytest.fixture(scope="module")
def predictions(opts, population):
    """The device's own predictions of the population on the module's dataset, computed once."""
    X, y, _ = _data(N)
    pred, _ = eval_tree_array_batch(population, Dataset(X, y), opts)
    return pred


@pytest.mark.parametrize("weighted", [False, True])
def test_every_combination_gives_the_same_bits(opts, population, predictions, weighted):
    X, y, w = _data(N)
    w = w if weighted else None
    ds = Dataset(X, y, weights=w)
    base = _run(population, ds, opts, **OFF)
    l0, c0, i0 = base
    print("weighted", weighted, "all 0:", i0)
    assert i0["path"] == 2 and i0["chunks"] == 2 and i0["exact"] >= len(BIG), i0
    assert c0[[100, 101, 702, 703, 1204, 1205]].all()  # (the planted trees' sums are finite: complete)
    fin = c0 & np.isfinite(l0)
    assert fin.sum() > 300
    for tail in (0, 1, 2, 4, 6):
        for early in (0, 1):
            r = _run(population, ds, opts, tail_chunk=tail, exact_early=early)
            print("weighted", weighted, "tail_chunk", tail, "exact_early", early, r[2])
            assert r[2]["path"] == 2 and r[2]["exact"] == i0["exact"], r[2]
            assert r[2]["chunks"] == (2 if tail == 0 else 3), r[2]
            assert r[2]["folded"] == i0["folded"] and r[2]["fallback"] == i0["fallback"], (r[2], i0)
            assert _same(r, base), (tail, early)
    # the all-0 result: numpy's sequential Float32 fold of the device's own predictions
    idx = np.nonzero(fin)[0]
    want = np.array([_np_fold_losses(predictions[t], y, w) for t in idx], dtype=np.float32)
    bad = idx[_bits(l0[idx]) != _bits(want)]
    assert bad.size == 0, (bad[:5], l0[bad[:5]], want[:5])


def test_the_same_call_three_times(opts, population):
    """Every knob on, the same call three times: an ordering mistake between the streams would show as bits
    that depend on the run."""
    X, y, _ = _data(N)
    ds = Dataset(X, y)
    base = _run(population, ds, opts, **OFF)
    for k in range(3):
        r = _run(population, ds, opts, **ON)
        print("run", k, r[2])
        assert r[2]["chunks"] == 3 and r[2]["exact"] > 0 and r[2]["path"] == 2, r[2]
        assert _same(r, base), k


def test_last_chunk_without_a_complete_tree(opts, trees):
    """700 incomplete trees at the end of the batch: the last chunk (a third of the trees) has no complete
    tree, so its chain has nothing to fold."""
    dead = [parse_expression(f"log(x1 - x1) * {1.0 + 0.5 * k}", opts) for k in range(700)]
    tb = flatten_trees(trees + dead, np.float32)
    X, y, _ = _data(N)
    ds = Dataset(X, y)
    base = _run(tb, ds, opts, **OFF)
    r = _run(tb, ds, opts, **ON)
    print("dead tail, all 0:", base[2], "all on:", r[2])
    assert r[2]["chunks"] == 3 and base[2]["chunks"] == 2 and r[2]["path"] == 2
    assert tb.n_trees - tb.n_trees * ON["tail_chunk"] // 12 >= len(trees)  # (the last chunk starts inside the dead trees)
    assert not r[1][len(trees):].any() and r[1][:len(trees)].sum() > 300
    assert _same(r, base)
    assert r[2]["folded"] == base[2]["folded"] and r[2]["exact"] == base[2]["exact"] > 0


def test_two_launch_regions_per_chunk(opts, trees):
    """Trees too deep for the register stack run in a second launch of the chunk, the LDS-stack kernel's, with
    a chain of its own: planted in every chunk."""
    def deep(k):
        c = 1.0 + 0.125 * k
        return parse_expression(
            f"(((x1 + x2) * (x3 - x4)) + ((x5 * {c}) - (x2 * x3))) * (((x4 + x1) * (x2 - x5)) + ((x3 * x1) - (x4 * {c})))",
            opts)
    d = [deep(k) for k in range(36)]
    assert compile_info(opts, flatten_trees(d, np.float32), N, 5, np.float32)[3] > 2  # (operand-stack slots)
    mixed = d[:12] + trees[:600] + d[12:24] + trees[600:] + d[24:]
    tb = flatten_trees(mixed, np.float32)
    X, y, _ = _data(N)
    ds = Dataset(X, y)
    base = _run(tb, ds, opts, **OFF)
    assert base[1][:12].all() and np.isfinite(base[0][:12]).all()
    for knobs in (ON, dict(ON, exact_early=0), dict(OFF, exact_early=1), dict(ON, tail_chunk=2)):
        r = _run(tb, ds, opts, **knobs)
        print(knobs, r[2])
        assert r[2]["path"] == 2 and r[2]["chunks"] == (3 if knobs["tail_chunk"] else 2), r[2]
        assert _same(r, base), knobs
    pred, _ = eval_tree_array_batch(tb.take(np.arange(12)), ds, opts)
    want = np.array([_np_fold_losses(pred[k], y) for k in range(12)], dtype=np.float32)
    assert np.array_equal(_bits(base[0][:12]), _bits(want)), (base[0][:12], want)


def test_other_calls_keep_their_schedule(opts, population):
    """A single-chunk call (the default "chunk_min") and a gathered call: the same bits with every knob on,
    and the chunk count unchanged."""
    X, y, _ = _data(N)
    ds = Dataset(X, y)
    a = _run(population, ds, opts, chunk_min=1024, **ON)
    b = _run(population, ds, opts, chunk_min=1024, **OFF)
    print("one chunk:", a[2], b[2])
    assert a[2]["chunks"] == 1 and b[2]["chunks"] == 1 and a[2]["path"] == 2 and a[2]["exact"] > 0
    assert _same(a, b)
    rows = np.random.default_rng(5).permutation(N)[:30_000]
    sub = SubDataset(ds, rows)
    g1 = _run(population, sub, opts, **ON)
    g0 = _run(population, sub, opts, **OFF)
    print("gathered:", g1[2], g0[2])
    assert g1[2]["chunks"] == 2 and g0[2]["chunks"] == 2 and g1[2]["path"] == 2 and g1[2]["exact"] > 0, (g1[2], g0[2])
    assert _same(g1, g0)
