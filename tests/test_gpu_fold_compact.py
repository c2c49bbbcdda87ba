"""GPU: the compacted FOLD re-run ("fold_compact") and the candidates' guess from the running prefix
("fold_cand_est") of a large call's in-order loss fold (path 2; csrc/sr_fold_dev.h).

* The FOLD pass used to launch the loss launch's grid again and found one or two trees per wave left: it now
  runs over per-row-block lists of the positions the plan left it (sr_fold_compact_kernel), G per workgroup.
* The loss launch guesses the running sum's binade at a row block from the tree's row blocks other
  workgroups have already finished instead of from the block's first tile alone.

Both only choose what is computed where: every composition is exact and the plan verifies each candidate
before taking it, so no bit of any result may change, whatever the timing.  `taken` and `rerun` become
run-dependent with the guess on; their sum does not.

Shapes: tests/test_gpu_fold_single_pass.py's (40,000 rows, "fold_store_mb" 0, "fold_seg_max" 2048,
"vstk_rows" 16, "max_row_blocks" 20: 20 row blocks of two 1,024-row tiles), and 2^19 rows as 512 one-tile
row blocks for the guess, so that more workgroups are launched than can be resident.
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
                max_row_blocks=512, fold_compact=1, fold_cand_est=1)


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


def _run(tb, ds, opts, **knobs):
    """One path-2 call at the module's shapes; every knob back to its default afterwards."""
    ctx = sr_amd.get_context()
    setup = dict(fold_store_mb=0, fold_seg_max=2048, vstk_rows=16, max_row_blocks=20)
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


def _same(a, b):
    """Two calls' (loss, complete): the same flags and the same bits."""
    (la, ca, _), (lb, cb, _) = a, b
    return (np.array_equal(ca, cb) and np.array_equal(np.isfinite(la), np.isfinite(lb)) and
            np.array_equal(_bits(la[np.isfinite(la)]), _bits(lb[np.isfinite(lb)])))


@pytest.fixture(scope="module")
def population():
    opts = Options(**OPTS)
    return opts, flatten_trees(gen_random_population(1200, opts, 5, max_size=30, seed=7), np.float32)


@pytest.fixture(scope="module")
def predictions(population):
    """The device's own predictions of the population on the module's dataset (the same X with and without
    weights), computed once."""
    opts, tb = population
    X, y, _ = _data(N)
    pred, _ = eval_tree_array_batch(tb, Dataset(X, y), opts)
    return pred


@pytest.mark.parametrize("weighted", [False, True])
def test_all_combinations_give_the_same_bits(population, predictions, weighted):
    opts, tb = population
    X, y, w = _data(N, weighted=weighted)
    ds = Dataset(X, y, weights=w)
    base = _run(tb, ds, opts, fold_single_pass=0)
    l0, c0, i0 = base
    assert i0["path"] == 2 and i0["taken"] == 0 and i0["rerun"] > 0, i0
    fin = c0 & np.isfinite(l0)
    assert fin.sum() > 300
    for compact in (0, 1):
        for est in (0, 1):
            r = _run(tb, ds, opts, fold_compact=compact, fold_cand_est=est)
            print("weighted", weighted, "fold_compact", compact, "fold_cand_est", est, r[2])
            assert r[2]["path"] == 2, r[2]
            assert _same(r, base), (compact, est)
            assert r[2]["taken"] > 0 and r[2]["taken"] + r[2]["rerun"] == i0["rerun"], (r[2], i0)
    # ... and without the candidates: the compacted launch runs every block of every complete tree
    assert _same(_run(tb, ds, opts, fold_single_pass=0, fold_compact=0), base)
    idx = np.nonzero(fin)[0]
    want = np.array([_np_fold_losses(predictions[t], y, w) for t in idx], dtype=np.float32)
    bad = idx[_bits(l0[idx]) != _bits(want)]
    assert bad.size == 0, (bad[:5], l0[bad[:5]], want[:5])


def test_prefix_guess_engaged(population):
    """2^19 rows as 512 one-tile row blocks x 1,200 trees: ~5k workgroups of the loss launch, about 1,000 of
    them resident at a time, so all but a tree's last ~100 row blocks have finished when a block starts and the
    guess comes from the running prefix.

    The bound, from `python tools/fold_cand_sim.py --data test --rows 524288 --trees 1200 --seed 7
    --block-rows 1024 --every 1 --lag 32 64 128 192 256 --min-count 4` (CPU, this dataset and population, 407
    complete trees x 512 blocks; ties not modelled): pairs left to the FOLD pass, one candidate (the build's
    default), 26.83 % with the first-tile guess; 9.34 / 13.18 / 17.65 / 20.60 / 22.51 % with the prefix guess at
    a lag of 32 / 64 / 128 / 192 / 256 row blocks (2.98 % are slow in the plan whatever the guess).  With two
    candidates (-DSR_FCAND_N=2): 19.87 %; 6.55 / 8.95 / 12.60 / 15.55 / 17.51 %.  Expected lag ~100 blocks
    (1,024 resident workgroups over 10 tree groups): a ratio of ~0.6 under either build (measured: one
    candidate 34,129 / 57,452 = 0.59, two 22,659 / 43,108 = 0.53).  Required: rerun(est 1) <= 0.8 x
    rerun(est 0), which a lag of up to ~190 blocks still meets (0.77 / 0.78 at 192)."""
    opts, tb = population
    n = 1 << 19
    X, y, _ = _data(n)
    ds = Dataset(X, y)
    knobs = dict(fold_seg_max=1024, max_row_blocks=512)
    r1 = _run(tb, ds, opts, fold_cand_est=1, **knobs)
    r0 = _run(tb, ds, opts, fold_cand_est=0, **knobs)
    (l1, c1, i1), (l0, c0, i0) = r1, r0
    print("prefix guess on:", i1, "off:", i0, "rerun ratio", i1["rerun"] / max(1, i0["rerun"]))
    assert i1["path"] == 2 and i0["path"] == 2, (i1, i0)
    assert _same(r1, r0)
    total = i0["taken"] + i0["rerun"]
    assert total == i1["taken"] + i1["rerun"] and total % 512 == 0 and total // 512 > 300, (i1, i0)
    fin = np.nonzero(c1 & np.isfinite(l1))[0]
    idx = fin[:: max(1, len(fin) // 24)][:24]
    pred, _ = eval_tree_array_batch(tb.take(idx), ds, opts)
    want = np.array([_np_fold_losses(pred[k], y) for k in range(len(idx))], dtype=np.float32)
    assert np.array_equal(_bits(l1[idx]), _bits(want)), (idx, l1[idx], want)
    assert i1["rerun"] <= 0.8 * i0["rerun"], (i1, i0)


def _simple_trees(opts, n_plain, n_heavy):
    """Complete trees: smooth ones (nearly every block's pair is taken: their row blocks' lists are empty)
    and heavy-tailed ones (the guess misses: they stay on the lists)."""
    ex = [f"x1 * {1.0 + 0.125 * k}" for k in range(n_plain)]
    ex += [f"exp(x1 * x1 * 1.5) * {1.0 + 0.25 * k}" for k in range(n_heavy)]
    return flatten_trees([parse_expression(e, opts) for e in ex], np.float32)


@pytest.mark.parametrize("n_plain,n_heavy", [(1, 0), (4, 0), (5, 0), (6, 2), (7, 2), (9, 3), (12, 4), (13, 4), (29, 4)])
def test_list_edges(n_plain, n_heavy):
    """The lists' edge cases: one complete tree (every block the plan took is a row block with no entry); the
    first row block lists every tree — these counts are multiples of the small calls' G = 4 trees per
    workgroup (4, 8, 16), one more (5, 9, 13, 17) and in between."""
    X, y, _ = _data(N, seed=6)
    opts = Options(**OPTS)
    tb = _simple_trees(opts, n_plain, n_heavy)
    ds = Dataset(X, y)
    r1 = _run(tb, ds, opts, fold_compact=1)
    r0 = _run(tb, ds, opts, fold_compact=0)
    print(n_plain, n_heavy, "compact:", r1[2], "grid:", r0[2])
    assert r1[1].all() and np.isfinite(r1[0]).all() and r1[2]["path"] == 2, r1[2]
    assert _same(r1, r0)
    assert r1[2]["taken"] > 0  # (with one tree: row blocks with nothing listed)
    assert r1[2]["taken"] + r1[2]["rerun"] == 20 * (n_plain + n_heavy), r1[2]
    pred, _ = eval_tree_array_batch(tb, ds, opts)
    want = np.array([_np_fold_losses(pred[k], y) for k in range(tb.n_trees)], dtype=np.float32)
    assert np.array_equal(_bits(r1[0]), _bits(want)), (r1[0], want)


@pytest.mark.parametrize("n", [40_001, 1_000])
def test_view_no_multiple_of_the_tile(n):
    """A view that is no multiple of the tile, and a call of one row block (every tree on its one list)."""
    X, y, _ = _data(n, seed=8)
    opts = Options(**OPTS)
    tb = flatten_trees(gen_random_population(300, opts, 5, max_size=30, seed=13), np.float32)
    ds = Dataset(X, y)
    r1 = _run(tb, ds, opts, fold_compact=1)
    r0 = _run(tb, ds, opts, fold_compact=0)
    print("n", n, "compact:", r1[2], "grid:", r0[2])
    assert r1[2]["path"] == 2 and r0[2]["path"] == 2
    assert _same(r1, r0)
    l1, c1, _ = r1
    idx = np.nonzero(c1 & np.isfinite(l1))[0][:60]
    pred, _ = eval_tree_array_batch(tb.take(idx), ds, opts)
    want = np.array([_np_fold_losses(pred[k], y) for k in range(len(idx))], dtype=np.float32)
    assert np.array_equal(_bits(l1[idx]), _bits(want))


@pytest.mark.parametrize("compact", [1, 0])
def test_exact_half_ulp_ties(compact):
    """tests/test_gpu_fold_single_pass.py's construction: losses that are exact multiples of 2^-12 under running
    sums near 2^17 (ulp 2^-6 ... 2^-7), about one row in 64 an exact half-ulp tie, which poisons a candidate —
    the blocks stay on the lists and take the FOLD pass's ordered composition.  The reference needs no device."""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((5, N)).astype(np.float32)
    X[0] = (rng.integers(0, 256, N) / 64.0).astype(np.float32)
    y = np.zeros(N, dtype=np.float32)
    opts = Options(**OPTS)
    tb = flatten_trees([parse_expression(e, opts) for e in ("x1", "x1 * 1.0", "x1 + 0.0")], np.float32)
    loss, comp, info = _run(tb, Dataset(X, y), opts, fold_compact=compact)
    print("ties, fold_compact", compact, info)
    assert info["path"] == 2 and comp.all(), info
    want = np.float32(np.add.accumulate((X[0] * X[0]).astype(np.float32), dtype=np.float32)[-1] / np.float32(N))
    assert np.array_equal(_bits(loss), _bits(np.full(3, want, dtype=np.float32))), (loss, want, info)


def test_slot_shortage(population):
    """128 slow-segment slots for 1,200 trees: the trees that find no slot are SKIP everywhere but their first
    block and take the fallback; the lists change nothing of that."""
    opts, tb = population
    X, y, _ = _data(N)
    ds = Dataset(X, y)
    r1 = _run(tb, ds, opts, fold_compact=1, fold_slot_mb=1)
    r0 = _run(tb, ds, opts, fold_compact=0, fold_slot_mb=1)
    rd = _run(tb, ds, opts, fold_compact=1)
    print("1 MB of slots, compact:", r1[2], "grid:", r0[2], "default slots:", rd[2])
    # (which trees get the slots is a race on the call's slot counter: the counts vary from run to run, their
    #  sum — every complete tree with a finite loss, folded one way or the other — does not)
    n_fin = int((rd[1] & np.isfinite(rd[0])).sum())
    for r in (r1, r0):
        assert r[2]["fallback"] > 0 and r[2]["folded"] + r[2]["fallback"] == n_fin, (r[2], n_fin)
    assert _same(r1, r0) and _same(r1, rd)
