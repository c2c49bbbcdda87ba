"""GPU: the compacted FOLD launch's entries per workgroup ("fold_list_wgs"; csrc/sr_aux.hip
sr_fold_compact_scan_kernel, csrc/sr_plan.h sr_fold_list_g).

The FOLD re-run of a large call runs over per-row-block lists of the positions the plan left it.  Its
workgroups took G entries each, G the launch's trees per workgroup; with "fold_list_wgs" > 0 the scan chooses g
from the row blocks' counts: the smallest multiple of the 4 waves, 4 <= g <= G, whose live workgroups (the sum
over the row blocks of ceil(count / g)) stay within the target and within the launch's grid, G when none does.
It only chooses which workgroup runs which listed tree: no bit of any result may change, and the plan's
`taken + rerun` does not depend on it.

Shapes: tests/test_gpu_fold_compact.py's (40,000 rows, "fold_store_mb" 0, "fold_seg_max" 2048, "vstk_rows" 16,
"max_row_blocks" 20: 20 row blocks of two 1,024-row tiles).  Such small calls have G = 4, which leaves g no
choice, so the cases set "trees_per_block" (every grid's G):
  G 8,   target 2^20: g = 4 — 1,200 trees are 150 groups x 20 row blocks = 3,000 workgroups of grid, and up to
         596 complete trees (the population has 411) x 20 / 4 + 20 workgroups at g = 4 fit it, whatever the plan
         took;
  G 128, target 150:  4 < g < 128 — row block 0 lists every complete tree with a finite loss (over 300: more than
         75 workgroups at g = 4, and the other 19 row blocks' lists come on top), and g = 124 needs at most
         596 x 20 / 124 + 20 = 117;
  G 128, target 2^20, "fold_single_pass" 0: every complete tree on every list, 10 groups x 20 = 200 workgroups
         of grid: g must grow until the launch fits it.
sr_last_phase_ms out[19 + 4 r ..] reports region r's {live workgroups, listed entries, g, longest list}.

The listed loss launch ("loss_compact") needs test_gpu_loss_compact.py's 2^18 rows and written-out populations:
the cases at the end run those, the all-dead population (every list empty) and the one with 50 live trees
among them.
"""
import ctypes

import numpy as np
import pytest

import sr_amd
from sr_amd import (_lib, Dataset, Options, eval_loss_batch, eval_tree_array_batch, flatten_trees,
                    gen_random_population, parse_expression)

pytestmark = pytest.mark.gpu

OPTS = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "log"])
N = 40_000
BIG = 1 << 20
DEFAULTS = dict(fold_single_pass=1, fold_store_mb=512, fold_seg_max=16384, vstk_rows=0, fold_slot_mb=24576,
                max_row_blocks=512, fold_compact=1, fold_cand_est=1, fold_list_wgs=2048, trees_per_block=0,
                loss_compact=1)
SMALL = dict(fold_store_mb=0, fold_seg_max=2048, vstk_rows=16, max_row_blocks=20)


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


def _run(tb, ds, opts, setup=SMALL, **knobs):
    """One call under `setup` and the knobs; every knob back to its default afterwards.  info: the fold's path
    and trees, the plan's pairs, the listed loss launches, and per compacted FOLD launch (region) its
    {wgs, entries, g, longest}."""
    ctx = sr_amd.get_context()
    setup = dict(setup, **knobs)
    try:
        for k, v in setup.items():
            ctx.set_tuning(k, v)
        loss, comp = eval_loss_batch(tb, ds, opts)
        info = ctx.last_ref_fold()
        info.pop("kernel_ms")
        info.update(ctx.last_fold_cand())
        out = (ctypes.c_double * 51)()
        _lib.check(_lib.lib.sr_last_phase_ms(ctx.handle, out, 51))
        info["listed"] = int(out[16])
        info["lists"] = [dict(region=r, wgs=int(out[19 + 4 * r]), entries=int(out[20 + 4 * r]), g=int(out[21 + 4 * r]),
                              longest=int(out[22 + 4 * r])) for r in range(8) if out[21 + 4 * r] > 0]
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


# (trees per workgroup G, "fold_list_wgs", further knobs): the module docstring's cases
CASES = [(8, 0, {}), (8, BIG, {}), (128, 0, {}), (128, 150, {}), (128, BIG, {}), (128, BIG, dict(fold_single_pass=0))]


@pytest.mark.parametrize("weighted", [False, True])
def test_all_combinations_give_the_same_bits(population, predictions, weighted):
    opts, tb = population
    X, y, w = _data(N, weighted=weighted)
    ds = Dataset(X, y, weights=w)
    base = _run(tb, ds, opts, fold_list_wgs=0, loss_compact=0)  # (all-zero: G = 4, the call's own)
    l0, c0, i0 = base
    print("weighted", weighted, "all-zero", i0)
    assert i0["path"] == 2 and i0["rerun"] > 0 and i0["lists"], i0
    assert all(li["g"] == 4 for li in i0["lists"]), i0
    total = i0["taken"] + i0["rerun"]
    fin = c0 & np.isfinite(l0)
    n_fin = int(fin.sum())
    assert 300 < n_fin <= 596  # (the docstring's bounds hold for these)
    for G, wgs, extra in CASES:
        for lc in (0, 1):
            r = _run(tb, ds, opts, trees_per_block=G, fold_list_wgs=wgs, loss_compact=lc, **extra)
            info = r[2]
            print("weighted", weighted, "G", G, "fold_list_wgs", wgs, extra, "loss_compact", lc, info)
            assert info["path"] == 2 and info["lists"], info
            assert _same(r, base), (G, wgs, extra, lc)
            assert info["taken"] + info["rerun"] == total, (info, i0)
            assert info["folded"] == i0["folded"] and info["fallback"] == i0["fallback"], (info, i0)
            for li in info["lists"]:
                grid = 20 * (-(-tb.n_trees // G))  # (one chunk, one launch: the region's groups x row blocks)
                assert li["wgs"] <= grid and li["longest"] >= n_fin, (li, grid)
                if wgs == 0:
                    assert li["g"] == G, li
                elif G == 8:
                    assert li["g"] == 4, li
                elif wgs == 150:
                    assert 4 < li["g"] < 128 and li["g"] % 4 == 0 and li["wgs"] <= 150, li
                elif extra:  # every complete tree on every list: g grows until the launch fits its grid
                    assert li["entries"] >= 20 * n_fin, li
                    assert 4 < li["g"] < 128 and li["g"] % 4 == 0, li
                    assert li["entries"] / (li["g"] - 4) > grid - 20, li  # (g - 4 would not have fitted)
                else:
                    assert li["g"] % 4 == 0 and 4 <= li["g"] <= 128, li
    idx = np.nonzero(fin)[0]
    want = np.array([_np_fold_losses(predictions[t], y, w) for t in idx], dtype=np.float32)
    bad = idx[_bits(l0[idx]) != _bits(want)]
    assert bad.size == 0, (bad[:5], l0[bad[:5]], want[:5])


def _simple_trees(opts, n_plain, n_heavy):
    """Complete trees: smooth ones (nearly every block's pair is taken: their row blocks' lists are empty)
    and heavy-tailed ones (the guess misses: they stay on the lists)."""
    ex = [f"x1 * {1.0 + 0.125 * k}" for k in range(n_plain)]
    ex += [f"exp(x1 * x1 * 1.5) * {1.0 + 0.25 * k}" for k in range(n_heavy)]
    return flatten_trees([parse_expression(e, opts) for e in ex], np.float32)


@pytest.mark.parametrize("n_plain,n_heavy", [(1, 0), (4, 0), (5, 0), (6, 2), (7, 2), (9, 3), (12, 4), (13, 4), (29, 4),
                                             (30, 4), (44, 4), (45, 4)])
def test_list_edges(n_plain, n_heavy):
    """The lists' edge cases: one complete tree (every block the plan took is a row block with no entry); the
    first row block lists every tree — counts that are multiples of g (4, 8, 16, 48), one more (5, 9, 17, 33, 49)
    and in between (34), under G = 16 (capped at the call's trees, so G = 5 and 9 are no multiple of the waves and
    a call of up to 16 trees has 20 workgroups of grid: g = 4 fits only where few blocks list anything).  A small
    target instead makes g the smallest with at most 24 workgroups."""
    X, y, _ = _data(N, seed=6)
    opts = Options(**OPTS)
    tb = _simple_trees(opts, n_plain, n_heavy)
    n = n_plain + n_heavy
    ds = Dataset(X, y)
    r0 = _run(tb, ds, opts, fold_compact=0)
    assert r0[1].all() and np.isfinite(r0[0]).all() and r0[2]["path"] == 2 and not r0[2]["lists"], r0[2]
    for G, wgs in ((16, 0), (16, BIG), (16, 24), (0, BIG)):
        r1 = _run(tb, ds, opts, trees_per_block=G, fold_list_wgs=wgs)
        info = r1[2]
        print(n_plain, n_heavy, "G", G, "fold_list_wgs", wgs, info)
        assert _same(r1, r0), (G, wgs)
        assert info["taken"] > 0  # (with one tree: row blocks with nothing listed)
        assert info["taken"] + info["rerun"] == 20 * n, info
        (li,) = info["lists"]
        Gc = min(G or 4, n)  # (the grid's G: at most the call's trees)
        assert li["longest"] == n and li["wgs"] <= 20 * (-(-n // Gc)), li
        if wgs == 0 or Gc < 4:
            assert li["g"] == Gc, li
        else:
            assert li["g"] == Gc or (li["g"] % 4 == 0 and 4 <= li["g"] < Gc), li
        if wgs == 24 and li["g"] != Gc:
            assert li["wgs"] <= 24, li
    pred, _ = eval_tree_array_batch(tb, ds, opts)
    want = np.array([_np_fold_losses(pred[k], y) for k in range(tb.n_trees)], dtype=np.float32)
    assert np.array_equal(_bits(r0[0]), _bits(want)), (r0[0], want)


def test_view_no_multiple_of_the_tile():
    X, y, _ = _data(40_001, seed=8)
    opts = Options(**OPTS)
    tb = flatten_trees(gen_random_population(300, opts, 5, max_size=30, seed=13), np.float32)
    ds = Dataset(X, y)
    r0 = _run(tb, ds, opts)
    assert r0[2]["path"] == 2
    for G, wgs in ((32, BIG), (32, 40)):
        r1 = _run(tb, ds, opts, trees_per_block=G, fold_list_wgs=wgs)
        print("n 40001, G", G, "fold_list_wgs", wgs, r1[2], "all-zero:", r0[2])
        assert r1[2]["path"] == 2 and r1[2]["lists"]
        assert _same(r1, r0)
    l0, c0, _ = r0
    idx = np.nonzero(c0 & np.isfinite(l0))[0][:60]
    pred, _ = eval_tree_array_batch(tb.take(idx), ds, opts)
    want = np.array([_np_fold_losses(pred[k], y) for k in range(len(idx))], dtype=np.float32)
    assert np.array_equal(_bits(l0[idx]), _bits(want))


@pytest.mark.parametrize("wgs", [0, BIG])
def test_exact_half_ulp_ties(wgs):
    """tests/test_gpu_fold_single_pass.py's construction: losses that are exact multiples of 2^-12 under running
    sums near 2^17 (ulp 2^-6 ... 2^-7), about one row in 64 an exact half-ulp tie, which poisons a candidate —
    the blocks stay on the lists and take the FOLD pass's ordered composition.  The reference needs no device."""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((5, N)).astype(np.float32)
    X[0] = (rng.integers(0, 256, N) / 64.0).astype(np.float32)
    y = np.zeros(N, dtype=np.float32)
    opts = Options(**OPTS)
    ex = ["x1", "x1 * 1.0", "x1 + 0.0", "x1 - 0.0", "1.0 * x1", "0.0 + x1", "x1 / 1.0"]
    tb = flatten_trees([parse_expression(e, opts) for e in ex], np.float32)
    loss, comp, info = _run(tb, Dataset(X, y), opts, trees_per_block=8, fold_list_wgs=wgs)
    print("ties, fold_list_wgs", wgs, info)
    assert info["path"] == 2 and comp.all(), info
    want = np.float32(np.add.accumulate((X[0] * X[0]).astype(np.float32), dtype=np.float32)[-1] / np.float32(N))
    assert np.array_equal(_bits(loss), _bits(np.full(len(ex), want, dtype=np.float32))), (loss, want, info)


def test_slot_shortage(population):
    """128 slow-segment slots for 1,200 trees: the trees that find no slot are SKIP everywhere but their first
    block and take the fallback, which is still counted; the lists' dealing changes nothing of that."""
    opts, tb = population
    X, y, _ = _data(N)
    ds = Dataset(X, y)
    rd = _run(tb, ds, opts)
    n_fin = int((rd[1] & np.isfinite(rd[0])).sum())
    for G, wgs in ((0, 0), (32, BIG), (128, 150)):
        r = _run(tb, ds, opts, trees_per_block=G, fold_list_wgs=wgs, fold_slot_mb=1)
        print("1 MB of slots, G", G, "fold_list_wgs", wgs, r[2])
        # (which trees get the slots is a race on the call's slot counter: the counts vary from run to run, their
        #  sum — every complete tree with a finite loss, folded one way or the other — does not)
        assert r[2]["fallback"] > 0 and r[2]["folded"] + r[2]["fallback"] == n_fin, (r[2], n_fin)
        assert _same(r, rd)


# ---- behind a listed loss launch: tests/test_gpu_loss_compact.py's shapes (2^18 rows, 256 row blocks)
N2 = 1 << 18


def _live(k):
    c = 1.0 + 0.01 * k
    return (f"x1 * {c} + x2", f"cos(x3 * {c}) - x4", f"(x1 * x2) * {c} + exp(x5 * 0.5)", f"x2 - cos(x1 + {c})")[k % 4]


def _dead(k):
    c = 1.0 + 0.01 * k
    return (f"log((0.0 - x1 * x1) - {c})", f"log(cos(x2) - {c + 1.0})", f"x3 / (x1 - x1) + {c}")[k % 3]


@pytest.fixture(scope="module")
def data2():
    X, y, _ = _data(N2)
    return X, y, Dataset(X, y)


@pytest.mark.parametrize("n_live,n_dead", [(333, 367), (50, 550), (0, 600)], ids=["mixed", "few_live", "all_dead"])
def test_behind_a_listed_loss_launch(data2, n_live, n_dead):
    """A listed loss launch's fold chain: 333 live trees of 700; 50 (the chunk's FOLD lists are shorter than one
    workgroup's G = 128 entries); none (every tree excluded: every list is empty, no workgroup is live)."""
    X, y, ds = data2
    opts = Options(**OPTS)
    ex = [_live(k) for k in range(n_live)] + [_dead(k) for k in range(n_dead)]
    ex = [ex[i] for i in np.random.default_rng(11).permutation(len(ex))]
    tb = flatten_trees([parse_expression(e, opts) for e in ex], np.float32)
    knobs = dict(chunk_min=1024)
    r0 = _run(tb, ds, opts, setup=knobs, loss_compact=0)
    (l0, c0, i0) = r0
    assert i0["path"] == 2 and i0["listed"] == 0 and int(c0.sum()) == n_live, i0
    for lc, wgs in ((1, 0), (1, BIG), (1, 1024), (0, BIG)):
        r1 = _run(tb, ds, opts, setup=knobs, loss_compact=lc, fold_list_wgs=wgs)
        info = r1[2]
        print(n_live, n_dead, "loss_compact", lc, "fold_list_wgs", wgs, info)
        assert info["path"] == 2 and info["listed"] == lc, info
        assert np.array_equal(r1[1], c0) and np.array_equal(_bits(r1[0]), _bits(l0))
        assert info["taken"] + info["rerun"] == i0["taken"] + i0["rerun"] == 256 * n_live, (info, i0)
        assert info["folded"] == i0["folded"] and info["fallback"] == i0["fallback"], (info, i0)
        for li in info["lists"]:
            assert li["longest"] == n_live and (li["wgs"] > 0) == (n_live > 0), li
    fin = np.nonzero(c0 & np.isfinite(l0))[0]
    if len(fin):
        idx = fin[:: max(1, len(fin) // 8)][:8]
        pred, _ = eval_tree_array_batch(tb.take(idx), ds, opts)
        want = np.array([_np_fold_losses(pred[k], y) for k in range(len(idx))], dtype=np.float32)
        assert np.array_equal(_bits(l0[idx]), _bits(want)), (idx, l0[idx], want)
