"""GPU: the listed loss launch ("loss_compact"; csrc/sr_aux.hip sr_loss_compact_kernel).

The candidate-composing loss launch of a large plain call runs over the launch positions its chunk's dead-tree
probe left alive — one list per launch, G entries per workgroup — and the reduce gives the excluded positions
their result (Σ 0, non-finite) without reading a partial.  It only chooses which workgroup runs which tree:
no bit of any result may change.

Shapes: 2^18 rows (256 row blocks; the register-stack kernel at 16 rows per lane) x 600 .. 1,100 trees (path 2
under the default "fold_store_mb"; one chunk of >= 512 trees has a probe), the smallest at which the probe, the
candidate launch and so the list run.  The populations are written out — trees finite on every row, trees
non-finite on every row (the probe marks them, whatever its rows), statically incomplete ones (left out by
their flag) — so that every
case knows its list's length; the counters come from sr_last_phase_ms out[16..18].

Every case: "loss_compact" 1 against 0 bit for bit (losses and flags), the same trees through the exact-sum
pass and the in-order fold, and a sample of complete trees against numpy's sequential Float32 fold of the
device's own predictions.
"""
import ctypes

import numpy as np
import pytest

import sr_amd
from bytecode_vm import compile_info
from oracle import Oracle
from sr_amd import _lib, Dataset, Options, eval_loss_batch, eval_tree_array_batch, flatten_trees, parse_expression

pytestmark = pytest.mark.gpu

OPTS = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "log"])
N = 1 << 18
ROW = 100_003  # x1 == x2 here and nowhere else (test_dead_off_the_stress_rows)
DEFAULTS = dict(loss_compact=1, chunk_min=1024)


@pytest.fixture(scope="module")
def opts():
    return Options(**OPTS)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(2)
    X = rng.standard_normal((5, N)).astype(np.float32)
    # an ordinary row (no feature's extreme or nearest-zero value: not among the probe's stress rows)
    r = ROW
    while not all(0.25 < abs(float(X[f, r])) < 1.5 for f in range(5)):
        r += 1
    assert r == ROW, r  # (the seed's row: kept literal so that the docstrings can name it)
    X[1, ROW] = X[0, ROW]
    assert int((X[0] == X[1]).sum()) == 1
    y = (2 * np.cos(X[3]) + X[0] ** 2 - 2 + 0.1 * rng.standard_normal(N)).astype(np.float32)
    return X, y, Dataset(X, y)


def _live(k):
    """Finite on every row."""
    c = 1.0 + 0.01 * k
    return (f"x1 * {c} + x2", f"cos(x3 * {c}) - x4", f"(x1 * x2) * {c} + exp(x5 * 0.5)", f"x2 - cos(x1 + {c})")[k % 4]


def _dead(k):
    """Non-finite on every row: log of a negative number, 0 / 0 or x / 0."""
    c = 1.0 + 0.01 * k
    return (f"log((0.0 - x1 * x1) - {c})", f"log(cos(x2) - {c + 1.0})", f"x3 / (x1 - x1) + {c}")[k % 3]


def _static(k):
    """Incomplete at compile time (a constant subtree that is NaN): an empty program."""
    return f"x{1 + k % 5} + log(0.0 - {1.0 + k})"


def _mix(opts, n_live, n_dead, n_static=0, extra=()):
    """The trees interleaved (the launch order sorts them by cost anyway); `extra` expressions go in the middle.
    Returns the batch and the indices of the extras."""
    ex = [_live(k) for k in range(n_live)] + [_dead(k) for k in range(n_dead)] + [_static(k) for k in range(n_static)]
    order = np.random.default_rng(11).permutation(len(ex))
    ex = [ex[i] for i in order]
    at = len(ex) // 2
    ex[at:at] = list(extra)
    return flatten_trees([parse_expression(e, opts) for e in ex], np.float32), np.arange(at, at + len(extra))


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _np_fold_loss(pred, y):
    """LossFunctions' L2 mean in Float32 and in row order (numpy's add.accumulate is a sequential left fold)."""
    d = (pred - y).astype(np.float32)
    return np.float32(np.add.accumulate(d * d, dtype=np.float32)[-1] / np.float32(len(y)))


def _run(tb, ds, opts, **knobs):
    """One call; every knob back to its default afterwards.  info: the fold's path, trees through the exact
    pass / the in-order fold, chunks, and the listed launches with their listed and excluded positions."""
    ctx = sr_amd.get_context()
    try:
        for k, v in knobs.items():
            ctx.set_tuning(k, v)
        loss, comp = eval_loss_batch(tb, ds, opts)
        out = (ctypes.c_double * 19)()
        _lib.check(_lib.lib.sr_last_phase_ms(ctx.handle, out, 19))
        ref = ctx.last_ref_fold()
        info = dict(path=ref["path"], folded=ref["folded"], fallback=ref["fallback"], exact=ctx.last_exact_trees(),
                    fold=ctx.last_fold_trees(),
                    chunks=ctx.last_launches(), listed=int(out[16]), live=int(out[17]), excl=int(out[18]))
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_tuning(k, v)
    return loss, comp, info


def _check(tb, data, opts, launches=1, **knobs):
    """The three comparisons; returns the listed call's (loss, complete, info)."""
    X, y, ds = data
    r1 = _run(tb, ds, opts, loss_compact=1, **knobs)
    r0 = _run(tb, ds, opts, loss_compact=0, **knobs)
    (l1, c1, i1), (l0, c0, i0) = r1, r0
    print("loss_compact 1:", i1, "0:", i0)
    assert i1["path"] == 2 and i0["path"] == 2, (i1, i0)
    assert i1["listed"] == launches and i0["listed"] == 0 and i0["live"] == 0 and i0["excl"] == 0, (i1, i0)
    assert np.array_equal(c1, c0)
    assert np.array_equal(_bits(l1), _bits(l0)), np.nonzero(_bits(l1) != _bits(l0))[0][:8]
    assert np.all(np.isinf(l1[~c1]))
    assert i1["exact"] == i0["exact"] and i1["fold"] == i0["fold"], (i1, i0)
    assert i1["folded"] == i0["folded"] and i1["fallback"] == i0["fallback"], (i1, i0)
    fin = np.nonzero(c1 & np.isfinite(l1))[0]
    if len(fin):
        idx = fin[:: max(1, len(fin) // 8)][:8]
        pred, _ = eval_tree_array_batch(tb.take(idx), ds, opts)
        want = np.array([_np_fold_loss(pred[k], y) for k in range(len(idx))], dtype=np.float32)
        assert np.array_equal(_bits(l1[idx]), _bits(want)), (idx, l1[idx], want)
    return r1


@pytest.mark.parametrize("n_live,n_dead", [(333, 367), (50, 550), (256, 344), (0, 600), (600, 0)],
                         ids=["mixed", "few_live", "full_groups", "all_dead", "none_dead"])
def test_list_lengths(opts, data, n_live, n_dead):
    """333 listed positions (no multiple of the launch's 128 positions per workgroup nor of the 4 waves), 50 (less
    than one workgroup's), 256 (a multiple of 128), none (every workgroup returns at once) and all 600 (the list is
    the identity).  The list is dealt over the launch's tree groups, so a workgroup takes ceil(listed / groups)
    entries, rounded up to the waves and to at least 32: ragged last workgroups and last waves in the first three."""
    tb, _ = _mix(opts, n_live, n_dead)
    l, c, info = _check(tb, data, opts)
    assert info["live"] == n_live and info["excl"] == n_dead, info
    assert int(c.sum()) == n_live


def test_dead_off_the_stress_rows(opts, data):
    """1 / (x1 - x2) with x1 == x2 at row 100,003 alone, an ordinary row the probe does not run: the tree is on
    the list, its row block finds it inside the listed launch and marks the tree's own launch position (a mark at
    its place in the list would kill a live tree's later row blocks and change that tree's result)."""
    X, y, _ = data
    tb, at = _mix(opts, 333, 367, extra=["1.0 / (x1 - x2)"])
    _, oc = Oracle.from_options(opts).eval_loss_batch(tb.take(at), X, y)
    assert not oc[0]  # (the reference's own verdict)
    l, c, info = _check(tb, data, opts)
    assert info["live"] == 334 and info["excl"] == 367, info
    assert not c[at[0]] and np.isinf(l[at[0]]) and int(c.sum()) == 333


def test_empty_programs(opts, data):
    """Statically incomplete trees (empty programs) among the live and the dead: the probe never runs them and
    leaves no hint, the list leaves them out by their static flag, and the reduce gives them that flag."""
    tb, _ = _mix(opts, 300, 330, n_static=7)
    l, c, info = _check(tb, data, opts)
    assert info["live"] == 300 and info["excl"] == 337, info
    assert int(c.sum()) == 300


def test_big_trees_reach_the_exact_pass(opts, data):
    """Planted trees whose values pass the deferred checks' bound (the exact-sum pass decides them: complete)."""
    tb, at = _mix(opts, 333, 367, extra=["x1 * 5.0e34", "cos(x1) * 2.0e33"])
    l, c, info = _check(tb, data, opts)
    assert info["exact"] >= 2 and c[at].all(), (info, c[at])
    assert info["live"] == 335 and info["excl"] == 367, info


def test_deep_trees_beside_the_list(opts, data):
    """Trees too deep for the register stack: the chunk's second launch (the LDS-stack kernel, no probe, every
    position) runs beside the listed one."""
    def deep(k):
        c = 1.0 + 0.125 * k
        return (f"(((x1 + x2) * (x3 - x4)) + ((x5 * {c}) - (x2 * x3))) * "
                f"(((x4 + x1) * (x2 - x5)) + ((x3 * x1) - (x4 * {c})))")
    d = [deep(k) for k in range(12)]
    assert compile_info(opts, flatten_trees([parse_expression(e, opts) for e in d], np.float32), N, 5, np.float32)[3] > 2
    tb, at = _mix(opts, 333, 367, extra=d)
    l, c, info = _check(tb, data, opts)
    assert info["live"] == 333 and info["excl"] == 367, info  # (the listed launch's positions only)
    assert c[at].all() and np.isfinite(l[at]).all()


def test_several_chunks(opts, data):
    """"chunk_min" 64: three chunks; the first (a sixth of the trees, fewer than 512) has no probe and keeps the
    full launch, the other two are listed, each with its own list and counter."""
    tb, _ = _mix(opts, 500, 600)
    l, c, info = _check(tb, data, opts, launches=2, chunk_min=64)
    assert info["chunks"] == 3, info
    assert info["live"] > 0 and info["excl"] > 0 and 1100 // 2 < info["live"] + info["excl"] < 1100, info
    assert int(c.sum()) == 500
