"""GPU: the BASIC operator bodies per value, on every build that runs them (csrc/sr_tile_impl.h).

The hand-written row bodies pick a fast or a slow path for the whole wave with one ballot: sr_exp_rows_f32
(every |x| <= 88), sr_log_rows (every row a positive normal), sr_trig_rows_fast (every |x| < 2^20) and
sr_div_rows_f32 (every |a|, |b| in [2^-40, 2^40]).  test_gpu_libm.py looks at values through the PRED build
only and cannot say which path a value took.  Here every operator of the BASIC set gets two datasets of
4,097 rows (2 x 64 x 32 + 1: two full tiles and a ragged one at every rows-per-lane count):

  A  every row inside the operator's fast range: every full wave of every build takes the fast path;
  B  A with the last row of every aligned group of 128 rows (the smallest tile of any build: Float64 at
     2 rows per lane) replaced by an outlier outside the range whose result is small and finite
     (exp -95, log 1e-40, cos / sin 3.0e6, / a = 2^-41): every full wave of every build takes the slow path.

A holds both signs, magnitudes log-uniform over the fast range, the range's ends exactly, and the
neighbourhoods where the functions are hard (log within 2^-10 of 1, cos / sin at the Float32 nearest k pi/2
for k <= 64, exp near 0; for / 256 pairs, divisor 1 + k ulp, whose exact quotient lies 2^-24 ulp from a
rounding midpoint).  x3 is 1.0 in every row: `* x3` turns a leaf into a computed operand, value and sign of
zero unchanged.

Two ends of those ranges cannot stand in a dataset whose trees stay complete on the BASIC builds, and are
replaced by the nearest that can:
  * log at floatmax: data at or above floatmax / (2 rows x tree nodes) sends a loss call to the per-node-check
    (FULL tier) kernels (choose_kernels), and a checked array that holds floatmax beside other positive values has
    no finite sum.  "log" tops out at 2^100 and runs both checks; "log_top" runs check 1 alone: one row at
    floatmax and the others at most 2^60, so that the feature's own sum (which PRED validates before a unary
    operator, in Float64) is floatmax itself and the tree complete.
  * exp at +88.0: e^88 is above the deferred checks' bound, so the tree goes through the exact-sum pass
    instead of keeping the loss launch's result (at 2^18 rows from e^73.4 on).  "exp" keeps x in [-88, 72]
    (-88.0 exactly: the ballot tests |x|) and asserts that no tree took the exact pass; "exp_top" is the same
    dataset with one row at +88.0 and runs through that pass.

Check 1 (PRED, per value): + - * / sqrt square cube neg abs bit-equal to numpy in T; Float32 cos / sin / log
bit-equal to the library's host function (sr_host_unary: exhaustively pinned on the CPU) and within F32_BAR of
numpy's Float64 value; Float32 exp within 1 ulp of it; Float64 transcendentals within 1 ulp on the
libm_ulp.json points that fill the last rows; and every row A and B share has the same bits in both.

Check 2 (every build, through the loss): PRED's output becomes y and the same operator is scored under L2, L1
and Huber(1.0) — the L2-folded, L1-folded and generic builds, each exactly 0 where d = 0 — over every knob
setting of test_gpu_build_table._knob_cases, the full view and a row view (a permutation that keeps every
aligned 128-row group together), plain and parametric.  The loss must be exactly 0.0 and the tree complete:
the build produced PRED's bits in every row.  One control per dtype shows that the channel sees one ulp in
one row.  The operand forms each tree is there for are asserted from the compiled programs; one form per operator
needs more than two operand-stack slots, so that the LDS-stack builds (the only ones at 16 and 32 rows per lane
beside the register-stack builds) run the operator too.

LOAD_DERIVED (`u(x1)` computed once per call by sr_launch_derived) is not visible through sr_compile_info, which
compiles without a column map, and no call below 16,384 rows uses it: the 2^18-row case asserts it from the
call's own count (last_derived_columns), on the fast path, on the slow path and over a gathered view.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import sr_amd
from bytecode_vm import compile_info
from parametric_util import to_parametric
from sr_amd import _lib, Dataset, Options, batch, eval_loss_batch, eval_tree_array_batch, flatten_trees, parse_expression
from test_gpu_build_table import DEFAULTS, _knob_cases
from test_gpu_libm import F32_BAR, host_unary, ulp_errors

HERE = os.path.dirname(os.path.abspath(__file__))
N, GROUP = 4097, 128
OUT_AT = np.arange(GROUP - 1, N - 1, GROUP)  # B's outliers: the last row of each of the 32 full groups
SHARED = np.setdiff1d(np.arange(N), OUT_AT)
UNARY = ("exp", "cos", "sin", "log", "sqrt", "square", "cube", "neg", "abs")
BINARY = ("+", "-", "*", "/")
OPTS = dict(binary_operators=list(BINARY), unary_operators=list(UNARY))
LOSSES = ("L2DistLoss()", "L1DistLoss()", "HuberLoss(1.0)")
DTYPES = {"float32": np.float32, "float64": np.float64}
OUTLIER = {"exp": -95.0, "log": 1e-40, "cos": 3.0e6, "sin": 3.0e6, "/": 2.0 ** -41}
C_IN, C_OUT = 3.0, 3.0 * 2.0 ** 41  # a constant operand inside and outside [2^-40, 2^40]
# opcodes (csrc/sr_ops.h)
LOAD_FEAT, UNARY0, UNARY_INF0, LOAD_PARAM, PBIN_DIV, PAIR_MUL, PAIR_DIV, BIN_MUL, BIN_DIV = 0, 4, 40, 184, 192, 268, 274, 92, 98
U_ID = dict(neg=1, square=2, cube=3, exp=4, cos=5, sin=6, log=8, sqrt=12, abs=13)


# ------------------------------------------------------------------------------------------- the datasets
def _logu(rng, n, lo, hi):
    """n Float32 magnitudes, log-uniform over [2^lo, 2^hi]."""
    return np.exp2(rng.uniform(lo, hi, n)).astype(np.float32)


def _signed(rng, v):
    return (v * rng.choice(np.float32([-1, 1]), len(v))).astype(np.float32)


def _fill(edges, *parts):
    """N rows: the edges first, then the parts; what is left over is dropped."""
    v = np.concatenate([np.asarray(edges, dtype=np.float32)] + [np.asarray(p, dtype=np.float32) for p in parts])
    assert len(v) >= N, len(v)
    return v[:N].copy()


def _hard_quotients():
    """256 Float32 pairs (a, b), b = 1 + k ulp for the odd k <= 255, whose exact quotient lies within 2^-20 ulp
    of a rounding midpoint.  With B = 2^23 + k and an odd Q in [2^24, 2^25), the midpoint Q 2^-24 times b is
    B Q 2^-47; a = A 2^-23 with B Q = A 2^24 + r gives a / b = (Q - r / B) 2^-24: |r| / (2 B) ulp from the
    midpoint.  B is odd, so Q = r B^-1 mod 2^24 exists for r = +-1: 2^-24 ulp."""
    a, b = [], []
    for k in range(1, 256, 2):
        B = (1 << 23) + k
        for r in (1, -1):
            Q = (r * pow(B, -1, 1 << 24)) % (1 << 24) + (1 << 24)
            A, rem = divmod(B * Q - r, 1 << 24)
            assert rem == 0 and Q % 2 == 1
            if A >= 1 << 24:  # the dividend in [2, 4): its last bit must be 0
                if A % 2:
                    continue
            a.append(A * 2.0 ** -23)
            b.append(B * 2.0 ** -23)
    a, b = np.array(a), np.array(b)
    assert len(a) >= 200 and np.all(a.astype(np.float32) == a) and np.all(b.astype(np.float32) == b)
    # (the CPU, in Float64: the quotient's fraction of a Float32 ulp is 1/2 to within 2^-20)
    q = a / b * 2.0 ** 23
    assert np.all(np.abs(np.abs(q - np.floor(q)) - 0.5) <= 2.0 ** -20)
    return a.astype(np.float32), b.astype(np.float32)


def _fn(op):
    """The operator of a dataset: "exp_top" and "log_top" are exp and log."""
    return op[:-4] if op.endswith("_top") else op


def _operands(op):
    """(x1, x2) of dataset A as Float32 arrays (Float64 runs the same values)."""
    rng = np.random.default_rng(sum(map(ord, _fn(op))) + 4097)
    one = np.float32(1)
    x2 = _signed(rng, _logu(rng, N, -20, 20))
    if op in ("exp", "exp_top"):
        e = [-88.0, np.nextafter(np.float32(-88), one), 72.0, 0.0, -0.0, 2.0 ** -126, -(2.0 ** -126), 1e-7, -1e-7,
             2.0 ** -24, -(2.0 ** -24), 2.0 ** -12, -(2.0 ** -12), 0.5, -0.5, 1.0, -1.0]
        near0 = _signed(rng, _logu(rng, 400, -40, -1))
        lin = rng.uniform(-88, 72, 1800).astype(np.float32)
        wide = _signed(rng, _logu(rng, 2000, -126, np.log2(88)))
        wide = np.where(wide > 72, -wide, wide)  # (e^x below the deferred checks' bound: module docstring)
        x1 = _fill(e, near0, lin, wide)
        if op == "exp_top":
            x1[2] = 88.0
        assert np.abs(x1).max() == 88 and (x1.max() == 88 if op == "exp_top" else x1.max() == 72)
    elif op in ("log", "log_top"):
        e = [2.0 ** -126, np.nextafter(np.float32(2.0 ** -126), one), 2.0 ** 100, 1.0, np.nextafter(one, np.float32(0)),
             np.nextafter(one, np.float32(2)), 2.0, 0.5, np.e, 10.0]
        d = _logu(rng, 600, -23, -10)
        x1 = _fill(e, one + d[:300], one - d[300:], _logu(rng, 3600, -126, 100))
        if op == "log_top":  # (every other row at most 2^60: their sum stays below half an ulp of floatmax in Float64)
            x1 = np.where(x1 > 2.0 ** 60, x1 * np.float32(2.0 ** -40), x1).astype(np.float32)
            x1[2] = np.finfo(np.float32).max
            assert float(np.sum(x1.astype(np.float64))) == float(np.finfo(np.float32).max)
        assert x1.min() == np.float32(2.0 ** -126) and x1.max() == (np.finfo(np.float32).max if op == "log_top" else np.float32(2.0 ** 100))
    elif op in ("cos", "sin"):
        top = np.nextafter(np.float32(2.0 ** 20), np.float32(0))
        kpi = (np.arange(1, 65) * (np.pi / 2)).astype(np.float32)
        e = [top, -top, 0.0, -0.0, 2.0 ** -126, -(2.0 ** -126)]
        x1 = _fill(e, kpi, -kpi, rng.uniform(-100, 100, 1500).astype(np.float32),
                   _signed(rng, _logu(rng, 2600, -126, 20)))
        assert np.abs(x1).max() == top
    elif op == "sqrt":
        x1 = _fill([0.0, -0.0, 2.0 ** -149, 2.0 ** -126, 2.0 ** 100, 1.0, 2.0, 3.0, 4.0], _logu(rng, N, -140, 100))
    elif op == "square":
        x1 = _fill([0.0, -0.0, 2.0 ** 50, -(2.0 ** 50), 2.0 ** -75, 3.0], _signed(rng, _logu(rng, N, -80, 50)))
    elif op == "cube":
        x1 = _fill([0.0, -0.0, 2.0 ** 33, -(2.0 ** 33), 2.0 ** -50, 3.0], _signed(rng, _logu(rng, N, -55, 33)))
    elif op in ("neg", "abs"):
        x1 = _fill([0.0, -0.0, 2.0 ** -149, -(2.0 ** -149), 2.0 ** 100, -(2.0 ** 100)], _signed(rng, _logu(rng, N, -149, 100)))
    elif op in ("+", "-", "*"):
        x1 = _signed(rng, _logu(rng, N, -60, 50))
        x2 = _signed(rng, _logu(rng, N, -60, 50))
        x2[:512] = np.nextafter(x1[:512], np.float32(0))  # cancellation in -, and in + after the sign flip
        x2[256:512] *= np.float32(-1)
    else:
        assert op == "/"
        ha, hb = _hard_quotients()
        nh = len(ha)
        hi, lo = np.float32(2.0 ** 40), np.float32(2.0 ** -40)
        x1 = _signed(rng, _logu(rng, N, -40, 40))
        x2 = _signed(rng, _logu(rng, N, -40, 40))
        x1[:4], x2[:4] = [hi, hi, lo, -lo], [hi, -lo, hi, lo]
        # the hard pairs: as they are, then scaled by powers of two inside the range, signs mixed
        ea, eb = rng.integers(-39, 39, nh), rng.integers(-39, 39, nh)
        x1[4:4 + nh], x2[4:4 + nh] = ha, hb
        x1[4 + nh:4 + 2 * nh] = _signed(rng, np.ldexp(ha, ea).astype(np.float32))
        x2[4 + nh:4 + 2 * nh] = _signed(rng, np.ldexp(hb, eb).astype(np.float32))
        assert 4 + 2 * nh < 1024 and np.abs(x1).max() == hi and np.abs(x1).min() == lo
        assert np.abs(x2).max() == hi and np.abs(x2).min() == lo
    return x1.astype(np.float32), x2.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _ulp_fixture():
    with open(os.path.join(HERE, "golden", "libm_ulp.json")) as f:
        return json.load(f)


def _in_fast_range(fn, x):
    if fn == "exp":
        return np.abs(x) <= 72
    if fn == "log":
        return (x >= 2.0 ** -126) & (x <= 2.0 ** 100)
    return np.abs(x) < 2.0 ** 20


@functools.lru_cache(maxsize=None)
def _dataset(op, dtype_name):
    """{A, B}: X [3, N] in T, and for Float64 transcendentals the libm_ulp.json entries that fill the rows before
    the last (rows `fix_rows`): those of the fixture inside the fast range, with a modest result."""
    T = DTYPES[dtype_name]
    x1, x2 = _operands(op)
    XA = np.stack([x1, x2, np.ones(N, dtype=np.float32)]).astype(T)
    fn = _fn(op)
    fix, fix_rows = [], np.zeros(0, dtype=np.int64)
    if T == np.float64 and fn in ("exp", "log", "cos", "sin"):
        pts = [e for e in _ulp_fixture()["float64"][fn] if np.isfinite(e[1]) and _in_fast_range(fn, np.float64(e[0]))]
        rows = SHARED[SHARED >= 1024][:-1]  # (after the edges and the hard neighbourhoods; the ragged row stays)
        assert len(pts) >= 256, (fn, len(pts))
        fix = [pts[k % len(pts)] for k in range(len(rows))]
        fix_rows = rows
        XA[0, rows] = [e[0] for e in fix]
    XB = XA.copy()
    out = OUTLIER.get("/" if op == "/" else fn)
    if out is not None:
        XB[0, OUT_AT] = T(out)
    return dict(A=XA, B=XB, fix=fix, fix_rows=fix_rows, has_b=out is not None)


def _expr(op, a="x1", b="x2"):
    return f"{a} {op} {b}" if op in BINARY else f"{_fn(op)}({a})"


def _numpy(op, X, T):
    """The operator in T by numpy (the exact class), or None."""
    a, b = X[0].astype(T), X[1].astype(T)
    with np.errstate(all="ignore"):
        if op in BINARY:
            return {"+": a + b, "-": a - b, "*": a * b, "/": a / b}[op].astype(T)
        return {"sqrt": lambda: np.sqrt(a), "square": lambda: a * a, "cube": lambda: (a * a) * a, "neg": lambda: -a,
                "abs": lambda: np.abs(a)}.get(op, lambda: None)()


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint32 if v.dtype == np.float32 else np.uint64)


@functools.lru_cache(maxsize=None)
def _pred(op, dtype_name, which):
    """PRED's output of `op(x1[, x2])` on dataset A or B: computed once, read by every test."""
    T = DTYPES[dtype_name]
    opts = Options(**OPTS)
    ds = Dataset(_dataset(op, dtype_name)[which])
    try:
        out, comp = eval_tree_array_batch(flatten_trees([parse_expression(_expr(op), opts)], T), ds, opts)
    finally:
        ds.free_device()
    assert comp[0], (op, dtype_name, which)
    out = np.array(out[0], dtype=T)
    out.setflags(write=False)
    return out


ALL_OPS = UNARY + ("exp_top", "log_top") + tuple(BINARY)


# ------------------------------------------------------------------------------------------- check 1
@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("op", ALL_OPS)
def test_pred_values(op, dtype_name):
    T = DTYPES[dtype_name]
    d = _dataset(op, dtype_name)
    fn = _fn(op)
    preds = {}
    for which in ("A", "B") if d["has_b"] else ("A",):
        X = d[which]
        out = preds[which] = _pred(op, dtype_name, which)
        what = (op, dtype_name, which)
        want = _numpy(op, X, T)
        if want is not None:  # the exact class
            bad = np.nonzero(_bits(out) != _bits(want))[0]
            assert len(bad) == 0, (what, len(bad), X[:2, bad[:4]], out[bad[:4]], want[bad[:4]])
            if op == "abs":
                assert not np.signbit(out).any(), what
            continue
        with np.errstate(all="ignore"):
            ref = getattr(np, fn)(X[0].astype(np.float64))
        entries = [[float(x), float(r), 0.0] for x, r in zip(X[0], ref)]
        if T == np.float32:
            err = ulp_errors(T, out, entries)
            print(f"{what}: max ulp error {err.max():.4f} at x = {X[0, int(err.argmax())]!r}")
            if fn == "exp":
                assert err.max() <= 1.0, (what, float(err.max()), X[0, int(err.argmax())])
            else:
                host = host_unary(T, fn, X[0])
                bad = np.nonzero(_bits(out) != _bits(host))[0]
                assert len(bad) == 0, (what, len(bad), X[0, bad[:4]], out[bad[:4]], host[bad[:4]])
                assert err.max() <= F32_BAR[fn], (what, float(err.max()), X[0, int(err.argmax())])
        else:  # the fixture's points at its 1 ulp; the other rows by the identities (fast == slow, check 2)
            rows = d["fix_rows"]
            err = ulp_errors(T, out[rows], d["fix"])
            print(f"{what}: {len(rows)} fixture rows, max ulp error {err.max():.4f}")
            assert err.max() <= 1.0, (what, float(err.max()), d["fix"][int(err.argmax())])
    if d["has_b"]:  # fast == slow
        a, b = preds["A"][SHARED], preds["B"][SHARED]
        bad = np.nonzero(_bits(a) != _bits(b))[0]
        assert len(bad) == 0, (op, dtype_name, len(bad), d["A"][:2, SHARED[bad[:4]]], a[bad[:4]], b[bad[:4]])
        assert np.all(np.isfinite(preds["B"][OUT_AT]))


# ------------------------------------------------------------------------------------------- check 2
def _deep(v):
    """v * x3^15 as a balanced product of 16 leaves (x3 = 1: the value and the sign of zero of v): more than two
    operand-stack slots, so the tree runs on the LDS-stack kernels, never on the register-stack ones."""
    terms = [v] + ["x3"] * 15
    while len(terms) > 1:
        terms = [f"({a} * {b})" for a, b in zip(terms[::2], terms[1::2])]
    return terms[0]


def _plain_groups(op):
    """[(expression whose PRED output is y, [trees with that value])] of one operator, plain family."""
    if op != "/":
        a = _expr(op)
        wrap = lambda inner: _expr(op, inner)  # noqa: E731
        return [(a, [a, wrap("x1 * x3"), wrap("((x1 * x3) * x3) * 1.0"), wrap(_deep("x1"))])]
    d1, d2 = _deep("x1"), _deep("x2")
    return [
        ("x1 / x2", ["x1 / x2", "(x1 * x3) / x2", "x1 / (x2 * x3)", "(x1 * x3) / (x2 * x3)",
                     "(x1 * x3) / ((x2 * x3) * (x3 * x3))", f"{d1} / {d2}"]),
    ] + [(f"x1 / {c}", [f"x1 / {c}", f"(x1 * x3) / {c}", f"((x1 * x3) * x3) / {c}", f"{d1} / {c}"]) for c in (C_IN, C_OUT)] \
      + [(f"{c} / x2", [f"{c} / x2", f"{c} / (x2 * x3)", f"{c} / ((x2 * x3) * x3)", f"{c} / {d2}"]) for c in (C_IN, C_OUT)]


def _param_groups(op):
    """The parametric family: x2 becomes p1 (leaf x4 before to_parametric) with one class.  p1 = 1.0 for a unary
    operator (`x1 * p1` is x1), 3.0 for /."""
    if op != "/":
        a = _expr(op)
        return 1.0, [(a, [a, _expr(op, "x1 * x4"), _expr(op, "((x1 * x3) * x3) * 1.0"), _expr(op, _deep("x1"))])]
    d = _deep("x1")
    return C_IN, [("x1 / x4", ["x1 / x4", "(x1 * x3) / x4", "(x1 * x3) / (x4 * x3)", f"{d} / x4"]),
                  ("x4 / x1", ["x4 / x1", "x4 / (x1 * x3)", "(x4 * x3) / (x1 * x3)", "(x4 * x3) / ((x1 * x3) * (x3 * x3))",
                               f"x4 / {d}"])]


def _batch(exprs, T, p=None):
    opts = Options(**OPTS)
    tb = flatten_trees([parse_expression(e, opts) for e in exprs], T)
    return tb if p is None else to_parametric(tb, 3, np.array([[p]], dtype=T))


def _depth(tb, T):
    """Operand-stack slots the batch's programs need (register stack: at most 2)."""
    return compile_info(Options(**OPTS), tb, N, 3, T)[3]


def _ops_of(tb, T):
    """Per tree, its LOSS program as [(opcode, POST unary, PBC)]."""
    code, offs, bad, _ = compile_info(Options(**OPTS), tb, N, 3, T)
    assert not bad.any()
    return [[(int(o) & 0x1FF, (int(o) >> 16) & 0x3F, (int(o) >> 24) & 7) for o in code["op"][offs[k]:offs[k + 1]]]
            for k in range(tb.n_trees)]


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_the_trees_compile_to_the_forms_they_are_there_for(dtype_name):
    """CPU: every operand form check 2 is there for is emitted by one of its trees."""
    T = DTYPES[dtype_name]
    for op in UNARY:
        u = U_ID[op]
        leaf, pair, own, deep = _ops_of(_batch(_plain_groups(op)[0][1], T), T)
        assert deep[-1][0] & 0x1FF in (BIN_MUL, BIN_MUL + 1) and deep[-1][1] == u, (op, deep)  # POST on a stack operand
        assert leaf == [(LOAD_FEAT, u, 0)], (op, leaf)  # (LOAD_DERIVED in a call that chooses columns)
        assert pair == [(PAIR_MUL, u, 0)], (op, pair)   # POST on a pair
        assert own[-1][0] in (UNARY0 + u, UNARY_INF0 + u) and own[-1][1] == 0, (op, own)  # its own opcode
        _, par, _, _ = _ops_of(_batch(_param_groups(op)[1][0][1], T, 1.0), T)
        assert par == [(LOAD_PARAM, 0, 0), (BIN_MUL + 3, u, 0)], (op, par)  # POST on (p1 * x1)
    seen = {o for g in _plain_groups("/") for prog in _ops_of(_batch(g[1], T), T) for o in prog}
    for name, want in [("PAIR FF", (PAIR_DIV, 0, 0)), ("PAIR FC", (PAIR_DIV + 1, 0, 0)), ("PAIR CF", (PAIR_DIV + 2, 0, 0)),
                       ("SL", (BIN_DIV, 0, 0)), ("SR", (BIN_DIV + 1, 0, 0)), ("FL", (BIN_DIV + 2, 0, 0)),
                       ("FR", (BIN_DIV + 3, 0, 0)), ("CL", (BIN_DIV + 4, 0, 0)), ("CR", (BIN_DIV + 5, 0, 0)),
                       ("PBC tos / c", (BIN_MUL + 3, 0, 5)), ("PBC c / tos", (BIN_MUL + 3, 0, 6))]:
        assert want in seen, (name, sorted(seen))
    p, groups = _param_groups("/")
    seen = {o[0] for g in groups for prog in _ops_of(_batch(g[1], T, p), T) for o in prog}
    assert {PBIN_DIV, PBIN_DIV + 1, BIN_DIV, BIN_DIV + 1, BIN_DIV + 2, BIN_DIV + 3} <= seen, sorted(seen)
    # every group: its last tree needs the LDS stack, the others fit the register stack
    for p, groups in [(None, _plain_groups(op)) for op in UNARY + ("/",)] + [_param_groups(op) for op in UNARY + ("/",)]:
        for g in groups:
            tb = _batch(g[1], T, p)
            assert _depth(tb.take(list(range(tb.n_trees - 1))), T) <= 2 < _depth(tb.take([tb.n_trees - 1]), T), g[1]


def _view():
    """A permutation of the rows that keeps every aligned 128-row group together (A stays fast, B slow): the 32
    full groups in another order, each one's rows shuffled; the ragged row stays last."""
    rng = np.random.default_rng(128)
    idx = np.concatenate([g * GROUP + rng.permutation(GROUP) for g in rng.permutation((N - 1) // GROUP)] + [[N - 1]])
    assert np.array_equal(np.sort(idx), np.arange(N))
    return idx.astype(np.int64)


def _y_of(group, T, X, cls, p):
    """PRED's output of the group's first tree on this dataset (parametric: through the parametric entry)."""
    opts = Options(**OPTS)
    ds = Dataset(X) if p is None else Dataset(X, extra={"class": cls}, n_classes=1)
    try:
        out, comp = eval_tree_array_batch(_batch([group[0]], T, p), ds, opts)
    finally:
        ds.free_device()
    assert comp[0], group[0]
    return np.array(out[0], dtype=T)


@pytest.mark.gpu
@pytest.mark.parametrize("view", ["full", "rows"])
@pytest.mark.parametrize("family", ["plain", "parametric"])
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("op", UNARY + ("exp_top", "/"))
def test_every_build_reproduces_pred(op, dtype_name, family, view):
    T = DTYPES[dtype_name]
    d = _dataset(op, dtype_name)
    cls = np.ones(N, dtype=np.int32)
    p, groups = _param_groups(op if op != "exp_top" else "exp") if family == "parametric" else (None, _plain_groups(op))
    idx = _view()
    ctx = sr_amd.get_context()
    cases = _knob_cases(family, T, True, view == "full")
    n_calls = 0
    try:
        for which in ("A", "B") if d["has_b"] else ("A",):
            X = d[which]
            for group in groups:
                y = _y_of(group, T, X, cls, p)
                if p is None and group[0] == _expr(op):  # the value check 1 looked at
                    assert np.array_equal(_bits(y), _bits(_pred(op, dtype_name, which)))
                elif op == "/":  # the other quotients: IEEE, as numpy's
                    c = {"x1": X[0], "x2": X[1], "x4": np.full(N, T(C_IN))}
                    a, b = (c[s] if s in c else np.full(N, T(float(s))) for s in group[0].split(" / "))
                    assert np.array_equal(_bits(y), _bits((a / b).astype(T))), (group[0], which)
                else:  # a unary operator's parametric PRED: the plain one's bits
                    assert np.array_equal(_bits(y), _bits(_pred(op, dtype_name, which)))
                tb = _batch(group[1], T, p)
                ds = Dataset(X, y) if p is None else Dataset(X, y, extra={"class": cls}, n_classes=1)
                target = ds if view == "full" else batch(ds, idx)
                try:
                    for spec in LOSSES:
                        opts = Options(elementwise_loss=spec, **OPTS)
                        for rpl, vstk, mrb in cases:
                            ctx.set_tuning("rows_per_lane", rpl)
                            ctx.set_tuning("vstk_rows", vstk)
                            ctx.set_tuning("max_row_blocks", mrb)
                            loss, comp = eval_loss_batch(tb, target, opts)
                            what = (op, dtype_name, family, view, which, spec, f"rows_per_lane={rpl} vstk_rows={vstk} "
                                    f"max_row_blocks={mrb}", group[1])
                            assert comp.all(), (what, comp)
                            assert np.all(loss == 0.0), (what, loss)
                            # the loss launch's own result, not the exact-sum pass's (module docstring: exp_top)
                            # (Float64's bound is far above e^88)
                            assert (ctx.last_exact_trees() > 0) == (op == "exp_top" and T == np.float32), (what, ctx.last_exact_trees())
                            n_calls += 1
                finally:
                    ds.free_device()
    finally:
        for name, value in DEFAULTS.items():
            ctx.set_tuning(name, value)
    assert n_calls == (2 if d["has_b"] else 1) * len(groups) * len(LOSSES) * len(cases)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_one_ulp_in_one_row_shows(dtype_name):
    """The control of check 2: y moved by one ulp in a single row, and the L1 loss is exactly ulp / 4097 in T."""
    T = DTYPES[dtype_name]
    X = _dataset("/", dtype_name)["A"]
    y = np.array(_pred("/", dtype_name, "A"))
    row = 1000
    moved = np.nextafter(y[row], T(np.inf))
    ulp = T(moved - y[row])
    assert ulp > 0 and np.float64(ulp) == np.float64(moved) - np.float64(y[row])
    y[row] = moved
    want = T(ulp / T(N))
    assert want == T(np.float64(ulp) / N) and want > 0  # (the same number however the mean is rounded)
    opts = Options(elementwise_loss="L1DistLoss()", **OPTS)
    ds = Dataset(X, y)
    try:
        loss, comp = eval_loss_batch(_batch(["x1 / x2", "(x1 * x3) / (x2 * x3)"], T), ds, opts)
    finally:
        ds.free_device()
    assert comp.all() and np.array_equal(_bits(loss), _bits(np.full(2, want, dtype=T))), (loss, want)


# ------------------------------------------------------------------------- the candidate build's own shape
@pytest.mark.gpu
@pytest.mark.parametrize("op", UNARY + ("/",))
def test_candidate_build_reproduces_pred(op):
    """The C2 kernel (SR_TIER_CAND: Float32, register stack, 16 rows per lane) at test_gpu_loss_compact.py's
    smallest shape: 2^18 rows (a dataset's first 4,096 rows tiled 64 times), one chunk of 520 register-stack trees
    (the operator's check 2 trees repeated) and 8 copies of the deep one beside them (the LDS-stack kernel at 16
    rows per lane, in the chunk's second launch), y from PRED.  Every loss exactly 0.  Three calls:
      A, full view   the listed candidate launch ran (sr_last_phase_ms out[16]) at 16 rows per lane;
      B, full view   the same with every wave on the slow path, the column kernel's waves included;
      A, row view    a permutation of the rows: the gathered builds.
    In each, for the operators sr_launch_derived computes, `u(x1)` came from a derived column."""
    T = np.float32
    opts = Options(**OPTS)
    group = _plain_groups(op)[0]
    shallow, deep = group[1][:-1], group[1][-1]
    tb = _batch([shallow[k % len(shallow)] for k in range(520)] + [deep] * 8, T)
    ctx = sr_amd.get_context()
    d = _dataset(op, "float32")
    idx = np.random.default_rng(18).permutation(1 << 18).astype(np.int64)
    for which, view in [("A", "full")] + ([("B", "full")] if d["has_b"] else []) + [("A", "rows")]:
        X = np.ascontiguousarray(np.tile(d[which][:, :N - 1], (1, 64)))
        assert X.shape == (3, 1 << 18)
        ds = Dataset(X)
        try:
            out, comp = eval_tree_array_batch(_batch([group[0]], T), ds, opts)
            assert comp[0]
            y = np.array(out[0], dtype=T)
            assert np.array_equal(_bits(y[:N - 1]), _bits(_pred(op, "float32", which)[:N - 1]))
        finally:
            ds.free_device()
        ds = Dataset(X, y)
        try:
            loss, comp = eval_loss_batch(tb, ds if view == "full" else batch(ds, idx), opts)
            info = (ctypes.c_double * 19)()
            _lib.check(_lib.lib.sr_last_phase_ms(ctx.handle, info, 19))
            what = dict(data=which, view=view, listed=int(info[16]), live=int(info[17]), rows_per_lane=ctx.last_rows_per_lane(),
                        path=ctx.last_ref_fold()["path"], derived=ctx.last_derived_columns(), exact=ctx.last_exact_trees())
            print(op, what)
        finally:
            ds.free_device()
        assert comp.all() and np.all(loss == 0.0), (op, what, np.nonzero(loss != 0.0)[0][:8], loss[loss != 0.0][:8])
        assert what["exact"] == 0, what
        if view == "full":
            assert what["listed"] >= 1 and what["live"] == 520 and what["rows_per_lane"] == 16 and what["path"] == 2, what
        if op in ("exp", "cos", "sin", "log", "sqrt"):
            assert what["derived"] == 1, what
