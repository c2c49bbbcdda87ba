"""GPU: every operator of the catalog (csrc/sr_ops.h: 33 unary, 16 binary) per value, in PRED mode, against
tests/golden/op_values.json (mpmath at 60 digits; the special cases of the reference's definitions).

Per operator and dtype, over one uploaded dataset (x1, x2 the operands, x3 = 1, x4 = -x1):
  * the `values` rows in one call (rows whose value or operand could overflow the checked arrays' sum: alone);
  * every `special` point alone, through a row view of one index: an `incomplete` point must come back incomplete
    (only the flag is asserted: an incomplete tree's output array is unspecified), the others complete with the
    expected bit pattern, sign of zero included, for every operator (exp(0) = 1, log2(8) = 3, gamma(5) = 24: Julia
    returns these exactly); then the points with a value together in one call;
  * every compiled form of the operator, which must agree with the first bit for bit and flag for flag: the
    operator's own opcode, the POST-fused form, the two INF-fused forms (SR_OP_UNARY_INF0 / POST_INF: a non-finite
    input must make the tree incomplete); for a binary operator PAIR FF / FC / CF, the S, F and C variants on both
    sides and the parameter-operand opcodes (PBIN) of the parametric build.  The forms are asserted from the compiled
    programs (test_the_forms_compile_as_named, no GPU);
  * the constant folder: the constant tree op(c) / op(c1, c2) has the device's completeness at the same point, and
    its bits for the exact class.
A row with a NaN operand and a finite result (the comparisons and logical operators) is complete or not by the
evaluation order of the form around it (a computed operand is validated, a feature leaf is not): there every form's
flag is the oracle's for that same tree (the oracle's operators are pinned by test_op_values_host.py).

Bars.  The exact class (neg square cube abs sign relu inv round floor ceil sqrt; + - * / max min mod cond, the
comparisons and the logical operators) is bit-equal to numpy in T (the fixture's `hi`; mod restated as Base's).  The
others are OCML's functions (Float32 exp / log / cos / sin: the library's own, csrc/sr_libm.h), with no project bar:
BARS holds, per operator and dtype, max |device - (hi + lo)| in ulps of T measured on the MI355X over the fixture's
points, doubled and rounded up to a whole ulp, at least 1 (the margin covers libm differences between ROCm releases;
a wrong branch or a wrong function is off by thousands).  The measured table is profiles/op_values_ulp.txt.
"""
import numpy as np
import pytest

from bytecode_vm import compile_info
from op_values_util import (BINARY, DTYPES, UNARY, C, bi, binary_const_forms, binary_forms, binary_param_forms, bits, entry,
                            options, rows, ulp_error, un, unary_forms)
from oracle import Oracle
from parametric_util import to_parametric
from sr_amd import Dataset, batch, eval_tree_array_batch, flatten_trees

OPS = [(1, n) for n in UNARY] + [(2, n) for n in BINARY]
IDS = [f"{'u' if d == 1 else 'b'}:{n}" for d, n in OPS]
COMMUTING = ("+", "*")  # the compiler canonicalises them to their R / FC variants

# measured max error in ulps of T (float32, float64) -> the bar: ceil(2 x measured), at least 1
MEASURED = {  # MI355X (gfx950), ROCm 7.2.0: profiles/op_values_ulp.txt
    "exp": (0.5717, 0.6212), "cos": (0.4965, 0.5227), "sin": (0.4872, 0.4639), "tan": (0.7856, 0.4669),
    "log": (0.5, 0.5), "log2": (0.9887, 0.5235), "log10": (1.2223, 0.4324), "log1p": (0.4725, 0.4085),
    "tanh": (0.4656, 0.4345), "sinh": (0.5363, 0.4344), "cosh": (0.4898, 0.4368), "atan": (1.4216, 0.8748),
    "asin": (0.9472, 0.4828), "acos": (0.6622, 0.5172), "acosh": (0.4616, 0.4468), "atanh": (0.3874, 0.4997),
    "asinh": (0.4867, 0.5269), "erf": (0.5081, 0.4831), "erfc": (0.6715, 0.9541), "gamma": (1.4098, 3.3444),
    "exp2": (0.5235, 0.5646), "expm1": (0.6925, 0.4722), "^": (0.76, 0.8536), "atan2": (1.0985, 0.5911),
}
BARS = {name: tuple(max(1.0, float(np.ceil(2 * m))) for m in ms) for name, ms in MEASURED.items()}


def _dataset(dtype_name, name, degree):
    T = DTYPES[dtype_name]
    args, hi, lo, inc = rows(dtype_name, name, degree)
    n = len(args)
    X = np.ones((4, n + 1), dtype=T)
    X[0, :n] = args[:, 0]
    if degree == 2:
        X[1, :n] = args[:, 1]
    X[0, n] = np.inf  # the INF-fused forms' row
    X[3] = -X[0]
    return X, args, hi, lo, inc


def _forms(name, degree, T):
    f = unary_forms(name) if degree == 1 else binary_forms(name)
    return list(f), flatten_trees(list(f.values()), T)


class _Device:
    """PRED over row views of one uploaded dataset."""

    def __init__(self, X, parametric=False):
        self.ds = Dataset(X, extra={"class": np.ones(X.shape[1], dtype=np.int32)}, n_classes=1) if parametric else Dataset(X)

    def __call__(self, tb, idx):
        out, comp = eval_tree_array_batch(tb, batch(self.ds, np.asarray(idx, dtype=np.int64)), options())
        return out, comp

    def close(self):
        self.ds.free_device()


def measure(dtype_name, name, degree):
    """max ulp error of the operator's first form over the fixture's `values` (each row alone: no sum to overflow):
    tools/op_values_ulp.py writes profiles/op_values_ulp.txt from it."""
    T = DTYPES[dtype_name]
    X, args, hi, lo, inc = _dataset(dtype_name, name, degree)
    nv = len(entry(dtype_name, name, degree)["values"])
    _, tb = _forms(name, degree, T)
    dev = _Device(X)
    try:
        got = np.array([dev(tb.take([0]), [k])[0][0, 0] for k in range(nv)], dtype=T)
    finally:
        dev.close()
    return float(ulp_error(T, got, hi[:nv], lo[:nv]).max())


def _check_value(T, bitwise, bar, got, hi, lo, what):
    if bitwise:
        assert bits(np.array([got], dtype=T))[0] == bits(np.array([hi], dtype=T))[0], (what, got, hi)
    else:
        err = float(ulp_error(T, [got], [hi], [lo])[0])
        assert err <= bar, (what, got, hi, err)
        if hi == 0:
            assert np.signbit(got) == np.signbit(hi), (what, got, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("degree,name", OPS, ids=IDS)
def test_device_meets_the_fixture(degree, name, dtype_name):
    T = DTYPES[dtype_name]
    e = entry(dtype_name, name, degree)
    exact = e["exact"]
    bar = None if exact else BARS[name][0 if T == np.float32 else 1]
    X, args, hi, lo, inc = _dataset(dtype_name, name, degree)
    n, nv = len(args), len(e["values"])
    names, tb = _forms(name, degree, T)
    orc = Oracle.from_options(options())
    dev = _Device(X)
    devp = _Device(X, parametric=True) if degree == 2 else None
    own = np.full(n, np.nan, dtype=T)      # the first form's value and flag per point
    own_comp = np.zeros(n, dtype=bool)
    try:
        # the values in one call, but for the rows that could overflow a checked array's sum
        big = float(np.finfo(T).max) / (4 * n)
        small = np.array([k < nv and np.all(np.abs(args[k].astype(np.float64)) <= big) and abs(hi[k]) <= big for k in range(n)])
        idx = np.nonzero(small)[0]
        out, comp = dev(tb, idx)
        assert comp.all(), (name, dtype_name, names, comp)
        for f in range(1, len(names)):
            assert np.array_equal(bits(out[f]), bits(out[0])), (name, dtype_name, names[f], args[idx][bits(out[f]) != bits(out[0])])
        own[idx], own_comp[idx] = out[0], True
        if exact:
            bad = bits(out[0]) != bits(hi[idx].astype(T))
            assert not bad.any(), (name, dtype_name, args[idx][bad], out[0][bad], hi[idx][bad])
        else:
            err = ulp_error(T, out[0], hi[idx], lo[idx])
            print(f"{name} {dtype_name}: {len(idx)} values in one call, max ulp error {err.max():.3f} (bar {bar})")
            assert err.max() <= bar, (name, dtype_name, args[idx][int(err.argmax())], float(err.max()))
            z = hi[idx] == 0
            assert np.array_equal(np.signbit(out[0][z]), np.signbit(hi[idx][z])), (name, dtype_name, args[idx][z], out[0][z])
        # the other points alone
        for k in np.nonzero(~small)[0]:
            what = (name, dtype_name, tuple(args[k]))
            out, comp = dev(tb, [k])
            if np.isfinite(args[k]).all():
                assert np.array_equal(comp, np.full(len(names), not inc[k])), (what, names, comp)
            else:  # a non-finite operand: by the evaluation order of each form, as the oracle restates it
                want = [orc.eval_tree_array(tb, f, np.ascontiguousarray(X[:, k:k + 1]))[1] for f in range(len(names))]
                assert np.array_equal(comp, want), (what, names, comp, want)
                assert inc[k] <= (not comp.any()), (what, comp)
            own_comp[k] = comp[0]
            for f in np.nonzero(comp)[0]:
                _check_value(T, exact or k >= nv, bar, out[f, 0], hi[k], lo[k], what + (names[f],))  # a special point: its bits
                assert bits(out[f])[0] == bits(out[int(np.argmax(comp))])[0], (what, names[f])
            if comp[0]:
                own[k] = out[0, 0]
        # the special points with a value once more, together in one call (those that cannot overflow a sum)
        sp = np.array([k for k in range(nv, n) if not inc[k] and np.all(np.abs(args[k].astype(np.float64)) <= big) and abs(hi[k]) <= big],
                      dtype=np.int64)
        out, comp = dev(tb, sp)
        assert comp.all(), (name, dtype_name, names, comp)
        for f in range(len(names)):
            bad = bits(out[f]) != bits(hi[sp].astype(T))
            assert not bad.any(), (name, dtype_name, names[f], args[sp][bad], out[f][bad], hi[sp][bad])
        if degree == 1:  # the fused forms: a non-finite input makes the tree incomplete
            out, comp = dev(tb, [n])
            assert not comp[names.index("post_inf")] and not comp[names.index("own_inf")], (name, dtype_name, names, comp)
        else:
            # a constant or a parameter as one operand, per point with finite operands
            pform = binary_param_forms(name)
            ptb = flatten_trees(list(pform.values()), T)
            for k in np.nonzero(np.isfinite(args).all(axis=1))[0]:
                x, y = args[k]
                what = (name, dtype_name, (x, y))
                cform = binary_const_forms(name, x, y)
                out, comp = dev(flatten_trees(list(cform.values()), T), [k])
                pout, pcomp = devp(to_parametric(ptb, 4, np.array([[[y]], [[x]]], dtype=T)), [k])
                for f, (o, c) in zip(list(cform) + list(pform), list(zip(out[:, 0], comp)) + list(zip(pout[:, 0], pcomp))):
                    assert c == own_comp[k], (what, f, c, own_comp[k])
                    if c:
                        assert bits(np.array([o], dtype=T))[0] == bits(own[k:k + 1])[0], (what, f, o, own[k])
        # the folder: op(c) / op(c1, c2) at the points with finite operands
        fin = np.nonzero(np.isfinite(args).all(axis=1))[0]
        ctb = flatten_trees([un(name, C(a[0])) if degree == 1 else bi(name, C(a[0]), C(a[1])) for a in args[fin]], T)
        out, comp = dev(ctb, [0])
        assert np.array_equal(comp, own_comp[fin]), (name, dtype_name, args[fin][comp != own_comp[fin]])
        if exact:
            ok = comp
            assert np.array_equal(bits(out[ok, 0]), bits(own[fin][ok])), (name, dtype_name, args[fin][ok], out[ok, 0], own[fin][ok])
    finally:
        dev.close()
        if devp is not None:
            devp.close()


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_the_forms_compile_as_named(dtype_name):
    """CPU: each form's program ends in the opcode it is named for (csrc/sr_ops.h)."""
    T = DTYPES[dtype_name]
    LOAD_FEAT, UNARY0, UNARY_INF0, BINARY0, PBIN0, PAIR0, POST_INF = 0, 4, 40, 80, 186, 256, 1 << 22

    def last(tb, nf=4):
        code, offs, bad, _ = compile_info(options(), tb, 1, nf, T)
        assert not bad.any()
        return [int(code["op"][offs[k + 1] - 1]) for k in range(tb.n_trees)]

    for name in UNARY:
        u = UNARY.index(name) + 1  # SrUnaryOp: the catalog's order
        names, tb = _forms(name, 1, T)
        op = dict(zip(names, last(tb)))
        assert op["leaf"] & 0x1FF == LOAD_FEAT and (op["leaf"] >> 16) & 0x3F == u, (name, op)
        assert op["post_inf"] & 0x1FF == PAIR0 + 6 * 2 and (op["post_inf"] >> 16) & 0x3F == u and op["post_inf"] & POST_INF, (name, op)
        assert op["own"] == UNARY0 + u and op["own_inf"] == UNARY_INF0 + u, (name, op)
    for name in BINARY:
        b = BINARY.index(name)  # SrBinaryOp - 1
        com = name in COMMUTING
        names, tb = _forms(name, 2, T)
        op = dict(zip(names, last(tb)))
        assert op["FF"] == PAIR0 + 6 * b, (name, op)
        assert op["FR"] == BINARY0 + 6 * b + 3 and op["FL"] == BINARY0 + 6 * b + (3 if com else 2), (name, op)
        assert {op["S"], op["S_other"]} == ({BINARY0 + 6 * b + 1} if com else {BINARY0 + 6 * b, BINARY0 + 6 * b + 1}), (name, op)
        cf = binary_const_forms(name, 1.5, 2.5)
        op = dict(zip(cf, last(flatten_trees(list(cf.values()), T))))
        assert op["FC"] == PAIR0 + 6 * b + 1 and op["CF"] == PAIR0 + 6 * b + (1 if com else 2), (name, op)
        assert op["CR"] == BINARY0 + 6 * b + 5 and op["CL"] == BINARY0 + 6 * b + (5 if com else 4), (name, op)
        pf = binary_param_forms(name)
        ptb = to_parametric(flatten_trees(list(pf.values()), T), 4, np.array([[1.5]], dtype=T))
        op = dict(zip(pf, last(ptb)))
        assert op["PR"] == PBIN0 + 2 * b + 1 and op["PL"] == PBIN0 + 2 * b + (1 if com else 0), (name, op)


def test_every_inexact_operator_has_a_measured_bar():
    for dtype_name in DTYPES:
        for degree, name in OPS:
            assert entry(dtype_name, name, degree)["exact"] == (name not in BARS), name
