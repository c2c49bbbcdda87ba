"""CPU: the operator-value fixture (tests/golden/op_values.json: 33 unary and 16 binary operators, mpmath at 60
digits, and the special cases of the reference's definitions with their citations) against the three host
restatements of the catalog, none of which a value-level test looked at for 18 of the operators:

  * the oracle's operators (oracle/de_eval.c through Oracle.eval_tree_array), one row per point;
  * sr_host_unary (csrc/sr_ops.h's sr_unary on the host: what the constant folder calls);
  * the constant folder: the trees op(c) and op(c1, c2) through sr_compile_info — its static verdict (an
    incomplete point is a statically incomplete tree) and the folded value (the program is one LOAD_CONST).

Bars.  The exact class (neg square cube abs sign relu inv round floor ceil sqrt; + - * / max min mod cond, the
comparisons and the logical operators) is bit-equal to the fixture, sign of zero included.  The rest are the host
libm's functions, which are not this project's code: their `values` are held to HOST_BAR = 16 ulp of T, far above any
libm's error (glibc documents single digits for every one of them) and far below what a wrong branch, a wrong
function or a swapped argument gives, which is what these tests are for.  Every special point with a value is an
exact bit pattern, sign of zero included, for every operator (exp(0) = 1, log2(8) = 3, gamma(5) = 24, ...): Julia
returns exactly these.
"""
import ctypes

import numpy as np
import pytest

from bytecode_vm import LOAD_CONST, compile_info
from op_values_util import BINARY, DTYPES, UNARY, C, X, bi, bits, entry, options, rows, special_mask, ulp_error, un
from oracle import Oracle
from sr_amd import _lib, flatten_trees

HOST_BAR = 16.0
OPS = [(1, n) for n in UNARY] + [(2, n) for n in BINARY]
IDS = [f"{'u' if d == 1 else 'b'}:{n}" for d, n in OPS]


def _meets(T, exact, got, hi, lo, spec, what):
    """The exact class and every special point: the fixture's bits.  The other operators' values: HOST_BAR, and the
    sign of a zero."""
    got = np.asarray(got, dtype=T)
    bitwise = spec | exact
    want = np.asarray(hi, dtype=T)
    bad = np.nonzero(bitwise & (bits(got) != bits(want)))[0]
    assert len(bad) == 0, (what, bad[:4], got[bad[:4]], want[bad[:4]])
    err = ulp_error(T, got, hi, lo)
    assert np.all(err[~bitwise] <= HOST_BAR), (what, float(np.max(err[~bitwise])))
    z = np.asarray(hi) == 0
    assert np.array_equal(np.signbit(got[z]), np.signbit(np.asarray(hi)[z])), what


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("degree,name", OPS, ids=IDS)
def test_oracle_meets_the_fixture(degree, name, dtype_name):
    T = DTYPES[dtype_name]
    args, hi, lo, inc = rows(dtype_name, name, degree)
    orc = Oracle.from_options(options())
    tree = un(name, X(1)) if degree == 1 else bi(name, X(1), X(2))
    tb = flatten_trees([tree], T)
    got, comp = np.empty(len(args), dtype=T), np.empty(len(args), dtype=bool)
    for k, a in enumerate(args):
        out, comp[k] = orc.eval_tree_array(tb, 0, np.ascontiguousarray(a.reshape(degree, 1)))
        got[k] = out[0]
    assert np.array_equal(comp, ~inc), (name, dtype_name, args[comp == inc])
    ok, spec = ~inc, special_mask(dtype_name, name, degree)
    _meets(T, entry(dtype_name, name, degree)["exact"], got[ok], hi[ok], lo[ok], spec[ok], (name, dtype_name, args[ok]))


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("name", UNARY)
def test_host_unary_meets_the_fixture(name, dtype_name):
    T = DTYPES[dtype_name]
    args, hi, lo, inc = rows(dtype_name, name, 1)
    x = np.ascontiguousarray(args[:, 0])
    got = np.empty_like(x)
    with np.errstate(all="ignore"):
        _lib.check(_lib.lib.sr_host_unary(_lib.SR_DTYPE_F32 if T == np.float32 else _lib.SR_DTYPE_F64, name.encode(), x.size,
                                          x.ctypes.data_as(ctypes.c_void_p), got.ctypes.data_as(ctypes.c_void_p)))
    assert np.array_equal(~np.isfinite(got), inc), (name, dtype_name, x[np.isfinite(got) == inc])
    ok = ~inc
    _meets(T, entry(dtype_name, name, 1)["exact"], got[ok], hi[ok], lo[ok], special_mask(dtype_name, name, 1)[ok], (name, dtype_name, x[ok]))


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("degree,name", OPS, ids=IDS)
def test_constant_folder_meets_the_fixture(degree, name, dtype_name):
    """op(c), op(c1, c2): a non-finite leaf constant is itself an invalid subtree, which is the
    expected verdict of every point with a NaN or Inf operand but the comparisons' and logical operators' NaN rows
    (value 0.0 or 1.0 by the definition, from an evaluation that never validates a feature leaf): those rows are
    left to the oracle and the device."""
    T = DTYPES[dtype_name]
    args, hi, lo, inc = rows(dtype_name, name, degree)
    fin = np.isfinite(args).all(axis=1) | inc
    args, hi, lo, inc, spec = args[fin], hi[fin], lo[fin], inc[fin], special_mask(dtype_name, name, degree)[fin]
    trees = [un(name, C(a[0])) if degree == 1 else bi(name, C(a[0]), C(a[1])) for a in args]
    tb = flatten_trees(trees, T)
    code, offs, bad, _ = compile_info(options(), tb, 1, 2, T)
    assert np.array_equal(bad, inc), (name, dtype_name, args[bad != inc])
    got = np.empty(len(args), dtype=T)
    for k in np.nonzero(~inc)[0]:
        assert offs[k + 1] - offs[k] == 1 and int(code["op"][offs[k]]) == LOAD_CONST, (name, args[k])
        got[k] = code["val"][offs[k]]
    ok = ~inc
    _meets(T, entry(dtype_name, name, degree)["exact"], got[ok], hi[ok], lo[ok], spec[ok], (name, dtype_name, args[ok]))


def test_the_fixture_holds_the_catalog():
    """33 + 16 operators per dtype, at most 64 values each, every special row cited."""
    from op_values_util import fixture

    for dtype_name in DTYPES:
        fx = fixture()[dtype_name]
        assert sorted(fx["unary"]) == sorted(UNARY) and sorted(fx["binary"]) == sorted(BINARY)
        for degree, group in ((1, "unary"), (2, "binary")):
            for name, e in fx[group].items():
                assert 8 <= len(e["values"]) <= 64, (name, len(e["values"]))
                assert all(len(v) == degree + 2 for v in e["values"])
                assert e["special"] and all(len(s) == degree + 2 and s[-1] for s in e["special"]), name
