"""Host-side checks of the per-row derivative calls (no GPU): the C prototypes against the ctypes
ones, argument validation before any device call, the output layout, the fixture, and the gradient programs of
the fixture's trees against their recorded digests (the program format did not move: the per-row kernels run
sr_compile_info_grad's programs as they were).

    python tests/test_diff_tree_array_host.py --write     rewrites tests/golden/diff_tree_array_programs.json
"""
import ctypes
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "diff_tree_array.json")
PROGRAMS = os.path.join(HERE, "golden", "diff_tree_array_programs.json")


def program_digests():
    """{case name: {dtype: {n_ins, depth, sha256 of the instruction bytes}}} of the fixture trees' gradient
    programs (sr_compile_info_grad, 100 rows, 3 features)."""
    from bytecode_vm import compile_info
    from sr_amd import Options, flatten_trees, parse_expression

    with open(FIXTURE) as f:
        g = json.load(f)
    opts = Options(binary_operators=g["binary_operators"], unary_operators=g["unary_operators"])
    out = {}
    for case in g["cases"]:
        out[case["name"]] = {}
        for dtype in (np.float32, np.float64):
            tb = flatten_trees([parse_expression(case["expr"], opts)], dtype)
            code, offs, bad, depth = compile_info(opts, tb, 100, 3, dtype, grad=True)
            n = int(offs[-1])
            assert not bad[0]
            out[case["name"]][np.dtype(dtype).name] = dict(
                n_ins=n, depth=depth, sha256=hashlib.sha256(code[:n].tobytes()).hexdigest())
    return out


def test_gradient_programs_did_not_move():
    with open(PROGRAMS) as f:
        want = json.load(f)
    assert program_digests() == want


def _c_args(name):
    text = open(os.path.join(ROOT, "include", "sr_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype_of(arg):
    if "*" in arg:
        return "ptr"
    return {"int": "c_int", "int64_t": "c_long"}[arg.split()[0]]


@pytest.mark.parametrize("name", ["sr_eval_grad_tree_array", "sr_eval_diff_tree_array"])
def test_header_matches_ctypes(name):
    from sr_amd import _lib

    args = _c_args(name)
    fn = getattr(_lib.lib, name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(args)
    for a, t in zip(args, fn.argtypes):
        kind = _ctype_of(a)
        if kind == "ptr":
            assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (a, t)
        elif kind == "c_int":
            assert t is ctypes.c_int, (a, t)
        else:
            assert t is ctypes.c_int64, (a, t)
    names = [a.replace("*", " ").split()[-1] for a in args]
    head = ["ctx", "ds", "opset_id", "trees", "row_idx", "n_idx"]
    if name == "sr_eval_grad_tree_array":
        assert names == head + ["variable", "out_pred", "out_grad", "out_complete"]
    else:
        assert names == head + ["direction", "out_pred", "out_diff", "out_complete"]
    assert name in _lib.EXPORTED_SYMBOLS


def test_exports():
    import sr_amd

    for n in ("eval_diff_tree_array", "eval_grad_tree_array", "eval_diff_tree_array_batch", "eval_grad_tree_array_batch"):
        assert n in sr_amd.__all__ and callable(getattr(sr_amd, n))


def test_validation_raises_before_any_device_call(monkeypatch):
    import sr_amd
    from sr_amd import Options, ParametricExpression, diff, parse_expression

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(diff, "get_context", no_device)
    monkeypatch.setattr(sr_amd.Dataset, "device_handle", no_device)
    opts = Options(binary_operators=["+", "*"], unary_operators=["cos"])
    X = np.ones((2, 8), dtype=np.float32)
    t = parse_expression("cos(x1) * x2", opts)
    for bad in (0, 3, -1, 1.5):
        with pytest.raises(ValueError):
            sr_amd.eval_diff_tree_array(t, X, opts, bad)
    ds = sr_amd.Dataset(X)
    with pytest.raises(ValueError):
        sr_amd.eval_diff_tree_array_batch([t, t], ds, opts, [1, 3])
    with pytest.raises(ValueError):
        sr_amd.eval_diff_tree_array_batch([t, t], ds, opts, [1])
    pe = ParametricExpression(parse_expression("p1 * x1", opts), np.ones((1, 2)))
    for call in (lambda: sr_amd.eval_grad_tree_array(pe, X, opts), lambda: sr_amd.eval_diff_tree_array(pe, X, opts, 1),
                 lambda: sr_amd.eval_grad_tree_array_batch([t, pe], ds, opts, variable=True),
                 lambda: sr_amd.eval_diff_tree_array_batch([pe], ds, opts, [1])):
        with pytest.raises(NotImplementedError, match="§15"):
            call()
    with pytest.raises(TypeError):
        sr_amd.eval_grad_tree_array_batch([t], X, opts)


def test_output_layout():
    from sr_amd import Options, flatten_trees, parse_expression
    from sr_amd.diff import check_directions, grad_layout, n_grad_of

    opts = Options(binary_operators=["+", "*"], unary_operators=["cos"])
    trees = [parse_expression(e, opts) for e in ("x1", "1.5 * x1 + 2.0", "cos(x2)", "0.5 * (0.25 + (3.0 * x1))")]
    tb = flatten_trees(trees, np.float32)
    assert list(n_grad_of(tb, 7, False)) == [0, 2, 0, 3]
    assert list(n_grad_of(tb, 7, True)) == [7, 7, 7, 7]
    assert list(grad_layout(n_grad_of(tb, 7, False), 10)) == [0, 0, 20, 20, 50]
    assert list(grad_layout(n_grad_of(tb, 7, True), 3)) == [0, 21, 42, 63, 84]
    assert list(grad_layout([], 5)) == [0]
    big = grad_layout([128, 128], 1 << 27)  # (past 2^31 elements: int64 offsets)
    assert big.dtype == np.int64 and big[-1] == 1 << 35
    with pytest.raises(ValueError):
        grad_layout([1, -1], 4)
    d = check_directions(2, 3, 5)
    assert d.dtype == np.int32 and list(d) == [2, 2, 2]


def test_fixture_covers_the_reference_cases():
    with open(FIXTURE) as f:
        g = json.load(f)
    X = np.array(g["X"])
    assert X.shape == (3, 100) and X.min() >= g["scale"] // 16 and X.max() < 5 * g["scale"]
    assert np.array_equal((X / g["scale"]).astype(np.float32).astype(np.float64), X / g["scale"])  # exact in Float32
    cases = {c["name"]: c for c in g["cases"]}
    assert sorted(cases) == ["equation1", "equation2", "equation3", "equation4", "equation5"]
    for name in ("equation1", "equation2", "equation3"):
        d = np.array(cases[name]["d_feature"])
        assert d.shape == (3, 100) and np.isfinite(d).all() and all(np.any(d[f] != 0) for f in range(3))
        assert np.array(cases[name]["value"]).shape == (100,)
    assert np.array(cases["equation1"]["d_feature"]).tolist() == [[1.0] * 100] * 3
    assert np.array(cases["equation4"]["d_constant"]).shape == (1, 100)
    assert np.allclose(cases["equation4"]["d_constant"][0], X[0] / g["scale"], rtol=1e-15)
    assert np.array(cases["equation5"]["d_constant"]).shape == (2, 100)
    assert cases["equation5"]["constants"] == [float(np.float32(2.1)), float(np.float32(-3.2))]
    assert len(cases["equation3"]["constants"]) == 12


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        sys.path[:0] = [HERE, os.path.join(ROOT, "symbolicregression.jl_amd")]
        with open(PROGRAMS, "w") as f:
            json.dump(program_digests(), f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", PROGRAMS)
