"""CPU: TemplateExpression host types, composition, the tied gradient compile, and composition + guards
against an independent stage-by-stage restatement (template_util.staged_eval) — DESIGN.md §16.
"""
import ctypes

import numpy as np
import pytest

import sr_amd
from oracle import Oracle
from sr_amd import (Options, ParametricExpression, TemplateExpression, TemplateExpressionSpec, TemplateStructure, _lib,
                    compose, compute_complexity, flatten_trees, get_scalar_constants, get_tree, parse_expression,
                    set_scalar_constants, string_tree)
from template_util import SUB_OPS, build_case, load_cases, random_template, staged_eval

OPTS = Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos"])


def _tmpl(expressions, combine, trees, opts=OPTS, **kw):
    st = TemplateStructure(expressions, combine, **{k: v for k, v in kw.items() if k != "values"})
    return TemplateExpression({k: parse_expression(v, opts) for k, v in trees.items()}, structure=st,
                              parameters=kw.get("values"))


# ------------------------------------------------------------------ errors and text
def test_arity_errors_carry_the_reference_messages():
    with pytest.raises(ValueError, match="Inconsistent number of arguments passed to f"):
        TemplateStructure(("f",), "f(x1) + f(x1, x2)")
    with pytest.raises(ValueError, match=r"Failed to infer number of features used by \('g',\)"):
        TemplateStructure(("f", "g"), "f(x1)")
    with pytest.raises(ValueError, match="Inconsistent number of arguments passed to f"):
        TemplateStructure(("f",), "f(x1)", num_features={"f": 2})
    assert TemplateStructure(("f", "g"), "f(x1)", num_features={"g": 2}).num_features == {"f": 1, "g": 2}


@pytest.mark.parametrize("combine,msg", [
    ("D(f, 1)(x1)", "D"),
    ("f(x1)^4", "literal integer power"),
    ("f(x1)^-1", "literal integer power"),
    ("f(x1) + q[1]", "not a parameter vector"),
    ("f(x1) + p[3]", "outside"),
    ("f(x1) + p[1] + p[x2]", "both"),
    ("f(x1) + nosuch(x1)", "device catalog"),
    ("f(x1) + z", "unknown name"),
    ("f(x1) +", "cannot parse"),
])
def test_parse_errors(combine, msg):
    with pytest.raises(ValueError, match=msg):
        TemplateStructure(("f",), combine, parameters={"p": 2})


def test_options_accepts_the_spec_and_refuses_others():
    st = TemplateStructure(("f",), "f(x1)")
    assert Options(expression_spec=TemplateExpressionSpec(structure=st)).expression_spec.structure is st
    with pytest.raises(ValueError):
        Options(expression_spec=object())


def test_literal_pow_and_catalog_operators():
    st = TemplateStructure(("f",), "sin(f(x1))^3 + log(x2)^1 + x1^2.0 + max(x1, x2)")
    assert st.unary_ops == ["sin", "safe_log"] and st.binary_ops == ["+", "*", "safe_pow", "max"]
    ex = TemplateExpression({"f": parse_expression("x1", OPTS)}, structure=st)
    c = compose(ex, OPTS)
    assert c.operators.unaops == ("cos", "sin", "safe_log") and c.operators.binops == ("+", "-", "*", "/", "safe_pow", "max")
    assert string_tree(c.tree, c.operators) == "(((((sin(x1) * sin(x1)) * sin(x1)) + log(x2)) + (x1 ^ 2.0)) + max(x1, x2))"


def test_fixture_strings_composition_and_scalars():
    for c in load_cases():
        opts, ex, X, y, rows = build_case(c)
        e = c["expect"]
        assert staged_eval(ex, X, opts)[1] == e["complete"]  # (the restatement reads the text, not the parse)
        if "string" in e:
            assert string_tree(ex, opts) == e["string"]
        if "num_features" in e:
            assert ex.structure.num_features == e["num_features"]
        if "composed" in e:
            assert string_tree(get_tree(ex, opts), opts) == e["composed"]
        if e.get("invalid_variables"):
            assert ex.has_invalid_variables() and compose(ex, opts).invalid
        if "scalar_tail" in e:
            v = get_scalar_constants(ex)
            assert v[-2:].tolist() == e["scalar_tail"]
            v[-2:] = e["set_tail"]
            set_scalar_constants(ex, v)
            assert ex.parameters["p"].tolist() == e["set_tail"]
            with pytest.raises(ValueError, match="parameters"):
                get_tree(ex, opts)


def test_scalar_order_round_trip_complexity_and_copy():
    ex = _tmpl(("f", "g"), "2.0 * f(x1) + g(x2, f(x3)) - p[2]", {"f": "1.5 * x1 + 0.25", "g": "cos(x1 * 3.0)"},
               parameters={"p": 2}, values={"p": [7.0, 8.0]})
    assert get_scalar_constants(ex).tolist() == [1.5, 0.25, 3.0, 7.0, 8.0]
    assert compute_complexity(ex) == 5 + 4 and sr_amd.compute_complexity(ex, OPTS) == 9
    assert string_tree(ex, OPTS) == "f = (1.5 * #1) + 0.25; g = cos((#1 * 3.0))"
    cp = ex.copy()
    set_scalar_constants(cp, [1.0, 2.0, 3.0, 4.0, 5.0])
    assert get_scalar_constants(cp).tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    assert get_scalar_constants(ex).tolist() == [1.5, 0.25, 3.0, 7.0, 8.0] and cp.structure is ex.structure
    with pytest.raises(ValueError):
        set_scalar_constants(cp, [1.0])
    omitted = _tmpl(("f",), "f(x1) + p[1]", {"f": "x1"}, parameters={"p": 3})
    assert omitted.parameters["p"].tolist() == [0.0, 0.0, 0.0]


def test_slots_frozen_marks_and_guards():
    ex = _tmpl(("f", "g"), "2.0 * f(x1) + g(x2, f(x3)) - p[2]", {"f": "1.5 * x1 + 0.25", "g": "cos(x1 * 3.0)"},
               parameters={"p": 2}, values={"p": [7.0, 8.0]})
    c = compose(ex, OPTS)
    assert string_tree(c.tree, c.operators) == "(((2.0 * ((1.5 * x1) + 0.25)) + cos((x2 * 3.0))) - 8.0)"
    assert c.slots == [-1, 0, 1, 2, 4] and c.n_scalars == 5
    # g drops its second argument f(x3): a guard, holding copies of f's scalars
    assert [string_tree(g, c.operators) for g in c.guards] == ["((1.5 * x3) + 0.25)"] and c.guard_slots == [[0, 1]]
    # no guard for a bare data argument, a literal, p[1], or an argument the callee uses
    for combine in ("g(x2, x3)", "g(x2, 1.5)", "g(x2, p[1])", "g(f(x2), x1)"):
        e2 = _tmpl(("f", "g"), combine + " + f(x1)", {"f": "x1", "g": "cos(x1)"}, parameters={"p": 2})
        assert compose(e2, OPTS).guards == []
    # a guard inside a dropped argument is kept too
    e3 = _tmpl(("f", "g"), "g(x1, f(g(x2, x2 / x3)))", {"f": "x1", "g": "cos(x1)"})
    assert [string_tree(g, OPTS) for g in compose(e3, OPTS).guards] == ["(x2 / x3)", "cos(x2)"]


def test_category_parameters_compose_to_a_parametric_expression():
    ex = _tmpl(("f", "g"), "p1[x3] * g(x1) + f(x1, p2[x3]) - p3[1]", {"f": "x1 * x2 + 0.5", "g": "cos(x1)"},
               parameters={"p1": 3, "p2": 3, "p3": 1}, values={"p1": [1, 2, 3], "p2": [4, 5, 6], "p3": [7]})
    c = compose(ex, OPTS)
    assert string_tree(c.tree, c.operators) == "(((p1 * cos(x1)) + ((x1 * p2) + 0.5)) - 7.0)"
    assert c.matrix.tolist() == [[1, 2, 3], [4, 5, 6]] and c.slots == [0, 7] and c.category == 3
    assert ParametricExpression(c.tree, c.matrix).max_parameters == 2
    with pytest.raises(ValueError, match="several category"):
        TemplateStructure(("f",), "f(x1) + p[x2] + p[x3]", parameters={"p": 2})


# ------------------------------------------------------------------ the tied compile (host dry run)
def _names(seq):
    return (ctypes.c_char_p * max(1, len(seq)))(*[s.encode() for s in seq])


def _compile_grad(c, dtype, tied):
    tb = flatten_trees([c.tree], dtype)
    ops, s = c.operators, tb.to_struct()
    ln, bad, depth = np.zeros(1, np.int32), np.zeros(1, np.uint8), ctypes.c_int(0)
    code = np.zeros((256, 4), np.uint32)
    args = (_lib.SR_DTYPE_F32 if dtype == np.float32 else _lib.SR_DTYPE_F64, len(ops.unaops), _names(ops.unaops),
            len(ops.binops), _names(ops.binops), ctypes.byref(s))
    tail = (100, 3, ln.ctypes.data_as(ctypes.c_void_p), bad.ctypes.data_as(ctypes.c_void_p), ctypes.byref(depth),
            code.ctypes.data_as(ctypes.c_void_p), 256)
    if tied:
        slot = np.asarray(c.slots, np.int32)
        ns = np.asarray([c.n_scalars], np.int32)
        ties = _lib.SrScalarTies(slot.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                 ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        _lib.check(_lib.lib.sr_compile_info_grad_tied(*args, None, ctypes.byref(ties), *tail))
    else:
        _lib.check(_lib.lib.sr_compile_info_grad(*args, *tail))
    return code[:int(ln[0])]


def _holds_constant(op) -> bool:
    """csrc/sr_ops.h: LOAD_CONST(_PUSH), or a binary with the CL / CR operand variant (gradient programs carry
    no fused fields above the opcode)."""
    op = int(op)
    return op in (1, 3) or (80 <= op < 80 + 6 * 32 and (op - 80) % 6 >= 4)


def _const_operands(code):
    """The operand index (meta & SR_M_INDEX) of every instruction holding a constant, in program order."""
    return [int(m) & 0xffff for op, m in zip(code[:, 0], code[:, 1]) if _holds_constant(op)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tied_compile_gives_both_copies_the_scalars_slots(dtype):
    """f(x1) - f(x2), f = c * #1 + d: the untied program numbers its constants 0..3 in pre-order, the tied
    one gives both copies' operands the indices 0 and 1; everything else of the program is the same."""
    c = compose(_tmpl(("f",), "f(x1) - f(x2)", {"f": "1.5 * x1 + 0.25"}), OPTS)
    assert c.slots == [0, 1, 0, 1]
    plain, tied = _compile_grad(c, dtype, False), _compile_grad(c, dtype, True)
    assert plain.shape == tied.shape and np.array_equal(plain[:, 0], tied[:, 0]) and np.array_equal(plain[:, 2:], tied[:, 2:])
    assert _const_operands(plain) == [0, 1, 2, 3] and _const_operands(tied) == [0, 1, 0, 1]
    other = [i for i in range(len(plain)) if not _holds_constant(plain[i, 0])]
    assert np.array_equal(plain[other], tied[other])
    # a frozen literal sits behind the scalars: index n_scalars
    c2 = compose(_tmpl(("f",), "2.0 * f(x1)", {"f": "1.5 * x1"}), OPTS)
    assert c2.slots == [-1, 0]
    p2, t2 = _compile_grad(c2, dtype, False), _compile_grad(c2, dtype, True)
    assert _const_operands(p2) == [1, 0] and _const_operands(t2) == [0, 1]  # (program order: 1.5, then 2.0 — frozen: n_scalars = 1)


def test_tied_compile_refuses_a_slot_out_of_range():
    c = compose(_tmpl(("f",), "f(x1) - f(x2)", {"f": "1.5 * x1 + 0.25"}), OPTS)
    c.n_scalars = 1
    with pytest.raises(sr_amd.SRError):
        _compile_grad(c, np.float32, True)


# ------------------------------------------------------------------ the independent restatement
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_composition_and_guards_equal_the_staged_restatement(dtype):
    """200 random templates from a fixed seed (K = 1..3, arities 0..3, sub-trees of 1..9 nodes, 65 rows): the
    oracle on the composed tree plus guards gives the restatement's flag, and its values bit for bit where
    complete.  The restatement alone shows that the set exercises the flags: at least 20 incomplete, at least 5
    incomplete ONLY through an argument its callee drops (complete when such arguments are not evaluated)."""
    rng = np.random.default_rng(1234)
    opts = Options(**SUB_OPS)
    X = rng.standard_normal((3, 65)).astype(dtype)
    n_bad = n_guard_only = 0
    for k in range(200):
        ex = random_template(rng, opts, dtype)
        c = compose(ex, opts)
        orc = Oracle(c.operators.unaops, c.operators.binops)
        want, ok = staged_eval(ex, X, opts)
        _, ok_lenient = staged_eval(ex, X, opts, skip_dropped=True)
        n_bad += not ok
        n_guard_only += (not ok) and ok_lenient
        got, comp = orc.eval_tree_array(flatten_trees([c.tree], dtype), 0, X)
        assert comp == ok_lenient, (k, ex.structure.combine, string_tree(ex, opts))
        for g in c.guards:
            comp = comp and orc.eval_tree_array(flatten_trees([g], dtype), 0, X)[1]
        assert comp == ok, (k, ex.structure.combine, string_tree(ex, opts))
        if ok:
            assert np.array_equal(got.view(np.uint32 if dtype == np.float32 else np.uint64),
                                  want.view(np.uint32 if dtype == np.float32 else np.uint64)), (k, ex.structure.combine)
    assert n_bad >= 20 and n_guard_only >= 5 and n_bad <= 180, (n_bad, n_guard_only)
