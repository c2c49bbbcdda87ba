"""CPU: the `complete` flag's two rules (validity_util.py) against the oracle, the compiler's check placement and
the bytecode VM.  No GPU.

The oracle (oracle/de_eval_impl.h) and the restatement (validity_util.analyse / verdict) were written separately;
here they must agree on every form and control, in both precisions.  The compiled programs must then carry one
check bit per array-checked node that is no constant, one inf form per inf-substituting node, and `static_bad`
exactly where the rules call a tree incomplete through a constant alone: a compiler that forgets a check site
(`arr_check` in a branch of evalmark, const_operand_check on an operand form) fails here without a GPU.
"""
import numpy as np
import pytest

import bytecode_vm
import validity_util as V
from bytecode_vm import BINARY0, CHECK, PAIR0, PBC_CHECK, POST_CHECK, POST_INF, UNARY_INF0
from oracle import Oracle
from parametric_util import to_parametric, x_ext
from sr_amd import parse_expression

OPSETS = ("basic", "full")
N_A, BAD_A = 65, 64  # rule A on the CPU: one ragged size, the bad row last
N_B = (1153, 4161)


def _oracle(opset):
    return Oracle.from_options(V.options(opset))


def _flags(opset, tb, X, n_threads=8):
    y = np.zeros(X.shape[1], dtype=X.dtype)
    return _oracle(opset).eval_loss_batch(tb, X, y, n_threads=n_threads)


# ------------------------------------------------------------------------------------------- the helper itself
def test_the_set_covers_every_operator_position_and_role():
    """rule_a_forms asserts its own coverage when it builds the set (every operator in every position under every
    wrapper with an infinite and a NaN producer; an absorbing form for every operator that has one); here the
    counts, the reasons of what is left out, and rule B's roles."""
    for opset in OPSETS:
        forms = V.rule_a_forms(opset)
        un, bi = V.OPSETS[opset]["unary_operators"], V.OPSETS[opset]["binary_operators"]
        assert {f.absorber for f in forms} == set(un) | set(bi)
        assert {(f.absorber, f.position) for f in forms if f.position} == {(b, p) for b in bi for p in V.POSITIONS}
        assert sum(len(V.rule_a_forms(opset, g)) for g in V.GROUPS) == len(forms)
        for kind, absorber, pos, reason in V.excluded(opset):
            assert absorber in V.DOMAIN and V.DOMAIN[absorber] in reason, (kind, absorber, pos)
        for dtype_name in V.DTYPES:
            for n in N_B:
                assert V.rule_b_roles(opset, dtype_name, n) >= V.RULE_B_ROLES, (opset, dtype_name, n)
    assert len(V.rule_a_forms("full")) == 4625 and len(V.rule_a_forms("basic")) == 1339
    assert sum(f.absorbing for f in V.rule_a_forms("full")) == 1970
    # absorbing forms of the operators the fixed tests never use
    full = {f.expr for f in V.rule_a_forms("full") if f.absorbing}
    for e in ("inv(exp(x1))", "tanh(exp(x1))", "(x2 > exp(x1))", "cond(neg(exp(x1)), x2)", "min(exp(x1), x2)",
              "atan2(2.0, exp(x1))", "atan((x2 / x3))"):
        assert e in full, e


# ------------------------------------------------------------------------------------------- rules against the oracle
@pytest.mark.parametrize("dtype_name", list(V.DTYPES))
@pytest.mark.parametrize("opset", OPSETS + ("grad",))
def test_rule_a_vs_oracle(opset, dtype_name):
    T = V.DTYPES[dtype_name]
    for n, bad_row in ((N_A, BAD_A), (1153, 0)):
        data = V.rule_a_data(n, T, bad_row)
        for group in V.GROUPS:
            tb = V.rule_a_batch(opset, group, dtype_name)
            forms = V.rule_a_forms(opset, group)
            loss, comp = _flags(opset, tb, data[group])
            wrong = [forms[k].expr for k in np.nonzero(comp)[0]]
            assert not wrong and np.all(np.isposinf(loss)), (group, n, wrong[:8])
            closs, ccomp = _flags(opset, tb, data["control"])
            if group == "K":
                assert not ccomp.any()
                continue
            wrong = [(forms[k].expr, float(closs[k])) for k in np.nonzero(~ccomp | ~np.isfinite(closs))[0]]
            assert not wrong, (group, n, wrong[:8])


@pytest.mark.parametrize("dtype_name", list(V.DTYPES))
@pytest.mark.parametrize("opset", OPSETS)
def test_rule_a_restatement_vs_construction(opset, dtype_name):
    """validity_util.verdict (numpy values + the restated control flow) gives what the forms were built to give."""
    T = V.DTYPES[dtype_name]
    opts = V.options(opset)
    data = V.rule_a_data(3, T, 2)
    n_forms = 0
    for group in V.GROUPS:
        for f in V.rule_a_forms(opset, group):
            tree = parse_expression(f.expr, opts)
            bad, static = V.verdict(tree, data[group], T, opts.operators)
            assert not bad and static == (group == "K"), f
            if group != "K":
                assert V.verdict(tree, data["control"], T, opts.operators) == (True, False), f
            n_forms += 1
    assert n_forms == len(V.rule_a_forms(opset))


@pytest.mark.parametrize("n", N_B)
@pytest.mark.parametrize("dtype_name", list(V.DTYPES))
@pytest.mark.parametrize("opset", OPSETS)
def test_rule_b_vs_oracle(opset, dtype_name, n):
    T = V.DTYPES[dtype_name]
    tb, want = V.rule_b_batch(opset, dtype_name, n)
    _, comp = _flags(opset, tb, V.rule_b_data(n, T))
    forms = V.rule_b_forms(opset, dtype_name, n)
    assert np.array_equal(comp, want), [(forms[k][0], bool(comp[k])) for k in np.nonzero(comp != want)[0]]
    assert want.sum() >= 20 and (~want).sum() >= 20


@pytest.mark.parametrize("dtype_name", list(V.DTYPES))
def test_rule_a_parametric_vs_oracle(dtype_name):
    """The parametric twin (p1 for x1, p2 for x3; the bad class on one row) is the plain tree on [X; P[:, class]]."""
    T = V.DTYPES[dtype_name]
    X = V.rule_a_data(N_A, T, BAD_A)["control"]
    for group in V.GROUPS:
        ext = V.rule_a_batch("full", group, dtype_name, parametric=True)
        P = V.rule_a_params(group, T)
        for bad in (True, False):
            cls = np.ones(N_A, dtype=np.int32)
            if bad:
                cls[BAD_A] = 2
            _, comp = _flags("full", ext, x_ext(X, P, cls))
            assert not comp.any() if (bad or group == "K") else comp.all(), (group, bad)


# ------------------------------------------------------------------------------------------- compiled programs
# csrc/sr_ops.h's opcodes and bits: bytecode_vm's where it has them (it executes them against the oracle in
# test_compiler.py); SR_OP_LOAD_DERIVED, SR_OP_LOAD_PARAM and SR_OP_PBIN0, which it does not interpret, from the header
LOAD_DERIVED, LOAD_PARAM, PBIN0 = 78, 184, 186


def _program_counts(code, lo, hi):
    op = code["op"][lo:hi].astype(np.int64)
    meta = code["meta"][lo:hi].astype(np.int64)
    opc = op & 0x1FF
    kinds = dict(m_check=int(np.sum((meta & CHECK) != 0)), post_check=int(np.sum((op & POST_CHECK) != 0)),
                 pbc_check=int(np.sum((op & PBC_CHECK) != 0)),
                 unary_inf=int(np.sum((opc >= UNARY_INF0) & (opc < LOAD_DERIVED))),
                 post_inf=int(np.sum((op & POST_INF) != 0)))
    return kinds, set(int(o) for o in opc)


def _batches(opset, dtype_name):
    """[(what, plain batch, its trees' expressions, expected static_bad, n_rows, parametric twin)]."""
    T = V.DTYPES[dtype_name]
    out = []
    for group in V.GROUPS:
        forms = V.rule_a_forms(opset, group)
        ext = V.rule_a_batch(opset, group, dtype_name, parametric=True)
        out.append((f"A/{group}", V.rule_a_batch(opset, group, dtype_name), [f.expr for f in forms],
                    np.full(len(forms), group == "K"), N_A, to_parametric(ext, V.NF, V.rule_a_params(group, T))))
    for n in N_B:
        forms = V.rule_b_forms(opset, dtype_name, n)
        opts = V.options(opset)
        X = V.rule_b_data(n, T)
        static = np.array([V.verdict(parse_expression(e, opts), X, T, opts.operators)[1] for e, _ in forms])
        assert static.sum() >= 5
        param = to_parametric(V.rule_b_batch(opset, dtype_name, n, parametric=True)[0], V.NF, V.rule_b_params(n, T))
        out.append((f"B/{n}", V.rule_b_batch(opset, dtype_name, n)[0], [e for e, _ in forms], static, n, param))
    return out


@pytest.mark.parametrize("dtype_name", list(V.DTYPES))
@pytest.mark.parametrize("opset", OPSETS)
def test_check_placement_in_compiled_programs(opset, dtype_name):
    T = V.DTYPES[dtype_name]
    opts = V.options(opset)
    seen, opcodes, n_programs, named = {}, {"plain": set(), "parametric": set()}, 0, 0
    for what, plain, exprs, static, n_rows, param in _batches(opset, dtype_name):
        for family, tb in (("plain", plain), ("parametric", param)):
            if tb is None:
                continue
            code, offs, bad, _ = bytecode_vm.compile_info(opts, tb, n_rows, V.NF, T)
            wrong = [exprs[k] for k in np.nonzero(bad != static)[0]]
            assert not wrong, (what, family, "static_bad", wrong[:8])
            for k, e in enumerate(exprs):
                got, ops = _program_counts(code, offs[k], offs[k + 1])
                if bad[k]:  # no program: the launch never runs the tree
                    assert offs[k + 1] == offs[k], (what, family, e)
                    continue
                tree = parse_expression(e, opts)
                a = V.analyse(tree)
                order = tree.preorder()
                live = [i for i in a["checked"] if not (i in a["folded"] or (order[i].degree == 0 and order[i].constant))]
                n_bits = got["m_check"] + got["post_check"] + got["pbc_check"]
                assert n_bits == len(live), (what, family, e, got, sorted(live))
                assert got["unary_inf"] + got["post_inf"] == len(a["infsub"]), (what, family, e, got, sorted(a["infsub"]))
                for name, c in got.items():
                    seen[name] = seen.get(name, 0) + c
                if what.startswith("B/"):  # the two forms whose only failing check is a fused one
                    assert e != V.RULE_B_POST_CHECK or got["post_check"] == 1, (what, e, got)
                    assert e != V.RULE_B_PBC_CHECK or got["pbc_check"] == 1, (what, e, got)
                    named += e in (V.RULE_B_POST_CHECK, V.RULE_B_PBC_CHECK)
                if what.startswith("A/") and what != "A/K":  # the deep wrapper, and it alone, needs the LDS stack
                    deep = V.rule_a_forms(opset, what[2:])[k].wrapper == "deep"
                    d = bytecode_vm.compile_info(opts, tb.take([k]), n_rows, V.NF, T)[3] if deep or k % 50 == 0 else 0
                    assert (d > 2) if deep else (d <= 2), (what, family, e, d)
                opcodes[family] |= ops
                n_programs += 1
    # coverage of encodings: all three kinds of check bit, both inf forms, PAIR, every operand variant
    assert all(seen.get(k, 0) > 0 for k in ("m_check", "post_check", "pbc_check", "unary_inf", "post_inf")), seen
    plain = opcodes["plain"]
    assert any(o >= PAIR0 for o in plain)
    variants = {(o - BINARY0) % 6 for o in plain if BINARY0 <= o < LOAD_PARAM}
    assert variants == {0, 1, 2, 3, 4, 5}, variants  # SL SR FL FR CL CR
    pvariants = {(o - PBIN0) % 2 for o in opcodes["parametric"] if PBIN0 <= o < PAIR0}
    assert pvariants == {0, 1} and LOAD_PARAM in opcodes["parametric"], sorted(opcodes["parametric"])  # PL PR
    assert n_programs >= 2 * len(V.rule_a_forms(opset, "E")) and named == 4 * len(N_B)


# ------------------------------------------------------------------------------------------- the bytecode VM
@pytest.mark.parametrize("dtype_name", list(V.DTYPES))
def test_bytecode_vm_gives_the_rules_flags(dtype_name):
    """The numpy interpreter of the compiled programs (the kernel's instruction semantics) on the BASIC forms."""
    T = V.DTYPES[dtype_name]
    opts = V.options("basic")
    data = V.rule_a_data(N_A, T, BAD_A)
    y = np.zeros(N_A, dtype=T)
    n_forms = 0
    for group in V.GROUPS:
        tb = V.rule_a_batch("basic", group, dtype_name)
        forms = V.rule_a_forms("basic", group)
        loss, comp = bytecode_vm.eval_loss_batch(opts, tb, data[group], y, T)
        assert not comp.any() and np.all(np.isposinf(loss)), [forms[k].expr for k in np.nonzero(comp)[0]][:8]
        if group != "K":
            loss, comp = bytecode_vm.eval_loss_batch(opts, tb, data["control"], y, T)
            assert comp.all() and np.isfinite(loss).all(), [forms[k].expr for k in np.nonzero(~comp)[0]][:8]
        n_forms += tb.n_trees
    assert n_forms == len(V.rule_a_forms("basic"))
    n = N_B[0]
    tb, want = V.rule_b_batch("basic", dtype_name, n)
    _, comp = bytecode_vm.eval_loss_batch(opts, tb, V.rule_b_data(n, T), np.zeros(n, dtype=T), T)
    forms = V.rule_b_forms("basic", dtype_name, n)
    assert np.array_equal(comp, want), [(forms[k][0], bool(comp[k])) for k in np.nonzero(comp != want)[0]]
