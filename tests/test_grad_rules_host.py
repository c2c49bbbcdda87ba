"""CPU: the gradient-rule fixture (tests/golden/grad_rules.json) against the gradient COMPILER and the CPU oracle.

No GPU here; what test_gpu_grad_rules.py then runs on the device is pinned twice over:
  * every case's GRADIENT program (sr_compile_info_grad / _parametric: the programs eval_grad_batch compiles)
    holds the opcode variants the case is there to hit, and over all cases every (binary operator x operand
    variant), every parameter-operand opcode and every unary opcode with a derivative rule appears — the
    matrix is read from csrc/sr_ops.h's enums, not kept here;
  * every case's mpmath reference agrees with central differences of the CPU oracle's Float64 loss
    (Oracle.loss_grad_fd, param_grad_fd) within 1e-6 max(1, |ref|_inf), the bar of the finite-difference tests
    in test_gpu_grad.py — every case, none filtered on the differences' own error estimate.
"""
import re

import numpy as np
import pytest

from bytecode_vm import compile_info
from grad_rules_util import arrays, batches, fixture, options, parameters, sr_ops_header, tree_batch, twin_batch
from oracle import Oracle
from parametric_grad_util import param_grad_fd
from parametric_util import x_ext

VARIANTS = ("SL", "SR", "FL", "FR", "CL", "CR")  # SR_V_*: the order of csrc/sr_ops.h
COMMUTING = ("ADD", "MUL")  # the compiler canonicalises + and * to their R variants


def _enum(src, name, prefix):
    body = re.search(r"enum %s : \w+ \{(.*?)\};" % name, src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names = [s.strip().split("=")[0].strip() for s in body.split(",") if s.strip()]
    assert names[0] == prefix + "NONE" and names[-1] == prefix + "COUNT", names
    return {n[len(prefix):]: k for k, n in enumerate(names) if n not in (prefix + "NONE", prefix + "COUNT")}


@pytest.fixture(scope="module")
def isa():
    src = sr_ops_header()
    opc = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bSR_OP_(\w+) = (\d+)u", src)}
    unary = _enum(src, "SrUnaryOp", "SR_U_")
    # the unary operators without a derivative rule: the ones sr_unary_grad_supported names
    rule = re.search(r"sr_unary_grad_supported\(uint32_t op\) \{ return ([^;]*);", src).group(1)
    for name in re.findall(r"op != SR_U_(\w+)", rule):
        unary.pop(name, None)
    return dict(opc=opc, unary=unary, binary=_enum(src, "SrBinaryOp", "SR_B_"))


@pytest.fixture(scope="module")
def programs():
    """{case name: [(opcode, operand index), ...]} of every case's gradient program."""
    out = {}
    for (group, dataset, spec, weighted, rows), cases in batches().items():
        opts = options(group, spec)
        tb = tree_batch(cases, opts, np.float64)
        code, offs, bad, depth = compile_info(opts, tb, 200, 3, np.float64, grad=True)
        assert not bad.any() and depth <= 62
        for k, c in enumerate(cases):
            ins = code[offs[k]:offs[k + 1]]
            assert np.all(ins["op"] >> 16 == 0), "gradient programs carry no fused post operators"
            out[c["name"]] = [(int(o) & 0x1FF, int(m) & 0xFFFF) for o, m in zip(ins["op"], ins["meta"])]
    return out


def _hit_opcode(isa, hit):
    kind, _, rest = hit.partition(":")
    opc = isa["opc"]
    if kind == "U":
        return opc["UNARY0"] + isa["unary"][rest]
    name, v = rest.split(":")
    if kind == "B":
        return opc["BINARY0"] + 6 * (isa["binary"][name] - 1) + VARIANTS.index(v)
    assert kind == "P"
    return opc["PBIN0"] + 2 * (isa["binary"][name] - 1) + ("PL", "PR").index(v)


def test_every_case_compiles_to_the_variants_it_is_there_to_hit(isa, programs):
    assert len(programs) == len(fixture()["cases"])
    for c in fixture()["cases"]:
        prog = programs[c["name"]]
        ops = [o for o, _ in prog]
        wanted = [_hit_opcode(isa, h) for h in c["hits"] if h[1] == ":"]
        for h, o in zip([h for h in c["hits"] if h[1] == ":"], wanted):
            assert o in ops, (c["name"], h, ops)
        if "LOADP" in c["hits"]:
            assert isa["opc"]["LOAD_PARAM"] in ops, c["name"]
        if "LOADP_PUSH" in c["hits"]:
            assert isa["opc"]["LOAD_PARAM_PUSH"] in ops, c["name"]
        for h in c["hits"]:
            if h.startswith("SLOT>="):
                # a constant OPERAND of the hit operators (their C variants) sits at that slot or beyond
                slots = [i for o, i in prog if o in wanted and (o - isa["opc"]["BINARY0"]) % 6 >= 4]
                assert slots and max(slots) >= int(h[6:]), (c["name"], h, slots)
        # the constants' slots are the pre-order numbering, each used once
        first_const = (isa["opc"]["LOAD_CONST"], isa["opc"]["LOAD_CONST_PUSH"])
        slots = [i for o, i in prog if o in first_const or
                 (isa["opc"]["BINARY0"] <= o < isa["opc"]["LOAD_PARAM"] and (o - isa["opc"]["BINARY0"]) % 6 >= 4)]
        assert sorted(slots) == list(range(len(c["constants"]))), c["name"]


def test_the_cases_cover_every_opcode_with_a_derivative_rule(isa, programs):
    seen = {o for prog in programs.values() for o, _ in prog}
    opc = isa["opc"]
    missing = []
    assert len(isa["unary"]) == 32 and len(isa["binary"]) == 16
    for name, u in isa["unary"].items():
        if opc["UNARY0"] + u not in seen and opc["UNARY_INF0"] + u not in seen:
            missing.append("unary " + name)
    for name, b in isa["binary"].items():
        for k, v in enumerate(VARIANTS):
            if name in COMMUTING and v[1] == "L":
                assert opc["BINARY0"] + 6 * (b - 1) + k not in seen, "the compiler commutes + and *"
            elif opc["BINARY0"] + 6 * (b - 1) + k not in seen:
                missing.append(f"binary {name} {v}")
        for k, v in enumerate(("PL", "PR")):
            if not (name in COMMUTING and v == "PL") and opc["PBIN0"] + 2 * (b - 1) + k not in seen:
                missing.append(f"parameter operand {name} {v}")
    for lead in ("LOAD_FEAT", "LOAD_CONST", "LOAD_PARAM", "LOAD_FEAT_PUSH", "LOAD_CONST_PUSH", "LOAD_PARAM_PUSH"):
        if opc[lead] not in seen:
            missing.append(lead)
    assert not missing, missing


def test_the_fixture_holds_the_coverage_the_rules_need():
    fx = fixture()
    names = [c["name"] for c in fx["cases"]]
    assert len(set(names)) == len(names)
    for d in fx["datasets"].values():
        assert len(d["X"]) == 3 and all(len(v) == 200 for v in d["X"] + [d["y"], d["ym"], d["w"], d["cls"]])
        assert set(d["cls"]) == {1, 2, 3} and set(d["ym"]) == {-d["scale"], d["scale"]}
        for v in d["X"] + [d["y"], d["w"]]:  # multiples of 2^-12 below 2^12: exact in Float32
            assert d["scale"] == 4096 and all(isinstance(k, int) and abs(k) < 1 << 24 for k in v)
    for c in fx["cases"]:
        n = len(c["constants"]) + (6 if fx["groups"][c["group"]]["max_parameters"] else 0)
        assert len(c["grad"]) == len(c["zero"]) == len(c["u32"]) == len(c["u64"]) == n
        assert all(np.float64(np.float32(v)) == v for v in c["constants"])
        assert all((g == 0 and u == 0) == bool(z) for g, u, z in zip(c["grad"], c["u64"], c["zero"])), c["name"]
    zeros = {c["name"]: c["zero"] for c in fx["cases"]}
    for u in ("sign", "round", "floor", "ceil"):  # c3 * u(c1 * x1 + c2): pre-order c3, c1, c2
        assert zeros[f"unary/{u}"] == [0, 1, 1]
    assert zeros["loss/ZeroOneLoss()/plain"] == [1, 1, 1] == zeros["loss/ZeroOneLoss()/weighted"]
    assert zeros["param/p2_only"][2:] == [1, 0, 1, 0, 1, 0]       # p1 unused: P[1, c] exactly 0
    assert zeros["param/class_absent"][2:] == [0, 0, 0, 0, 1, 1]  # no row of class 3
    assert len([n for n in names if n.startswith("loss/")]) == 40
    assert len(next(c for c in fx["cases"] if c["name"] == "windows/70_constants")["constants"]) == 70


def test_every_case_agrees_with_the_oracles_finite_differences():
    """The mpmath references against an independent implementation: central differences (Richardson) of the
    C oracle's Float64 loss.  Bar: 1e-6 max(1, |ref|_inf), every case."""
    n_checked = 0
    for (group, dataset, spec, weighted, rows), cases in batches().items():
        K = fixture()["groups"][group]["max_parameters"]
        opts = options(group, spec, parametric=False)
        orc = Oracle.from_options(opts)
        X, y, w, cls = arrays(dataset, opts, np.float64)
        if rows is not None:
            r = np.asarray(rows)
            X, y, w, cls = X[:, r], y[r], w[r], cls[r]
        w = w if weighted else None
        kw = dict(loss_kind=opts.loss_kind, loss_param=opts.loss_param)
        if K:
            P = parameters(np.float64)
            tb = twin_batch(cases, opts, 3, np.float64)
            Xe = x_ext(X, P, cls)
            gc, loss, comp = orc.loss_grad_fd(tb, Xe, y, w, **kw)
            assert opts.loss_kind == 0  # (param_grad_fd takes no loss parameter)
            gp, _ = param_grad_fd(orc, tb, X, y, cls, P, w)
        else:
            tb = tree_batch(cases, opts, np.float64)
            gc, loss, comp = orc.loss_grad_fd(tb, X, y, w, **kw)
        co = tb.constant_offsets()
        for k, c in enumerate(cases):
            g = gc[co[k]:co[k + 1]]
            if K:
                g = np.concatenate([g, gp[k].T.ravel()])  # constants, then P column-major
            ref = np.asarray(c["grad"])
            scale = max(1.0, float(np.abs(ref).max()))
            assert comp[k] and abs(loss[k] - c["loss"]) <= 1e-12 * max(1.0, abs(c["loss"])), (c["name"], loss[k], c["loss"])
            assert g.shape == ref.shape and np.all(np.abs(g - ref) <= 1e-6 * scale), (c["name"], g, ref)
            n_checked += 1
    assert n_checked == len(fixture()["cases"])
