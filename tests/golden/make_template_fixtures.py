"""Writes tests/golden/template_known_answers.json: the reference's own known answers from its
TemplateExpression tests (test/integration/ext/loopvectorization/test_template_expression.jl and
test/integration/ext/mlj/templates/test_parametric_template_expressions.jl), re-expressed as data.

Each case holds the structure as text (the body of the reference's ``do`` block), the sub-expressions as
expression strings over ``x1..`` (``x<i>`` is the reference's ``#i``), the operators, the data and what the
reference test asserts: the value its ``@test ... ≈`` compares with (random inputs are drawn here from a
fixed seed and the right-hand side of the reference's test is evaluated in Float64 with numpy), or
``complete = false`` where it asserts ``=== nothing``.  Run from the repository root:

    python tests/golden/make_template_fixtures.py
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ARITH = ["+", "-", "*", "/"]


def case(name, expressions, combine, trees, X, *, binary=ARITH, unary=(), dtype="float64", arguments=None,
         parameters=None, parameter_values=None, y=None, rows=None, **expect):
    return dict(name=name, expressions=list(expressions), combine=combine, trees=trees, binary_operators=list(binary),
                unary_operators=list(unary), dtype=dtype, arguments=arguments, parameters=parameters,
                parameter_values=parameter_values, X=np.asarray(X, dtype=np.float64).tolist(),
                y=None if y is None else np.asarray(y, dtype=np.float64).tolist(), rows=rows, expect=expect)


def main():
    rng = np.random.default_rng(20240521)
    cases = []
    X = rng.standard_normal((3, 5))
    cases.append(case("sin_outside_operators", ("f", "g"), "sin(f(x1, x2)) + g(x3)^2", {"f": "x1 * x2", "g": "x1"}, X,
                      complete=True, predictions=(np.sin(X[0] * X[1]) + X[2] * X[2]).tolist(),
                      string="f = #1 * #2; g = #1"))
    cases.append(case("divide_by_zero", ("f",), "1.0 + f(x1) / x1", {"f": "x1"}, [[0.0], [1.0]], complete=False))
    cases.append(case("divide_ok", ("f",), "1.0 + f(x1) / x1", {"f": "x1"}, [[1.0], [2.0]], complete=True,
                      predictions=[2.0]))
    cases.append(case("power_law_negative", ("f",), "f(x1)^f(x2)", {"f": "x1"}, -rng.random((2, 32)),
                      binary=ARITH + ["^"], complete=False))
    cases.append(case("feature_constraints_valid", ("f", "g"), "f(x1, x2) + g(x3)", {"f": "x1 + x2", "g": "x1"},
                      [[1.0], [2.0], [3.0]], complete=True, predictions=[6.0]))
    cases.append(case("feature_constraints_f_uses_x3", ("f", "g"), "f(x1, x2) + g(x3)", {"f": "x1 + x3", "g": "x1"},
                      [[1.0], [2.0], [3.0]], complete=False, invalid_variables=True))
    cases.append(case("feature_constraints_g_uses_x2", ("f", "g"), "f(x1, x2) + g(x3)", {"f": "x1 + x2", "g": "x2"},
                      [[1.0], [2.0], [3.0]], complete=False, invalid_variables=True))
    cases.append(case("argument_less", ("f", "g"), "f() + g(x1, x2)", {"f": "3.0", "g": "x1 + x2"}, [[1.0], [2.0]],
                      binary=["+", "*", "/", "-"], unary=["sin", "cos"], complete=True, predictions=[6.0],
                      num_features={"f": 0, "g": 2}))
    X = rng.standard_normal((2, 7))
    cases.append(case("nested_calls", ("f", "g"), "f(f(f(x1))) - f(g(x2, x1))", {"f": "x1", "g": "x2 * x2"}, X,
                      complete=True, predictions=(X[0] - X[0] * X[0]).tolist(), composed="(x1 - (x1 * x1))",
                      num_features={"f": 1, "g": 2}))
    X = rng.standard_normal((2, 32))
    cases.append(case("literal_pow", ("f", "g"), "f(x1) * g(x2)^2", {"f": "x1 + x1", "g": "x1"}, X,
                      binary=["+", "*", "/", "-"], unary=["sin", "cos"], complete=True,
                      predictions=((X[0] + X[0]) * (X[1] * X[1])).tolist()))
    cases.append(case("float64_literal_float32_data", ("f",), "0.5 * f(x1, x2)", {"f": "x1 + x2"},
                      [[1.0, 2.0], [3.0, 4.0]], binary=["+", "*", "/", "-"], dtype="float32", y=[2.0, 3.0],
                      complete=True, predictions=[2.0, 3.0], loss=0.0))
    X = np.array([[1.0, 2.0, 3.0], [2.0, 3.0, 4.0], [0.0, 0.0, 0.0]])
    y = 2.0 * X[0] + X[1] ** 2
    pred = X[0] + 3.0
    for rows in (None, [0, 1]):
        sel = slice(None) if rows is None else rows
        cases.append(case("parameters_sum" + ("" if rows is None else "_batched"), ("f",), "f(x) + p[1] + p[2]",
                          {"f": "x1"}, X, binary=["+", "*"], dtype="float32", arguments=["x"], parameters={"p": 2},
                          parameter_values={"p": [1.0, 2.0]}, y=y, rows=rows, complete=True,
                          predictions=pred[sel].tolist(), loss=float(np.mean((pred[sel] - y[sel]) ** 2))))
    cases.append(case("parameters_in_scalar_constants", ("f",), "f(x) + p[1]", {"f": "x1"}, [[5.0, 6.0]],
                      arguments=["x"], parameters={"p": 2}, parameter_values={"p": [1.0, 2.0]}, complete=True,
                      predictions=[6.0, 7.0], scalar_tail=[1.0, 2.0], set_tail=[3.0, 4.0]))
    with open(os.path.join(HERE, "template_known_answers.json"), "w") as f:
        json.dump({"cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
