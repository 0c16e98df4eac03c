"""CPU: the math program ops (FLOOR .. CAST) through nut_prog_type, the three hipRTC generators
(every kernel tests/test_gpu_math.py runs is compiled here, no GPU needed) and the SQL front
end: every new name lowers and is described, constants fold with the functions the kernels run
(csrc/prog_ops.hpp), the rejected forms are NUT_ERR_PLAN naming the expression."""
import ctypes as C
import json
import re

import pytest

import math_edges as M
from nutdb_amd import _lib as L
from nutdb_amd import NutError, ProgQuery
from nutdb_amd.executor import _prog
from nutdb_amd.sql import Plan
from test_expr_edges_cpu import FakeCol, compile_

C0, C1 = M.C0, M.C1
I, F = L.T_I64, L.T_F64


def prog_type(nodes, types):
    keep = []
    pr = _prog(nodes, keep)
    ct = (C.c_int32 * L.NUT_MAX_PROG_COLS)(*types)
    t = C.c_int32(-1)
    st = L.lib.nut_prog_type(C.byref(pr), ct, len(types), C.byref(t))
    return st, t.value


# ------------------------------------------------------------------ typing
def test_op_numbers_and_abi():
    names = ["floor", "ceil", "trunc", "round", "math", "pow", "sign", "least", "greatest", "cast"]
    assert [L.P[n] for n in names] == list(range(35, 45)) and len(L.PROG_OPS) == 45 and L.PROG_OPS[34] is None
    assert (L.MF_SQRT, L.MF_LOG10, L.CAST_I64, L.CAST_U8, L.CAST_F32, L.MAX_ROUND_DIGITS) == (0, 4, 0, 6, 7, 18)
    assert L.lib.nut_abi_version() == 1


def test_prog_types():
    n = 0
    for op in M.MODES:
        for d in (-18, -2, 0, 2, 18):
            assert prog_type(C0 + [(op, d)], [F]) == (0, L.PT_F64) and prog_type(C0 + [(op, d)], [I]) == (0, L.PT_I64)
            n += 2
        assert prog_type(C0 + C0 + [("eq",), (op, -1)], [I]) == (0, L.PT_I64)  # a bool counts as 0 / 1
    for t in (I, F):
        for m in range(5):
            assert prog_type(C0 + [("math", m)], [t]) == (0, L.PT_F64)
        assert prog_type(C0 + [("sign",)], [t]) == (0, L.PT_I64)
        for c in range(7):
            assert prog_type(C0 + [("cast", c)], [t]) == (0, L.PT_I64)
        assert prog_type(C0 + [("cast", 7)], [t]) == (0, L.PT_F64)
        n += 14
    for op in ("least", "greatest"):
        assert prog_type(C0 + C1 + [(op,)], [I, I]) == (0, L.PT_I64)
        assert prog_type(C0 + C1 + [(op,)], [I, F]) == prog_type(C0 + C1 + [(op,)], [F, I]) == (0, L.PT_F64)
        assert prog_type(C0 + C0 + [("eq",)] + C1 + [(op,)], [I, I]) == (0, L.PT_I64)
    assert prog_type(C0 + C1 + [("pow",)], [I, I]) == (0, L.PT_F64) and n == 68


@pytest.mark.parametrize("nodes, msg", [
    (C0 + [("round", 19)], "outside [-18, 18]"), (C0 + [("floor", -19)], "outside [-18, 18]"),
    (C0 + [("math", 5)], "MATH: unknown function"), (C0 + [("math", -1)], "MATH: unknown function"),
    (C0 + [("cast", 8)], "CAST: unknown target"), (C0 + [("cast", -1)], "CAST: unknown target"),
    (C0 + [("pow",)], "stack underflow"), (C0 + [("least",)], "stack underflow"), (C0 + [(45,)], "unknown program op 45"), (C0 + [(34,)], "unknown program op 34"),
])
def test_prog_type_rejects(nodes, msg):
    assert prog_type(nodes, [F])[0] != 0
    assert msg in L.lib.nut_last_error().decode()


# ------------------------------------------------------------------ hipRTC: every kernel of the GPU file
@pytest.mark.parametrize("name", sorted(M.EVAL_SPECS))
def test_eval_specs_compile(name):
    src, progs = M.EVAL_SPECS[name]
    cols = [FakeCol(t) for t in M.col_types(src)]
    compile_(L.lib.nut_eval_jit_compile, ProgQuery(keys=[], cols=cols, aggs=[("sum", v, None) for v in progs]))


@pytest.mark.parametrize("name", sorted(M.TR_SPECS))
def test_transcendental_specs_compile(name):
    src, progs, _ = M.TR_SPECS[name]
    cols = [FakeCol(t) for t in M.col_types(src)]
    compile_(L.lib.nut_eval_jit_compile, ProgQuery(keys=[], cols=cols, aggs=[("sum", v, None) for v in progs]))


def every_op():
    """one f64 program that adds up every op and literal class over (f64 col 0, int64 col 1)"""
    every = [C0 + [(m, n)] for m in M.MODES for n in (0, 2, -2)] + [C1 + [(m, -2)] for m in M.MODES]
    every += [C0 + [("math", m)] for m in range(5)] + [C0 + C1 + [("pow",)], C0 + [("sign",)], C1 + [("sign",)]]
    every += [C0 + C1 + [(op,)] for op in ("least", "greatest")] + [C1 + C1 + [(op,)] for op in ("least", "greatest")]
    every += [c + [("cast", k)] for c in (C0, C1) for k in range(8)]
    total = every[0]
    for v in every[1:]:
        total = total + v + [("add",)]
    assert len(every) == 44 and len(total) < L.NUT_MAX_PROG_NODES
    return total


def test_every_op_compiles_through_all_three_generators():
    total = every_op()
    cols = [FakeCol("f"), FakeCol("i")]
    pos = total + [("f64", 0, 0.0), ("ge",)]
    key = total + [("cast", 0)]
    compile_(L.lib.nut_eval_jit_compile, ProgQuery(keys=[], cols=cols, aggs=[("sum", total, pos)]))
    compile_(L.lib.nut_groupby_jit_compile, ProgQuery(keys=[key], cols=cols, where=pos, aggs=[("max", total, pos)]))
    compile_(L.lib.nut_select_jit_compile, ProgQuery(keys=[], cols=cols, aggs=[], where=pos))


def test_groupby_key_specs_compile_and_f64_keys_do_not():
    cols = [FakeCol("f"), FakeCol("i")]
    aggs = [("count", None, None), ("sum", C0 + [("round", 2)], None)]
    compile_(L.lib.nut_groupby_jit_compile, ProgQuery(keys=[M.KEY_F, M.KEY_I], cols=cols, aggs=aggs))
    q = ProgQuery(keys=[C0 + [("round", 1)]], cols=cols, aggs=aggs)
    assert L.lib.nut_groupby_jit_compile(C.byref(q.to_spec(None))) != 0
    assert "key program is float64" in L.lib.nut_last_error().decode()


def test_generated_source_carries_the_literals():
    """N and the rounding mode reach the device code as literals (an integer's divisor 10^-N
    then folds to one: the device has no 64-bit divide), N >= 0 over an integer emits nothing"""
    from test_expr_cpu import jit_source
    cols = [FakeCol("f"), FakeCol("i")]
    src = jit_source(ProgQuery(keys=[M.KEY_I], cols=cols, aggs=[("sum", C1 + [("ceil", -18)], None), ("sum", C1 + [("round", 3)], None),
                                                                 ("sum", C0 + [("trunc", 2)], None)]))
    assert "jroundi(((int64_t)v[1][r]), 3, -2)" in src and "jroundi(((int64_t)v[1][r]), 1, -18)" in src
    assert "jroundf(as_f64(v[0][r]), 2, 2)" in src and src.count("jround") == 3 and "p.kc[" not in src.split("struct QShape")[1]


# ------------------------------------------------------------------ SQL
NAMES = [
    ("floor(f)", "floor(f)"), ("FLOOR(f, 2)", "floor(f, 2)"), ("ceil(f)", "ceil(f)"), ("ceiling(f, 1)", "ceil(f, 1)"),
    ("trunc(f)", "trunc(f)"), ("truncate(a, -2)", "trunc(a, -2)"), ("round(f)", "round(f)"), ("round(f, 2)", "round(f, 2)"),
    ("round(a, -2)", "round(a, -2)"), ("round(f, 1 - 3)", "round(f, -2)"), ("sqrt(f)", "sqrt(f)"), ("exp(f)", "exp(f)"),
    ("ln(f)", "ln(f)"), ("log(f)", "ln(f)"), ("log2(a)", "log2(a)"), ("log10(f)", "log10(f)"), ("pow(f, 2)", "pow(f, 2)"),
    ("power(a, f)", "pow(a, f)"), ("sign(f)", "sign(f)"), ("Sign(a)", "sign(a)"), ("least(a, f)", "least(a, f)"),
    ("greatest(a, 0)", "greatest(a, 0)"), ("least(a, f, 3, 4.5)", "least(least(least(a, f), 3), 4.5)"),
    ("greatest(1, a, 2, a, 3, a, 4, a)", "greatest(greatest(greatest(greatest(greatest(greatest(greatest(1, a), 2), a), 3), a), 4), a)"),
    ("toInt64(f / 100)", "toInt64((f / 100))"), ("toInt32(f)", "toInt32(f)"), ("toInt16(a)", "toInt16(a)"), ("toInt8(f)", "toInt8(f)"),
    ("toUInt32(a)", "toUInt32(a)"), ("toUInt16(f)", "toUInt16(f)"), ("toUInt8(a)", "toUInt8(a)"), ("toFloat32(f)", "toFloat32(f)"),
    ("toint64(sqrt(abs(f)) * 10)", "toInt64((sqrt(abs(f)) * 10))"),
]


def test_every_new_name_lowers_and_is_described():
    p = Plan("select " + ", ".join(f"{sql} as x{i}" for i, (sql, _) in enumerate(NAMES)) + " from t")
    assert p.describe()["project"] == [shown for _, shown in NAMES] and len(NAMES) >= 33
    p.prepare({"a": "int64", "f": "float64"})
    p.prepare({"a": "int16", "f": "float32"})


FOLDS = [("round(2.5)", "2"), ("round(3.5)", "4"), ("round(-0.125, 2)", "-0.12"), ("floor(-1.5)", "-2"), ("ceil(1234, -2)", "1300"),
         ("round(1250, -2)", "1300"), ("round(-1250, -2)", "-1300"), ("trunc(-1299, -2)", "-1200"), ("floor(-1201, -2)", "-1300"),
         ("pow(2, 10)", "1024"), ("sqrt(16)", "4"), ("sqrt(2)", "1.4142135623730951"), ("sign(-2.5)", "-1"), ("sign(0.0)", "0"),
         ("least(3, 2, 5)", "2"), ("greatest(3, 2.5)", "3"), ("toInt64(-3.9)", "-3"), ("toInt8(128)", "-128"), ("toInt8(127.9)", "127"),
         ("toUInt8(-1)", "255"), ("toInt32(4294967297)", "1"), ("toInt64(10000000000000000000.0)", "9223372036854775807"),
         ("toFloat32(16777217)", "16777216"), ("toFloat32(0.5)", "0.5"), ("toInt64(pow(2, 62)) + 1", "4611686018427387905"),
         ("log2(8)", "3"), ("exp(0)", "1"), ("ln(1)", "0"), ("log10(1000)", "3"), ("round(9223372036854775807, -1)", "-9223372036854775806")]


def test_constants_fold_with_the_ops_functions():
    for sql, want in FOLDS:
        d = Plan(f"select {sql} as x, a from t").describe()
        assert d["project"][0] == want, (sql, d["project"][0])
    # what no decimal constant holds stays in the program: NaN, infinity, -0.0
    for sql in ("sqrt(-1)", "ln(0)", "ceil(-0.5)", "pow(10, 400)"):
        assert Plan(f"select {sql} as x, a from t").describe()["project"][0] != "0", sql


def test_folded_constant_keeps_the_fused_route():
    p = Plan("select x from t where x < pow(2, 10)")
    d = p.describe()
    assert d["mode"] == "fused" and d["where"] == [{"col": "x", "op": "<", "value": "1024", "value_kind": "decimal"}]
    assert p.route({"x": "int64"}).startswith("fused")
    d = Plan("select x from t where x % 2 = 0 and x >= toInt64(round(99.5))").describe()
    assert d["mode"] == "compiled" and "100" in d["where_expr"] and "round" not in json.dumps(d)


def test_where_aggregates_keys_and_outputs():
    p = Plan("select toInt64(price / 100) as b, count(), round(avg(price), 2), sqrt(sum(price * price) / count()), "
             "sum(case when sign(price) = 1 then ln(price) end), greatest(min(a), 0) from t "
             "where greatest(a, 3) > 3 and floor(price) != 7 group by b having round(sum(price) / count(), 1) > 2 "
             "order by round(sum(price) / count(), 1) desc, b")
    d = p.describe()
    assert d["kind"] == "groupby" and d["keys"] == ["toInt64(price / 100)"] and d["having"] is True
    assert "greatest(a, 3)" in d["where_expr"] and "floor(price)" in d["where_expr"]
    assert [o["from"] for o in d["outputs"] if not o.get("hidden")][:4] == ["key", "agg", "expr", "expr"]
    types = {"price": "float64", "a": "int64"}
    p.prepare(types)
    assert p.route(types) == "packed-groupby"
    p = Plan("select round(a, -2) as k, count() from t group by k")
    p.prepare({"a": "int64"})
    assert p.route({"a": "int32"}) == "packed-groupby"


def test_float64_key_stays_a_plan_error():
    p = Plan("select round(f, 1) as k, count() from t group by k")
    with pytest.raises(NutError, match=r"round\(f, 1\).*float64") as e:
        p.route({"f": "float64"})
    assert e.value.status == 7
    p.route({"f": "int64"})  # (an integer rounds to an integer: a key)


@pytest.mark.parametrize("sql, msg", [
    ("round(f, a)", r"round\(f, a\).*constant integer"), ("round(f, 1.5)", r"round\(f, 1.5\).*constant integer"),
    ("floor(f, 19)", r"floor\(f, 19\).*outside \[-18, 18\]"), ("trunc(f, -19)", r"outside \[-18, 18\]"),
    ("round(f, 1, 2)", r"round\(f, 1, 2\).*takes 1 to 2 arguments"), ("sqrt(f, 2)", r"sqrt\(f, 2\).*takes 1 argument"),
    ("pow(f)", r"pow\(f\).*takes 2 arguments"), ("least(f)", r"least\(f\).*takes 2 to 8 arguments"),
    ("greatest(1, 2, 3, 4, 5, 6, 7, 8, f)", "takes 2 to 8 arguments"), ("toInt8(f, 1)", "takes 1 argument"),
    ("sqrt('x')", r"sqrt\('x'\).*not the string"), ("least(f, 'x')", r"least\(f, 'x'\).*not the string"),
])
def test_rejected_forms_name_the_expression(sql, msg):
    for q in (f"select {sql} from t", f"select a from t where {sql} > 0", f"select sum({sql}) from t"):
        with pytest.raises(NutError, match=msg) as e:
            Plan(q)
        assert e.value.status == 7
    # over aggregates (evaluated per result group on the host): the same errors
    with pytest.raises(NutError, match=msg.split(".*")[-1]) as e:
        Plan("select k, " + re.sub(r"\bf\b", "sum(f)", sql) + " from t group by k")
    assert e.value.status == 7


def test_unknown_function_message_lists_the_new_names():
    with pytest.raises(NutError, match="is not executed") as e:
        Plan("select cbrt(f) from t")
    for name in ("cbrt", "floor", "round", "sqrt", "log10", "pow", "greatest", "toInt64", "toFloat32"):
        assert name in str(e.value)
