"""Narrow physical column types (NUT_T_I32 .. NUT_T_F32, include/nutexec.h) without a GPU:
type checking, the generated kernels' run-time compilation (hipRTC needs no device) and
the rejections of the fused mode."""
import ctypes as C

import pytest
import torch

from nutdb_amd import _lib as L
from nutdb_amd.executor import Agg, AggQuery, ProgQuery, _phys_code

NARROW = [(torch.int32, L.T_I32), (torch.int16, L.T_I16), (torch.int8, L.T_I8), (torch.uint8, L.T_U8),
          (torch.float32, L.T_F32)]
for _name, _code in (("uint16", L.T_U16), ("uint32", L.T_U32)):
    if hasattr(torch, _name):
        NARROW.append((getattr(torch, _name), _code))
ALL_CODES = [L.T_I32, L.T_I16, L.T_I8, L.T_U32, L.T_U16, L.T_U8, L.T_F32]


class FakeCol:
    """stands in for a tensor when only types matter (no device pointer is read)"""

    def __init__(self, dtype):
        self.dtype = dtype
        self.device = None

    def numel(self):
        return 0

    def is_contiguous(self):
        return True

    def dim(self):
        return 1

    def data_ptr(self):
        return 0


def prog_type(nodes, types):
    keep = []
    from nutdb_amd.executor import _prog
    t = C.c_int32()
    arr = (C.c_int32 * len(types))(*types)
    L.check(L.lib.nut_prog_type(C.byref(_prog(nodes, keep)), arr, len(types), C.byref(t)), "nut_prog_type")
    return t.value


def mixed_spec(codes):
    """WHERE, a computed key and SUM / MIN / MAX / COUNT over columns of the given nut_type
    codes (one COL node per column, so every column is loaded)"""
    n = len(codes)
    s = L.NutAggSpec()
    keep = []
    s._keep = keep
    from nutdb_amd.executor import _prog
    s.prog_mode = 1
    s.nprog_cols = n
    for i, c in enumerate(codes):
        s.prog_col_type[i] = c
    total = [("col", 0), ("to_f64",)]
    for i in range(1, n):
        total += [("col", i), ("add",)]
    ints = [i for i, c in enumerate(codes) if c not in (L.T_F64, L.T_F32)]
    s.where = _prog([("col", ints[0]), ("i64", 0, 3), ("gt",)], keep)
    s.nkeys = 1
    s.key_prog[0] = _prog([("col", ints[-1])], keep)
    s.naggs = 4
    for a, op in enumerate((L.AGG_SUM, L.AGG_MIN, L.AGG_MAX, L.AGG_COUNT)):
        s.agg_op[a] = op
        if op != L.AGG_COUNT:
            s.agg_val[a] = _prog(total, keep)
    return s


def test_prog_type_maps_narrow_codes():
    for code in ALL_CODES:
        want = L.PT_F64 if code == L.T_F32 else L.PT_I64
        assert prog_type([("col", 0)], [code]) == want
        assert prog_type([("col", 0), ("col", 1), ("add",)], [code, L.T_I64]) == want
        assert prog_type([("col", 0), ("col", 1), ("add",)], [code, L.T_F64]) == L.PT_F64
        assert prog_type([("col", 0), ("i64", 0, 3), ("lt",)], [code]) == L.PT_BOOL
    for dt, code in NARROW:
        assert _phys_code(FakeCol(dt)) == code


def test_jit_compiles_all_seven_codes_mixed():
    """one spec reading a column of every narrow type next to int64 / float64 columns
    compiles into all three generated kernels"""
    s = mixed_spec(ALL_CODES + [L.T_I64, L.T_F64])
    assert L.lib.nut_groupby_jit_compile(C.byref(s)) == 0, L.lib.nut_last_error()
    assert L.lib.nut_select_jit_compile(C.byref(s)) == 0, L.lib.nut_last_error()
    s.naggs = 3  # projections: every output has a value program (COUNT has none)
    assert L.lib.nut_eval_jit_compile(C.byref(s)) == 0, L.lib.nut_last_error()


def test_jit_compiles_sixteen_int8_columns():
    s = mixed_spec([L.T_I8] * L.NUT_MAX_PROG_COLS)
    assert L.lib.nut_groupby_jit_compile(C.byref(s)) == 0, L.lib.nut_last_error()


def jit_source(spec):
    buf = C.create_string_buffer(1 << 16)
    ln = C.c_size_t()
    L.check(L.lib.nut_groupby_jit_source(C.byref(spec), buf, 1 << 16, C.byref(ln)), "nut_groupby_jit_source")
    return buf.value.decode()


def test_jit_source_carries_the_column_types():
    """the generated shape names each column's physical type (4 bits per column), so two
    specs that differ only in a column's width never share a compiled kernel; an 8-byte
    spec differs from its narrow twin in that one constant only"""
    wide = jit_source(mixed_spec([L.T_I64, L.T_F64, L.T_I64]))
    narrow = jit_source(mixed_spec([L.T_I32, L.T_F32, L.T_U8]))
    assert f"kColTypes = {L.T_I64 | L.T_F64 << 4 | L.T_I64 << 8}ull" in wide
    assert f"kColTypes = {L.T_I32 | L.T_F32 << 4 | L.T_U8 << 8}ull" in narrow
    diff = [(a, b) for a, b in zip(wide.splitlines(), narrow.splitlines()) if a != b]
    assert len(wide.splitlines()) == len(narrow.splitlines())
    assert len(diff) == 1 and "kColTypes" in diff[0][0]


def test_unknown_program_column_type_is_rejected():
    s = mixed_spec([L.T_I64, L.T_F64])
    s.prog_col_type[1] = 10
    assert L.lib.nut_groupby_jit_compile(C.byref(s)) == 1
    s.prog_col_type[1] = -1
    assert L.lib.nut_groupby_jit_compile(C.byref(s)) == 1


@pytest.mark.parametrize("code", ALL_CODES)
def test_fused_spec_rejects_narrow_types(code):
    """fused mode (val_type / pred_type) stays int64 / float64: NUT_ERR_INVALID_ARG naming
    the column"""
    s = L.NutAggSpec()
    s.nkeys = 0
    s.nvals = 2
    s.val_type[0] = L.T_F64
    s.val_type[1] = code
    s.naggs = 1
    s.agg_op[0] = L.AGG_SUM
    s.agg_expr[0] = L.EX_COL
    s.agg_arg[0][0] = 1
    buf = C.create_string_buffer(64)
    assert L.lib.nut_groupby_jit_source(C.byref(s), buf, 64, None) == 1  # validate() runs first
    msg = L.lib.nut_last_error().decode()
    assert "value column 1" in msg and "prog_mode" in msg
    p = L.NutAggSpec()
    p.n = 4
    p.npred = 1
    p.pred_col[0] = 64  # never read: the spec is rejected
    p.pred_type[0] = code
    p.pred_op[0] = L.LT
    assert L.lib.nut_groupby_jit_source(C.byref(p), buf, 64, None) == 1
    assert "predicate column 0" in L.lib.nut_last_error().decode()


def test_fused_python_query_keeps_raising():
    for dt, _ in NARROW:
        q = AggQuery(keys=[], values=[FakeCol(dt)], aggs=[Agg("sum", "col", (0,))])
        with pytest.raises(TypeError):
            q.to_spec(None)
        q = AggQuery(keys=[], aggs=[Agg("count")], preds=[(FakeCol(dt), "<", 3)])
        with pytest.raises(TypeError):
            q.to_spec(None)
        with pytest.raises((TypeError, ValueError)):
            ProgQuery(keys=[FakeCol(dt)], cols=[], aggs=[("count", None, None)]).to_spec(None)


def test_gather_typed_argument_checks_without_a_device():
    """argument checks come before any device work: a NULL context, and an unknown column
    type (NUT_T_STR, 10) with a context pointer that is never read"""
    assert L.lib.nut_gather_typed(None, None, L.T_I32, None, 0, 0, None) == 1
    assert b"NULL" in L.lib.nut_last_error()
    for code in (L.T_STR, 10, -1):
        assert L.lib.nut_gather_typed(C.c_void_p(64), None, code, None, 0, 0, None) == 1
        assert b"unknown column type" in L.lib.nut_last_error()


def test_select_and_eval_reject_string_typed_columns():
    """NUT_T_STR is no program column type for the scan and projection kernels either"""
    s = mixed_spec([L.T_I64, L.T_F64])
    s.naggs = 3
    s.prog_col_type[0] = L.T_STR
    for fn in (L.lib.nut_select_jit_compile, L.lib.nut_eval_jit_compile, L.lib.nut_groupby_jit_compile):
        assert fn(C.byref(s)) == 1
        assert b"unknown type 2" in L.lib.nut_last_error() or b"bad program column type" in L.lib.nut_last_error()


# ------------------------------------------------------------------ plans (nut_plan_route)
from test_plan_route_cpu import GROUPS, SCANS, SORTS  # noqa: E402  (the shapes, unchanged)
from nutdb_amd.sql import Plan  # noqa: E402

NARROW_PAIRS = [("int32", "int64"), ("int64", "int32"), ("int32", "int32"), ("float32", "int64"),
                ("int64", "float32"), ("float32", "float32"), ("int32", "float32"), ("float32", "int32")]


@pytest.mark.parametrize("sql", SCANS + SORTS + GROUPS)
@pytest.mark.parametrize("tx,ty", NARROW_PAIRS)
def test_narrow_plans_route_and_never_fused(sql, tx, ty):
    """every single-table shape routes over int32 / float32 columns, and a plan that binds a
    narrow column takes no fused route (only the generated kernels read narrow bytes)"""
    cols = Plan(sql).describe()["columns"]
    r = Plan(sql).route({"x": tx, "y": ty})
    assert r, sql
    bound_narrow = cols == ["*"] or any({"x": tx, "y": ty}.get(c, "int64") != "int64" for c in cols) \
        or Plan(sql).describe().get("column") == "*"
    if bound_narrow:
        assert "fused-" not in r, (sql, tx, ty, r)


@pytest.mark.parametrize("sql", SORTS)
@pytest.mark.parametrize("tx,ty", NARROW_PAIRS)
def test_narrow_single_key_sorts(sql, tx, ty):
    """a single-key sort of a float32 key ends in expr-sort-f64-order, of an int32 key in
    expr-sort or the row-id scan"""
    r = Plan(sql).route({"x": tx, "y": ty})
    final = r.split(" -> ")[-1]
    ordered = {"x": tx, "y": ty}[sql.split("order by")[1].split()[0].rstrip(",")]
    if ordered == "float32":
        assert final in ("expr-sort-f64-order", "rowid-scan"), (sql, r)
        if final != "rowid-scan":
            assert final == "expr-sort-f64-order"
    elif ordered == "int32":
        assert final in ("expr-sort", "rowid-scan"), (sql, r)
    if final == "expr-sort":
        assert ordered in ("int32", "int64"), (sql, r)
    if final == "expr-sort-f64-order":
        assert ordered == "float32", (sql, r)


def test_narrow_route_names_and_prepare():
    assert Plan("select x from t order by x").route({"x": "float32"}) == "rerun-expression -> expr-sort-f64-order"
    assert Plan("select x from t order by x").route({"x": "int32"}) == "rerun-expression -> expr-sort"
    assert Plan("select x from t where x < 2").route({"x": "uint8"}) == "rerun-expression -> expr-filter"
    assert Plan("select y, sum(x) from t group by y").route({"x": "float32", "y": "int64"}) == "expr-groupby"
    assert Plan("select y, sum(x) from t group by y").route({"x": "int64", "y": "int16"}) == "packed-groupby"
    assert Plan("select y, sum(x) from t group by y").route({"x": "int8", "y": "float32"}) == \
        "expr-groupby (float64 key words)"
    for types in ({"x": "int32", "y": "float32"}, {"x": "uint16", "y": "int8"}):
        Plan("select y, sum(x * 2), min(x) from t where x > 1 group by y").prepare(types)
        Plan("select y, sum(x) from t where x > 1 group by y").prepare(types)  # a fused shape, compiled for narrow columns
        Plan("select x * 2, y from t where x + y > 1").prepare(types)
    with pytest.raises(KeyError):
        Plan("select x from t").route({"x": "int128"})


# ------------------------------------------------------------------ tables (nut_table_set_narrow)
SCHEMA = """CREATE TABLE lineitem (a Int8, b UInt16, c Float32, d Float64, e Boolean, f Date,
    g DateTime, h String, i Dictionary(String), j Enum('x' = 1, 'y' = 5), k Nullable(Int32), l Chars(4),
    m UInt64, n Int64, o Serial32, p USerial64)"""


def test_table_set_narrow_reports_narrow_exec_types():
    from nutdb_amd.table import Table
    wide = Table(None, SCHEMA)
    today = {"a": L.T_I64, "b": L.T_I64, "c": L.T_F64, "d": L.T_F64, "e": L.T_I64, "f": L.T_I64, "g": L.T_I64,
             "h": L.T_I64, "i": L.T_I64, "j": L.T_I64, "k": L.T_I64, "l": L.T_I64, "m": L.T_I64, "n": L.T_I64,
             "o": L.T_I64, "p": L.T_I64}
    assert wide.exec_types() == today  # without the call: today's answers
    t = Table(None, SCHEMA, narrow=True)
    want = dict(today, a=L.T_I8, b=L.T_U16, c=L.T_F32, e=L.T_U8, k=L.T_I32, o=L.T_I32)
    assert t.exec_types() == want
    assert t.columns == wide.columns  # kinds and host widths are untouched
    t.set_narrow(False)
    assert t.exec_types() == today
