"""CPU: the exact restatement of the calendar ops (tests/time_edges.py) against `datetime`, the
known answers, nut_prog_type over the new ops, every kernel tests/test_gpu_time.py runs
compiled here with hipRTC (no GPU needed), constant folding on the host (the same functions,
csrc/prog_ops.hpp), the temporal kinds at binding, and every new SQL name."""
import calendar
import ctypes as C
import datetime
import json

import numpy as np
import pytest

import time_edges as T
from expr_edges import EPOCH, MAX, MIN
from nutdb_amd import _lib as L
from nutdb_amd import NutError, ProgQuery
from nutdb_amd.executor import _prog
from nutdb_amd.sql import Plan
from test_expr_edges_cpu import FakeCol, compile_

E0 = datetime.datetime(1970, 1, 1)


def day_of(date):
    return date.toordinal() - EPOCH


def check_day(d):
    """every day op of in-calendar day d against datetime; returns the cells compared"""
    x = datetime.date.fromordinal(d + EPOCH)
    assert T.civil(d) == (x.year, x.month, x.day) and T.days_of(x.year, x.month, x.day) == d
    assert [T.date_part(d, p) for p in range(8)] == [
        x.year, x.month, x.day, (x.month - 1) // 3 + 1, x.isoweekday(), x.timetuple().tm_yday,
        x.year * 100 + x.month, x.year * 10000 + x.month * 100 + x.day]
    last = T.month_days(x.year, x.month)
    assert last == calendar.monthrange(x.year, x.month)[1]
    want = [d - x.weekday(), d - x.isoweekday() % 7, day_of(x.replace(day=1)),
            day_of(x.replace(month=(x.month - 1) // 3 * 3 + 1, day=1)), day_of(x.replace(month=1, day=1)),
            day_of(x.replace(day=last))]
    assert [T.date_trunc(d, u) for u in range(6)] == want
    assert T.rel_part(d, T.REL_MONTH) == x.year * 12 + x.month
    assert T.rel_part(d, T.REL_QUARTER) == x.year * 4 + (x.month - 1) // 3
    # weeks start on Monday: the Monday of d's week is a whole number of weeks from Monday 1969-12-29 (day -3)
    assert (want[0] + 3) % 7 == 0 and T.rel_part(d, T.REL_WEEK) == (want[0] + 3) // 7
    return 8 + 6 + 3


def test_restatement_month_ends_years_1_to_9999():
    cells = 0
    for y in range(1, 10000):
        for m in range(1, 13):
            first = day_of(datetime.date(y, m, 1))
            cells += check_day(first) + check_day(first + T.month_days(y, m) - 1)
    assert cells == 9999 * 12 * 2 * 17


def test_restatement_every_day_1968_to_2032():
    a, b = day_of(datetime.date(1968, 1, 1)), day_of(datetime.date(2032, 12, 31))
    assert sum(check_day(d) for d in range(a, b + 1)) == (b - a + 1) * 17 and b - a + 1 == 23742


def test_restatement_add_months():
    """against datetime: the month arithmetic by hand, the day clamped by datetime's own month ends"""
    rng = np.random.default_rng(12)
    n = 0
    for d, k in zip(rng.integers(day_of(datetime.date(1000, 1, 1)), day_of(datetime.date(9000, 1, 1)), 5000).tolist(),
                    rng.integers(-12000, 12000, 5000).tolist()):
        x = datetime.date.fromordinal(d + EPOCH)
        t = x.year * 12 + x.month - 1 + k
        y, m = divmod(t, 12)
        nxt = datetime.date(y + (m == 11), (m + 1) % 12 + 1, 1)  # the first of the month after the target
        last = (nxt - datetime.timedelta(days=1)).day
        assert T.add_months(d, k) == day_of(datetime.date(y, m + 1, min(x.day, last)))
        n += 1
    assert n == 5000


def test_restatement_random_seconds():
    rng = np.random.default_rng(10**4)
    lo, hi = day_of(datetime.date(1, 1, 1)) * 86400, (day_of(datetime.date(9999, 12, 31)) + 1) * 86400
    secs = rng.integers(lo, hi, 10**4).tolist()
    for s in secs:
        x = E0 + datetime.timedelta(seconds=s)
        assert [T.time_part(s, p) for p in range(4)] == [day_of(x.date()), x.hour, x.minute, x.second]
        for p, fl in ((4, x.replace(second=0)), (5, x.replace(minute=x.minute // 5 * 5, second=0)),
                      (6, x.replace(minute=x.minute // 15 * 15, second=0)), (7, x.replace(minute=0, second=0)),
                      (8, x.replace(hour=0, minute=0, second=0))):
            assert T.time_part(s, p) == (fl - E0) // datetime.timedelta(seconds=1)
    assert len(secs) == 10**4 and min(secs) < 0 < max(secs)


def test_known_answers():
    assert len(T.KNOWN) == 15
    for got, want in T.KNOWN:
        assert got == want


def test_clamps_restated():
    for fn, args in ((T.time_part, range(9)), (T.date_trunc, range(6)), (T.date_part, range(11))):
        c = T.SEC_CLAMP if fn is T.time_part else T.DAY_CLAMP
        for a in args:
            assert fn(MIN, a) == fn(-c - 1, a) == fn(-c, a) and fn(MAX, a) == fn(c + 1, a) == fn(c, a)
    assert T.add_months(MIN, MIN) == T.add_months(-T.DAY_CLAMP, -T.MONTH_CLAMP)
    assert T.add_months(MAX, MAX) == T.add_months(T.DAY_CLAMP, T.MONTH_CLAMP) < 2**63
    assert T.add_months(0, T.MONTH_CLAMP - 1) != T.add_months(0, T.MONTH_CLAMP) == T.add_months(0, MAX)


def test_operand_sets():
    assert (len(T.DAYS), len(T.SECONDS), len(T.MONTHS[0])) == (122, 473, 884)
    assert all(n % 64 for n in (122, 473, 884))
    s = set(T.SECONDS)
    assert {0, MIN, MAX, T.SEC_CLAMP, -T.SEC_CLAMP - 1, 86399, -86401, 899, -300} <= s
    assert sum(T.SEC_IN_CALENDAR) == 465 and len(T.CAL_DAYS) == 111
    assert set(T.STEPS) >= {0, 13, -1200, 2**36 + 1, MIN, MAX}


# ------------------------------------------------------------------ nut_prog_type
def prog_type(nodes, types=(L.T_I64, L.T_I64)):
    keep = []
    pr = _prog(nodes, keep)
    ct = (C.c_int32 * L.NUT_MAX_PROG_COLS)(*types)
    t = C.c_int32(-1)
    st = L.lib.nut_prog_type(C.byref(pr), ct, len(types), C.byref(t))
    return st, t.value


def test_prog_type_accepts_every_op_and_arg():
    n = 0
    for op, args in (("timepart", range(9)), ("datetrunc", range(6)), ("datepart", range(11))):
        for a in args:
            assert prog_type(T.C0 + [(op, a)]) == (0, L.PT_I64), (op, a)
            n += 1
    assert prog_type(T.C0 + T.C1 + [("addmonths",)]) == (0, L.PT_I64) and n == 26
    assert (L.P["map"], L.P["timepart"], L.P["datetrunc"], L.P["addmonths"]) == (30, 31, 32, 33)
    assert (L.TP_START_DAY, L.DT_MONTH_END, L.DP_REL_MONTH, L.DP_REL_QUARTER, L.DP_REL_WEEK) == (8, 5, 8, 9, 10)
    assert L.lib.nut_abi_version() == 1


@pytest.mark.parametrize("op, bad", [("timepart", (-1, 9)), ("datetrunc", (-1, 6)), ("datepart", (-1, 11))])
def test_prog_type_rejects_unknown_arg_and_f64(op, bad):
    for a in bad:
        assert prog_type(T.C0 + [(op, a)])[0] != 0
        assert "unknown" in L.lib.nut_last_error().decode()
    assert prog_type(T.C0 + [(op, 0)], (L.T_F64,))[0] != 0
    assert "integer operand" in L.lib.nut_last_error().decode()


def test_prog_type_addmonths_rejects_f64_and_unknown_op():
    assert prog_type(T.C0 + T.C1 + [("addmonths",)], (L.T_I64, L.T_F64))[0] != 0
    assert prog_type(T.C0 + T.C1 + [("addmonths",)], (L.T_F64, L.T_I64))[0] != 0
    assert prog_type(T.C0 + [(34,)])[0] != 0 and "unknown program op" in L.lib.nut_last_error().decode()
    assert prog_type(T.C0 + [("addmonths",)])[0] != 0  # one operand: stack underflow


# ------------------------------------------------------------------ hipRTC: every kernel of the GPU file
def cols_for(name):
    return [FakeCol("i") for _ in T.operands(name)]


@pytest.mark.parametrize("name", sorted(T.EVAL_SPECS))
def test_eval_specs_compile(name):
    src, progs = T.EVAL_SPECS[name]
    assert 1 <= len(progs) <= 8
    compile_(L.lib.nut_eval_jit_compile, ProgQuery(keys=[], cols=cols_for(src), aggs=[("sum", v, None) for v in progs]))


def test_select_spec_compiles():
    compile_(L.lib.nut_select_jit_compile, ProgQuery(keys=[], cols=[FakeCol("i")], aggs=[], where=T.SELECT_WHERE))


@pytest.mark.parametrize("name", sorted(T.KEY_SPECS))
def test_groupby_specs_compile(name):
    src, keys = T.KEY_SPECS[name]
    q = ProgQuery(keys=keys, cols=[FakeCol("i"), FakeCol("i")], aggs=[("count", None, None), ("sum", T.C1, None)])
    compile_(L.lib.nut_groupby_jit_compile, q)


def test_every_op_compiles_through_all_three_generators():
    """one program that adds up every op and arg (a compile costs seconds: three in all)"""
    every = ([T.C0 + [("timepart", p)] for p in range(9)] + [T.C0 + [("datetrunc", u)] for u in range(6)] +
             [T.C0 + [("datepart", p)] for p in (8, 9, 10)] + [T.C0 + T.C1 + [("addmonths",)]])
    total = every[0]
    for v in every[1:]:
        total = total + v + [("add",)]
    assert len(every) == 19 and len(total) < L.NUT_MAX_PROG_NODES
    cols = [FakeCol("i"), FakeCol("i")]
    pos = total + [("i64", 0, 0), ("ge",)]
    compile_(L.lib.nut_eval_jit_compile, ProgQuery(keys=[], cols=cols, aggs=[("sum", total, pos)]))
    compile_(L.lib.nut_groupby_jit_compile, ProgQuery(keys=[total], cols=cols, where=pos, aggs=[("max", total, pos)]))
    compile_(L.lib.nut_select_jit_compile, ProgQuery(keys=[], cols=cols, aggs=[], where=pos))


# ------------------------------------------------------------------ constant folding
def test_constants_fold_to_the_known_answers():
    assert len(T.FOLDS) >= 55
    for sql, want in T.FOLDS:
        d = Plan(f"select {sql} as x, a from t").describe()
        assert d["project"][0] == str(want), sql


def test_where_expr_shows_the_folded_constant():
    d = Plan("select a from t where a % 2 = 0 and d < addMonths(toDate('2024-01-31'), 1)").describe()
    assert "19782" in json.dumps(d) and "addMonths" not in json.dumps(d)
    d = Plan("select a from t where ts >= toStartOfHour(toDateTime('2024-02-29 13:47:05'))").describe()
    assert "1709211600" in json.dumps(d)


@pytest.mark.parametrize("lit", ["2024-02-30 00:00:00", "2024-02-29 24:00:00", "2024-02-29 23:60:00", "2024-02-29 23:59:60",
                                 "2024-02-29", "2024-02-29 1:00:00", "2024-13-01 00:00:00"])
def test_bad_datetime_literal_is_a_plan_error(lit):
    with pytest.raises(NutError, match="toDateTime") as e:
        Plan(f"select a from t where ts < toDateTime('{lit}')")
    assert e.value.status == 7


def test_time_function_of_a_date_constant_is_a_plan_error():
    for sql in ("toHour(toDate('2024-02-29'))", "addHours(toDate('2024-02-29'), 1)",
                "dateDiff('hour', toDate('2024-02-29'), 5)", "toDate('2024-02-29') + interval 1 hour"):
        with pytest.raises(NutError):
            Plan(f"select {sql} as x, a from t")
    with pytest.raises(NutError, match="toStartOfWeek"):
        Plan("select toStartOfWeek(d, 2) from t")
    with pytest.raises(NutError, match="dateDiff"):
        Plan("select dateDiff('fortnight', d, d) from t")


# ------------------------------------------------------------------ kinds at binding
def test_day_function_prepares_over_every_kind():
    p = Plan("select toYear(ts) as y, count() from t group by y")
    for kind in ("datetime", "date", "int64"):
        p.prepare({"ts": kind})
        assert p.route({"ts": kind}) == "packed-groupby"


def test_time_function_over_a_date_is_a_plan_error_naming_it():
    """(route resolves a group-by's key programs, prepare a scan's and an aggregate's arguments)"""
    for sql, how in (("select toHour(d) as h, count() from t group by h", "route"),
                     ("select sum(toHour(d)) from t", "prepare"), ("select sum(toHour(d)) from t", "route"),
                     ("select a from t where toStartOfHour(d) > 5", "prepare"),
                     ("select toMinute(toStartOfMonth(d)) from t", "prepare"),
                     ("select dateDiff('minute', d, a) from t", "prepare"), ("select addSeconds(d, a) from t", "prepare")):
        p = Plan(sql)
        with pytest.raises(NutError, match=r"\bd\b") as e:
            getattr(p, how)({"d": "date", "a": "int64"})
        assert e.value.status == 7, sql
        if "toStartOfMonth" not in sql:  # (that one is a Date whatever d is)
            getattr(p, how)({"d": "int64", "a": "int64"})  # a plain integer reads as seconds


def test_interval_below_a_day_needs_a_datetime():
    p = Plan("select d + interval 1 hour from t")
    for kind in ("date", "int64"):
        with pytest.raises(NutError, match="below a day") as e:
            p.prepare({"d": kind})
        assert e.value.status == 7
    p.prepare({"d": "datetime"})
    Plan("select d + interval 1 month, d - interval 3 day from t").prepare({"d": "date"})


def test_kind_flags_need_int64():
    arr = (L.NutColumn * 1)()
    arr[0].name, arr[0].data = b"d", None
    p = Plan("select toYear(d) from t")
    for bad in (L.T_F64 | L.NUT_COL_AS_DATE, L.T_I32 | L.NUT_COL_AS_DATETIME,
                L.T_I64 | L.NUT_COL_AS_DATE | L.NUT_COL_AS_DATETIME):
        arr[0].type = bad
        assert L.lib.nut_plan_prepare(p._handle(), arr, 1) == 1  # NUT_ERR_INVALID_ARG
    arr[0].type = L.T_I64 | L.NUT_COL_AS_DATE
    assert L.lib.nut_plan_prepare(p._handle(), arr, 1) == 0


def test_kinds_flow_through_if_and_truncations():
    types = {"ts": "datetime", "d": "date", "a": "int64"}
    Plan("select toHour(case when a > 0 then ts else toStartOfHour(ts) end) from t").prepare(types)
    Plan("select toHour(addDays(ts, a)) from t").prepare(types)
    for sql in ("toHour(case when a > 0 then d else toStartOfMonth(ts) end)", "toHour(addDays(d, a))", "toHour(toDate(ts))",
                "toHour(addMonths(a, 1))", "toHour(d + interval 1 month)"):
        with pytest.raises(NutError, match="Date"):
            Plan(f"select {sql} from t").prepare(types)


# ------------------------------------------------------------------ names
def test_every_new_name_lowers_and_is_described():
    """all of them as the projections of one plan: one describe, one prepare"""
    assert len(T.NAMES) >= 45
    p = Plan("select " + ", ".join(f"{sql} as x{i}" for i, (sql, _) in enumerate(T.NAMES)) + " from t")
    assert p.describe()["project"] == [shown for _, shown in T.NAMES]
    p.prepare(T.NAME_TYPES)


def test_truncation_is_a_select_alias_key():
    p = Plan("select toStartOfMonth(d) as m, count() from t group by m order by m")
    d = p.describe()
    assert d["kind"] == "groupby" and "toStartOfMonth(d)" in json.dumps(d)
    p.prepare({"d": "date"})
    assert p.route({"d": "datetime"}) == "packed-groupby"


def test_unknown_function_message_lists_the_new_names():
    with pytest.raises(NutError, match="toStartOfMinute") as e:
        Plan("select toStartOfSecond(ts) from t")
    assert "dateDiff" in str(e.value) and "toStartOfSecond" in str(e.value)
