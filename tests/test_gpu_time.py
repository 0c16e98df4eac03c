"""GPU: the calendar program ops (TIMEPART, DATETRUNC, ADDMONTHS, the REL_* parts of DATEPART:
csrc/jit.cpp jtimepart, jdatetrunc, jaddmonths, jdatepart) and the SQL built on them, on the
edge operands of tests/time_edges.py.  The reference is that file's exact restatement in
Python integers, which tests/test_time_edges_cpu.py holds to `datetime`; the in-calendar rows
are compared with `datetime` here as well.  Everything is bit-exact; every test asserts how
many cells it compared.  Inputs are a few thousand rows (the SQL table: 20011): the cost is
the hipRTC compiles."""
import collections
import datetime
import math

import numpy as np
import pytest
import torch

import time_edges as T
from expr_edges import EPOCH, MAX, MIN, i64
from nutdb_amd import NutError, ProgQuery
from nutdb_amd.table import Table
from nutdb_amd.sql import Plan

pytestmark = pytest.mark.gpu

E0 = datetime.datetime(1970, 1, 1)


def dev(x, ex):
    return torch.from_numpy(np.ascontiguousarray(x)).to(ex.device)


def run_eval(ex, cols, progs):
    out, valid = ex.eval_rows([dev(c, ex) for c in cols], [(p, None) for p in progs])
    assert all(bool(v.all()) for v in valid)
    return np.stack([o.cpu().numpy() for o in out], axis=1)  # [rows, programs] int64


# ------------------------------------------------------------------ a. nut_eval_rows over the edge lists
@pytest.mark.parametrize("name", sorted(T.EVAL_SPECS))
def test_eval_edges(ex, name):
    src, progs = T.EVAL_SPECS[name]
    cols = T.operands(src)
    got = run_eval(ex, cols, progs)
    want = [T.EVAL_WANT[name](*[int(c[r]) for c in cols]) for r in range(len(cols[0]))]
    assert got.shape == (len(cols[0]), len(progs)) and got.shape[0] % 64 != 0
    assert got.tolist() == want, [(r, got[r].tolist(), want[r]) for r in range(len(want)) if got[r].tolist() != want[r]][:5]


def test_timepart_in_calendar_against_datetime(ex):
    secs = [s for s, c in zip(T.SECONDS, T.SEC_IN_CALENDAR) if c]
    got = run_eval(ex, [i64(secs)], [T.C0 + [("timepart", p)] for p in (0, 1, 2, 3, 7, 8)])
    want = []
    for s in secs:
        x = E0 + datetime.timedelta(seconds=s)
        want.append([x.toordinal() - EPOCH, x.hour, x.minute, x.second,
                     (x.replace(minute=0, second=0) - E0) // datetime.timedelta(seconds=1),
                     (x.toordinal() - EPOCH) * 86400])
    assert len(want) == 465 and got.tolist() == want


def test_datetrunc_and_addmonths_in_calendar_against_datetime(ex):
    got = run_eval(ex, [i64(T.CAL_DAYS)], [T.C0 + [("datetrunc", u)] for u in range(6)] +
                   [T.C0 + [("datepart", p)] for p in (T.REL_MONTH, T.REL_QUARTER)])
    want = []
    for d in T.CAL_DAYS:
        x = datetime.date.fromordinal(d + EPOCH)
        day = lambda y: y.toordinal() - EPOCH  # noqa: E731
        nxt = datetime.date(x.year + (x.month == 12), x.month % 12 + 1, 1) if (x.year, x.month) != (9999, 12) else None
        want.append([d - x.weekday(), d - x.isoweekday() % 7, day(x.replace(day=1)),
                     day(x.replace(month=(x.month - 1) // 3 * 3 + 1, day=1)), day(x.replace(month=1, day=1)),
                     day(nxt) - 1 if nxt else day(x.replace(day=31)), x.year * 12 + x.month,
                     x.year * 4 + (x.month - 1) // 3])
    assert len(want) == 111 and got.tolist() == want
    # one month on, inside the calendar: the day of month kept or clamped to the month's end
    d, n = T.MONTHS
    keep = [r for r in range(len(d)) if T.month_step_in_calendar(int(d[r]), int(n[r]))]
    got = run_eval(ex, [d[keep], n[keep]], [T.C0 + T.C1 + [("addmonths",)]])[:, 0]
    cells = 0
    for r, g in zip(keep, got.tolist()):
        x = datetime.date.fromordinal(int(d[r]) + EPOCH)
        y, m = divmod(x.year * 12 + x.month - 1 + int(n[r]), 12)
        last = (datetime.date(y + (m == 11), (m + 1) % 12 + 1, 1) - datetime.timedelta(days=1)).day if (y, m) != (9999, 11) else 31
        assert g == datetime.date(y, m + 1, min(x.day, last)).toordinal() - EPOCH, (x, int(n[r]))
        cells += 1
    assert cells == len(keep) >= 300


def test_clamp_plateaus(ex):
    """INT64_MIN / MAX give what the clamp gives; one step inside the clamp gives something else"""
    s = [MIN, -T.SEC_CLAMP - 1, -T.SEC_CLAMP, -T.SEC_CLAMP + 1, T.SEC_CLAMP - 1, T.SEC_CLAMP, T.SEC_CLAMP + 1, MAX]
    d = [MIN, -T.DAY_CLAMP - 1, -T.DAY_CLAMP, -T.DAY_CLAMP + 1, T.DAY_CLAMP - 1, T.DAY_CLAMP, T.DAY_CLAMP + 1, MAX]
    tp = run_eval(ex, [i64(s)], [T.C0 + [("timepart", p)] for p in (0, 3, 4, 8)]).tolist()
    dt = run_eval(ex, [i64(d)], [T.C0 + [("datetrunc", u)] for u in (0, 1, 2, 5)] +
                  [T.C0 + [("datepart", p)] for p in (8, 9, 10, 2)]).tolist()
    # (a truncation is the same for neighbouring days: the second and the day of month tell them apart)
    for rows in (tp, dt):
        assert rows[0] == rows[1] == rows[2] != rows[3] and rows[7] == rows[6] == rows[5] != rows[4]
    m = [MIN, -T.MONTH_CLAMP - 1, -T.MONTH_CLAMP, -T.MONTH_CLAMP + 1, T.MONTH_CLAMP - 1, T.MONTH_CLAMP, T.MONTH_CLAMP + 1, MAX]
    am = run_eval(ex, [i64([19782] * 8), i64(m)], [T.C0 + T.C1 + [("addmonths",)]])[:, 0].tolist()
    assert am[0] == am[1] == am[2] != am[3] and am[7] == am[6] == am[5] != am[4]
    am = run_eval(ex, [i64(d), i64([1] * 8)], [T.C0 + T.C1 + [("addmonths",)]])[:, 0].tolist()
    assert am[0] == am[1] == am[2] != am[3] and am[7] == am[6] == am[5] != am[4]


# ------------------------------------------------------------------ b. select, group-by
def test_select_rows_last_hour_of_a_sunday(ex):
    got = ex.select_rows([dev(i64(T.SECONDS), ex)], T.SELECT_WHERE).cpu().numpy()
    want = T.select_want()
    assert got.dtype == np.int64 and got.tolist() == want and 5 <= len(want) < len(T.SECONDS) // 4
    for r in want:  # (the clamp itself is no Sunday evening: every hit is a real instant)
        x = E0 + datetime.timedelta(seconds=T.SECONDS[r])
        assert x.hour == 23 and x.isoweekday() == 7


@pytest.mark.parametrize("hint", [4, 4096], ids=["private", "shared"])
@pytest.mark.parametrize("name", sorted(T.KEY_SPECS))
def test_groupby_computed_keys(ex, name, hint):
    """COUNT and an int64 SUM per computed key, over the edge list repeated to about 5000 rows,
    through the private-table kernel (a hint of at most 8 groups) and the shared-table one"""
    src, keys = T.KEY_SPECS[name]
    base = T.operands(src)[0]
    rows = 5003
    col = np.resize(base, rows)
    v = (np.arange(rows, dtype=np.int64) * 2654435761) % 2001 - 1000
    q = ProgQuery(keys=keys, cols=[dev(col, ex), dev(v, ex)], aggs=[("count", None, None), ("sum", T.C1, None)])
    gk, gw = ex.groupby(q, group_hint=hint).to_host_words()
    want = collections.defaultdict(lambda: [0, 0])
    for x, y in zip(col.tolist(), v.tolist()):
        acc = want[T.KEY_WANT[name](x)]
        acc[0] += 1
        acc[1] += y
    order = sorted(want)
    assert rows % 64 and len(order) > 100 and gk.shape == (len(order), len(keys))
    assert [tuple(k) for k in gk.tolist()] == order
    assert gw.view(np.int64).tolist() == [want[k] for k in order] and int(gw[:, 0].sum()) == rows


# ------------------------------------------------------------------ c. SQL over a typed table
N = 20011
Y0, Y1 = datetime.date(1960, 1, 1).toordinal() - EPOCH, datetime.date(2040, 12, 31).toordinal() - EPOCH


def _rows():
    """seeded: instants drawn from 600 hours (so groups repeat) and days from 500 days, 1960-2040"""
    rng = np.random.default_rng(20011)
    hours = rng.integers(Y0 * 24, (Y1 + 1) * 24, 600)
    ts = hours[rng.integers(0, 600, N)] * 3600 + rng.integers(0, 3600, N)
    d = rng.integers(Y0, Y1 + 1, 500)[rng.integers(0, 500, N)]
    v = rng.integers(-1000, 1001, N)
    return ts.astype(np.int64), d.astype(np.int64), v.astype(np.int64)


ROWS = _rows()


def tmod(a, b):
    return int(math.fmod(a, b))  # % truncates toward zero (include/nutexec.h)


def _want():
    """every query's exact answer, computed once"""
    ts, d, v = (c.tolist() for c in ROWS)
    w = {}
    hours = collections.defaultdict(lambda: [0, 0])
    ymh = collections.Counter()
    for s, x in zip(ts, v):
        a = hours[T.time_part(s, 7)]
        a[0] += 1
        a[1] += x
        t = E0 + datetime.timedelta(seconds=s)
        assert (t.year, t.month, t.hour) == (T.date_part(T.time_part(s, 0), 0), T.date_part(T.time_part(s, 0), 1),
                                             T.time_part(s, 1))
        ymh[(t.year, t.month, t.hour)] += 1
    w["hours"] = [[k, *hours[k]] for k in sorted(hours)]
    w["ymh"] = [[*k, ymh[k]] for k in sorted(ymh)]
    cut = datetime.date(2000, 3, 31).toordinal() - EPOCH
    months = collections.Counter(T.date_trunc(x, 2) for x in d if T.add_months(x, 1) < cut)
    w["months"] = [[k, months[k]] for k in sorted(months)]
    w["diff"] = [T.date_diff("month", x, s, b_datetime=True) for x, s in zip(d, ts)]
    w["diff_rows"] = [x for x, dd in zip(v, w["diff"]) if -2 <= dd <= 2]
    w["addm"] = [T.add_months(x, tmod(y, 25) - 12) for x, y in zip(d, v)]
    w["year"] = [T.date_part(T.time_part(s, 0), 0) for s in ts]
    w["hour"] = [T.time_part(s, 1) for s in ts]
    return w


QUERIES = {
    "hours": "select toStartOfHour(ts) as h, count() as c, sum(v) as s from t group by h order by h",
    "ymh": "select toYear(ts) as y, toMonth(ts) as m, toHour(ts) as hr, count() as c from t group by y, m, hr "
           "order by y, m, hr",
    "months": "select toStartOfMonth(d) as m, count() as c from t where d + interval 1 month < toDate('2000-03-31') "
              "group by m order by m",
    "diff": "select dateDiff('month', d, toDate(ts)) as dd from t",
    "diff_rows": "select v from t where dateDiff('month', d, toDate(ts)) between -2 and 2",
    "addm": "select addMonths(d, v % 25 - 12) as am from t",
}


@pytest.fixture(scope="module")
def want():
    return _want()


def table_of(ex, narrow=False):
    t = Table(ex, "CREATE TABLE t (ts Datetime, d Date, v Int64)", narrow=narrow)
    ts, d, v = ROWS
    # (numpy.datetime64 and ISO strings are accepted for Datetime columns; half of each here)
    half = N // 2
    t.append(ts=ts[:half].astype("datetime64[s]"), d=d[:half], v=v[:half])
    t.append(ts=[str(x) for x in ts[half:].astype("datetime64[s]")], d=[str(x) for x in d[half:].astype("datetime64[D]")],
             v=v[half:])
    return t


def rows_of(got):
    cols = [np.asarray(c).tolist() for c in got.values()]
    return [list(r) for r in zip(*cols)]


def check(got, name, want):
    w = want[name]
    if name in ("diff", "diff_rows", "addm"):
        (col,) = got.values()
        assert col.dtype == np.int64 and col.tolist() == w, name
    else:
        assert rows_of(got) == w, name
    return len(w)


@pytest.mark.parametrize("narrow", [False, True], ids=["wide", "narrow"])
def test_sql_typed_table(ex, want, narrow):
    t = table_of(ex, narrow)
    assert t.nrows == N and N % 64
    cells = sum(check(t.execute(Plan(sql)), name, want) for name, sql in QUERIES.items())
    assert cells == sum(len(want[k]) for k in QUERIES)
    assert len(want["hours"]) == 600 and len(want["months"]) > 50 and 0 < len(want["diff_rows"]) < N
    assert min(want["diff"]) < -300 and max(want["diff"]) > 300
    # the same through toDate: a Datetime's day, then the day function
    got = t.execute(Plan("select toYear(toDate(ts)) as y, toHour(ts) as h, toYYYYMM(ts) as ym, toDate(d) as dd from t"))
    assert got["y"].tolist() == want["year"] and got["h"].tolist() == want["hour"]
    assert got["ym"].tolist() == [T.date_part(T.time_part(int(s), 0), 6) for s in ROWS[0]]
    assert got["dd"].tolist() == ROWS[1].tolist()


def test_sql_raw_columns_with_declared_kinds(ex, want):
    ts, d, v = ROWS
    cols = {"ts": dev(ts, ex), "d": dev(d, ex), "v": dev(v, ex)}
    kinds = {"ts": "datetime", "d": "date"}
    for name, sql in QUERIES.items():
        check(Plan(sql).execute(ex, cols, types=kinds), name, want)
    # host-memory columns carry the kind as well
    check(Plan(QUERIES["hours"]).execute(ex, {"ts": ts, "d": d, "v": v}, types=kinds), "hours", want)
    # without the kinds a column is a plain integer: day functions read days, time functions seconds
    got = Plan("select toYear(toDate(ts)) as y, toHour(ts) as h, toYear(d) as yd from t").execute(ex, cols)
    assert got["y"].tolist() == want["year"] and got["h"].tolist() == want["hour"]
    assert got["yd"].tolist() == [T.date_part(int(x), 0) for x in d]
    plain = Plan("select toYear(ts) as y from t").execute(ex, cols)["y"].tolist()
    assert plain == [T.date_part(int(s), 0) for s in ts] != want["year"]
    with pytest.raises(ValueError):
        Plan(QUERIES["diff"]).execute(ex, cols, types={"ts": "timestamp"})


def test_errors_at_execution(ex):
    t = table_of(ex)
    with pytest.raises(NutError, match=r"toHour\(d\)") as e:
        t.execute(Plan("select toHour(d) as h, count() as c from t group by h"))
    assert e.value.status == 7
    with pytest.raises(NutError, match=r"toStartOfHour\(d\)") as e:
        t.execute(Plan("select v from t where toStartOfHour(d) > 0"))
    assert e.value.status == 7
    with pytest.raises(NutError, match="below a day") as e:
        t.execute(Plan("select d + interval 1 hour as x from t"))
    assert e.value.status == 7
    # error scoping is unchanged: a zero divisor next to a time function still fails the query
    with pytest.raises(NutError, match="division by zero"):
        t.execute(Plan("select toHour(ts) + intDiv(v, 0) as q from t"))
    got = t.execute(Plan("select toHour(ts) + intDiv(v, 1) as q from t"))
    assert got["q"].tolist() == [T.time_part(int(s), 1) + int(x) for s, x in zip(ROWS[0], ROWS[2])]
