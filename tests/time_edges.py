"""Edge operands of the calendar program ops (include/nutexec.h: TIMEPART, DATETRUNC,
ADDMONTHS and the REL_* parts of DATEPART; csrc/prog_ops.hpp: jtimepart, jdatetrunc,
jaddmonths, jdatepart), and an exact restatement of each in Python integers.

oracle/expr.py does not know these ops, so the restatement below is the reference:
tests/test_time_edges_cpu.py pins it against `datetime`, tests/test_gpu_time.py runs the ops
on the GPU against it.  Everything is bit-exact.  Python's // and % floor, which is what the
ops' fdiv / fmod are.

  DAYS     expr_edges.DAYS (122 day numbers)
  SECONDS  the granule edges, every in-calendar day x 4 times of day, the clamp, the ends
  MONTHS   (day, month count) pairs: month-end days x month steps, plus the day clamps
"""
import datetime


from expr_edges import DAYS, EPOCH, FIRST_DAY, IN_CALENDAR, LAST_DAY, MAX, MIN, i64

DAY_CLAMP, SEC_CLAMP, MONTH_CLAMP = 2**40, 2**40 * 86400, 2**36

# nut_time_part / nut_date_trunc / the new nut_date_part values
TP = ["DATE", "HOUR", "MINUTE", "SECOND", "START_MINUTE", "START_FIVE_MINUTES", "START_FIFTEEN_MINUTES", "START_HOUR",
      "START_DAY"]
DT = ["WEEK_MONDAY", "WEEK_SUNDAY", "MONTH", "QUARTER", "YEAR", "MONTH_END"]
REL_MONTH, REL_QUARTER, REL_WEEK = 8, 9, 10
GRANULE = {4: 60, 5: 300, 6: 900, 7: 3600, 8: 86400}


def clamp(x, m):
    return max(-m, min(m, x))


def wrap(x):
    return (x + 2**63) % 2**64 - 2**63


def leap(y):
    return (y % 4 == 0 and y % 100 != 0) or y % 400 == 0


def month_days(y, m):
    return 29 if m == 2 and leap(y) else [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31][m - 1]


def civil(d):
    """(year, month, day) of day number d, proleptic Gregorian, any integer d"""
    z = d + 719468
    era = z // 146097
    doe = z - era * 146097
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    m = mp + 3 if mp < 10 else mp - 9
    return yoe + era * 400 + (1 if m <= 2 else 0), m, doy - (153 * mp + 2) // 5 + 1


def days_of(y, m, d):
    """day number of a civil date, any integer year"""
    y -= 1 if m <= 2 else 0
    era = y // 400
    yoe = y - era * 400
    doy = (153 * (m - 3 if m > 2 else m + 9) + 2) // 5 + d - 1
    return era * 146097 + yoe * 365 + yoe // 4 - yoe // 100 + doy - 719468


def time_part(s, part):
    s = clamp(s, SEC_CLAMP)
    if part == 0:
        return s // 86400
    if part == 1:
        return s % 86400 // 3600
    if part == 2:
        return s % 3600 // 60
    if part == 3:
        return s % 60
    return s - s % GRANULE[part]


def date_trunc(d, unit):
    d = clamp(d, DAY_CLAMP)
    if unit == 0:
        return d - (d + 3) % 7
    if unit == 1:
        return d - (d + 4) % 7
    y, m, _ = civil(d)
    if unit == 2:
        return days_of(y, m, 1)
    if unit == 3:
        return days_of(y, (m - 1) // 3 * 3 + 1, 1)
    if unit == 4:
        return days_of(y, 1, 1)
    return days_of(y, m, month_days(y, m))


def add_months(d, n):
    d, n = clamp(d, DAY_CLAMP), clamp(n, MONTH_CLAMP)
    y, m, dd = civil(d)
    t = y * 12 + (m - 1) + n
    ny, nm = t // 12, t % 12 + 1
    return days_of(ny, nm, min(dd, month_days(ny, nm)))


def rel_part(d, part):
    d = clamp(d, DAY_CLAMP)
    if part == REL_WEEK:
        return (d + 3) // 7
    y, m, _ = civil(d)
    return y * 12 + m if part == REL_MONTH else y * 4 + (m - 1) // 3


def date_part(d, part):
    """all 11 nut_date_part values"""
    if part >= REL_MONTH:
        return rel_part(d, part)
    d = clamp(d, DAY_CLAMP)
    y, m, dd = civil(d)
    return [y, m, dd, (m - 1) // 3 + 1, (d + 3) % 7 + 1, d - days_of(y, 1, 1) + 1, y * 100 + m,
            y * 10000 + m * 100 + dd][part]


def date_diff(unit, a, b, a_datetime=False, b_datetime=False):
    """dateDiff(unit, a, b) = f(b) - f(a); for day and larger units a Datetime gives its day first"""
    def f(x, is_dt):
        if unit in ("second", "minute", "hour"):
            return x if unit == "second" else clamp(x, SEC_CLAMP) // (60 if unit == "minute" else 3600)
        d = time_part(x, 0) if is_dt else x
        return {"day": lambda: d, "week": lambda: rel_part(d, REL_WEEK), "month": lambda: rel_part(d, REL_MONTH),
                "quarter": lambda: rel_part(d, REL_QUARTER), "year": lambda: date_part(d, 0)}[unit]()
    return wrap(f(b, b_datetime) - f(a, a_datetime))


# ------------------------------------------------------------------ operands
CAL_DAYS = [d for d, c in zip(DAYS, IN_CALENDAR) if c]


def _seconds():
    out = [0]
    for g in (1, 59, 60, 61, 299, 300, 899, 900, 3599, 3600, 86399, 86400, 86401):
        out += [g, -g]
    for d in CAL_DAYS:
        out += [d * 86400 + t for t in (0, 1, 43199, 86399)]
    out += [SEC_CLAMP, -SEC_CLAMP, SEC_CLAMP + 1, SEC_CLAMP - 1, -SEC_CLAMP + 1, -SEC_CLAMP - 1, MIN, MAX]
    return list(dict.fromkeys(out))


SECONDS = _seconds()
SEC_IN_CALENDAR = [FIRST_DAY * 86400 <= s < (LAST_DAY + 1) * 86400 for s in SECONDS]
STEPS = [0, 1, -1, 11, -11, 12, -12, 13, -13, 1200, -1200, 2**36, -2**36, 2**36 + 1, -2**36 - 1, MIN, MAX]
STEP_YEARS = [2024, 2023, 1900, 2000, 1, 9999]  # leap, not leap, century not leap, century leap, the calendar's ends


def _months():
    days = []
    for y in STEP_YEARS:
        md = [(1, 29), (1, 30), (1, 31), (2, 28), (3, 31), (12, 31), (1, 1)]
        if leap(y):
            md.insert(4, (2, 29))
        days += [datetime.date(y, m, d).toordinal() - EPOCH for m, d in md]
    days += [DAY_CLAMP, -DAY_CLAMP, DAY_CLAMP + 1, DAY_CLAMP - 1, -DAY_CLAMP + 1, -DAY_CLAMP - 1, MIN, MAX]
    return i64([d for d in days for _ in STEPS]), i64([n for _ in days for n in STEPS])


MONTHS = _months()


def month_step_in_calendar(d, n):
    """d, and d plus n months, are dates `datetime` has (years 1 to 9999)"""
    return FIRST_DAY <= d <= LAST_DAY and abs(n) <= 10**6 and FIRST_DAY <= add_months(d, n) <= LAST_DAY


# the tail lanes of a wavefront run: no row count is a multiple of 64
assert len(DAYS) % 64 and len(SECONDS) % 64 and len(MONTHS[0]) % 64

# ------------------------------------------------------------------ programs (nut_eval_rows specs, <= 8 each)
C0, C1 = [("col", 0)], [("col", 1)]
EVAL_SPECS = {
    "timepart_a": ("SECONDS", [C0 + [("timepart", p)] for p in range(5)]),
    "timepart_b": ("SECONDS", [C0 + [("timepart", p)] for p in range(5, 9)]),
    "datetrunc": ("DAYS", [C0 + [("datetrunc", u)] for u in range(6)]),
    "rel": ("DAYS", [C0 + [("datepart", p)] for p in (REL_MONTH, REL_QUARTER, REL_WEEK)]),
    "addmonths": ("MONTHS", [C0 + C1 + [("addmonths",)]]),
}
EVAL_WANT = {
    "timepart_a": lambda s: [time_part(s, p) for p in range(5)],
    "timepart_b": lambda s: [time_part(s, p) for p in range(5, 9)],
    "datetrunc": lambda d: [date_trunc(d, u) for u in range(6)],
    "rel": lambda d: [rel_part(d, p) for p in (REL_MONTH, REL_QUARTER, REL_WEEK)],
    "addmonths": lambda d, n: [add_months(d, n)],
}


def operands(name):
    return {"SECONDS": (i64(SECONDS),), "DAYS": (i64(DAYS),), "MONTHS": MONTHS}[name]


# toHour(s) = 23 and toDayOfWeek(toDate(s)) = 7: the last hour of a Sunday
SELECT_WHERE = (C0 + [("timepart", 1), ("i64", 0, 23), ("eq",)] +
                C0 + [("timepart", 0), ("datepart", 4), ("i64", 0, 7), ("eq",), ("and",)])


def select_want():
    return [i for i, s in enumerate(SECONDS) if time_part(s, 1) == 23 and date_part(time_part(s, 0), 4) == 7]


# computed GROUP BY keys
KEY_SPECS = {
    "start_hour": ("SECONDS", [C0 + [("timepart", 7)]]),
    "month_week": ("DAYS", [C0 + [("datetrunc", 2)], C0 + [("datepart", REL_WEEK)]]),
}
KEY_WANT = {
    "start_hour": lambda s: (time_part(s, 7),),
    "month_week": lambda d: (date_trunc(d, 2), rel_part(d, REL_WEEK)),
}

# ------------------------------------------------------------------ known answers (the issue's table)
D = lambda y, m, d: datetime.date(y, m, d).toordinal() - EPOCH  # noqa: E731
KNOWN = [
    (date_trunc(D(2024, 2, 29), 2), 19754), (date_trunc(D(2024, 2, 29), 3), 19723), (date_trunc(D(2024, 2, 29), 0), 19779),
    (date_trunc(D(2024, 2, 29), 1), 19778), (add_months(D(2024, 1, 31), 1), 19782), (add_months(D(2023, 1, 31), 1), 19416),
    (add_months(D(2024, 3, 31), -1), 19782), (add_months(D(2024, 2, 29), 12), 20147),
    (tuple(time_part(-1, p) for p in range(4)), (-1, 23, 59, 59)), (time_part(-1, 7), -3600),
    (tuple(time_part(1709214425, p) for p in (1, 2, 3)), (13, 47, 5)), (time_part(1709214425, 7), 1709211600),
    (time_part(1709214425, 8), 1709164800), (date_diff("month", D(2023, 12, 31), D(2024, 1, 1)), 1),
    (tuple(rel_part(d, REL_WEEK) for d in (-4, -3, 3, 4)), (-1, 0, 0, 1)),
]
# the same answers as SQL constants (Plan.describe folds them): (expression, value)
FOLDS = [
    ("toStartOfMonth(toDate('2024-02-29'))", 19754), ("toStartOfQuarter(toDate('2024-02-29'))", 19723),
    ("toMonday(toDate('2024-02-29'))", 19779), ("toStartOfWeek(toDate('2024-02-29'), 0)", 19778),
    ("toStartOfWeek(toDate('2024-02-29'))", 19778), ("toStartOfWeek(toDate('2024-02-29'), 1)", 19779),
    ("toStartOfYear(toDate('2024-02-29'))", D(2024, 1, 1)), ("toLastDayOfMonth(toDate('2024-02-01'))", 19782),
    ("addMonths(toDate('2024-01-31'), 1)", 19782), ("addMonths(toDate('2023-01-31'), 1)", 19416),
    ("subtractMonths(toDate('2024-03-31'), 1)", 19782), ("addMonths(toDate('2024-02-29'), 12)", 20147),
    ("addYears(toDate('2024-02-29'), 1)", 20147), ("addQuarters(toDate('2024-01-31'), 1)", D(2024, 4, 30)),
    ("addDays(toDate('2024-02-29'), 1)", 19783), ("addWeeks(toDate('2024-02-29'), -1)", 19775),
    ("subtractDays(toDate('2024-02-29'), 29)", 19753), ("subtractWeeks(toDate('2024-02-29'), 1)", 19775),
    ("subtractQuarters(toDate('2024-05-31'), 1)", 19782), ("subtractYears(toDate('2024-02-29'), 1)", D(2023, 2, 28)),
    ("toDate(-1)", -1), ("toHour(-1)", 23), ("toMinute(-1)", 59), ("toSecond(-1)", 59), ("toStartOfHour(-1)", -3600),
    ("toDateTime('2024-02-29 13:47:05')", 1709214425), ("toHour(toDateTime('2024-02-29 13:47:05'))", 13),
    ("toMinute(1709214425)", 47), ("toSecond(1709214425)", 5), ("toStartOfHour(1709214425)", 1709211600),
    ("toStartOfDay(1709214425)", 1709164800), ("toStartOfMinute(1709214425)", 1709214420),
    ("toStartOfFiveMinutes(1709214425)", 1709214300), ("toStartOfFifteenMinutes(1709214425)", 1709214300),
    ("toDate(toDateTime('2024-02-29 13:47:05'))", 19782), ("toYear(toDateTime('2024-02-29 13:47:05'))", 2024),
    ("toStartOfMonth(toDateTime('2024-02-29 13:47:05'))", 19754), ("toDate(toDate('2024-02-29'))", 19782),
    ("addSeconds(toDateTime('2024-02-29 13:47:05'), 55)", 1709214480), ("addMinutes(1709214425, 13)", 1709215205),
    ("addHours(toDateTime('2024-02-29 13:47:05'), -14)", 1709164025),
    ("subtractSeconds(1709214425, 5)", 1709214420), ("subtractMinutes(1709214425, 47)", 1709211605),
    ("subtractHours(1709214425, 13)", 1709167625),
    ("addMonths(toDateTime('2024-01-31 13:47:05'), 1)", 1709214425),
    ("toDateTime('2024-01-31 13:47:05') + interval 1 month", 1709214425),
    ("toDateTime('2024-02-29 13:47:05') + interval 13 minute", 1709215205),
    ("toDateTime('2024-02-29 13:47:05') - interval 1 day", 1709214425 - 86400),
    ("toDate('2024-01-31') + interval 1 month", 19782),
    ("dateDiff('month', toDate('2023-12-31'), toDate('2024-01-01'))", 1),
    ("dateDiff('year', toDate('2023-12-31'), toDate('2024-01-01'))", 1),
    ("dateDiff('quarter', toDate('2023-12-31'), toDate('2024-01-01'))", 1),
    ("dateDiff('week', toDate('2024-02-25'), toDate('2024-02-26'))", 1),  # Sunday -> Monday
    ("dateDiff('day', toDate('2024-02-29'), toDateTime('2024-03-01 00:00:00'))", 1),
    ("dateDiff('hour', toDateTime('2024-02-29 13:59:59'), toDateTime('2024-02-29 14:00:00'))", 1),
    ("dateDiff('minute', -1, 0)", 1), ("dateDiff('second', -1, 1)", 2),
    ("toRelativeMonthNum(toDate('2024-02-29'))", 2024 * 12 + 2), ("toRelativeQuarterNum(toDate('2024-02-29'))", 2024 * 4),
    ("toRelativeWeekNum(-4)", -1), ("toRelativeWeekNum(4)", 1),
]

# every new SQL name over columns: (SQL item, what describe() shows for it); ts is a Datetime
# column, d a Date column, v an int64
NAMES = [
    ("toHour(ts)", "toHour(ts)"), ("getHour(ts)", "toHour(ts)"), ("toMinute(ts)", "toMinute(ts)"),
    ("getMinute(ts)", "toMinute(ts)"), ("toSecond(ts)", "toSecond(ts)"), ("getSecond(ts)", "toSecond(ts)"),
    ("toRelativeMonthNum(d)", "toRelativeMonthNum(d)"), ("toRelativeQuarterNum(d)", "toRelativeQuarterNum(d)"),
    ("toRelativeWeekNum(d)", "toRelativeWeekNum(d)"), ("TOSTARTOFMINUTE(ts)", "toStartOfMinute(ts)"),
    ("toStartOfFiveMinutes(ts)", "toStartOfFiveMinutes(ts)"), ("toStartOfFifteenMinutes(ts)", "toStartOfFifteenMinutes(ts)"),
    ("toStartOfHour(ts)", "toStartOfHour(ts)"), ("toStartOfDay(ts)", "toStartOfDay(ts)"), ("toMonday(d)", "toMonday(d)"),
    ("toStartOfWeek(d)", "toStartOfWeek(d, 0)"), ("toStartOfWeek(d, 0)", "toStartOfWeek(d, 0)"),
    ("toStartOfWeek(d, 1)", "toMonday(d)"), ("toStartOfMonth(d)", "toStartOfMonth(d)"),
    ("toStartOfQuarter(d)", "toStartOfQuarter(d)"), ("toStartOfYear(ts)", "toStartOfYear(ts)"),
    ("toLastDayOfMonth(d)", "toLastDayOfMonth(d)"), ("toDate(ts)", "toDate(ts)"),
    ("addSeconds(ts, v)", "addSeconds(ts, v)"), ("addMinutes(ts, v)", "addMinutes(ts, v)"),
    ("addHours(ts, v)", "addHours(ts, v)"), ("addDays(d, v)", "addDays(d, v)"), ("addWeeks(d, v)", "addWeeks(d, v)"),
    ("addMonths(d, v)", "addMonths(d, v)"), ("addQuarters(d, v)", "addQuarters(d, v)"), ("addYears(ts, v)", "addYears(ts, v)"),
    ("subtractSeconds(ts, v)", "addSeconds(ts, (0 - v))"), ("subtractMinutes(ts, v)", "addMinutes(ts, (0 - v))"),
    ("subtractHours(ts, v)", "addHours(ts, (0 - v))"), ("subtractDays(d, v)", "addDays(d, (0 - v))"),
    ("subtractWeeks(d, v)", "addWeeks(d, (0 - v))"), ("subtractMonths(d, v)", "addMonths(d, (0 - v))"),
    ("subtractQuarters(d, v)", "addQuarters(d, (0 - v))"), ("subtractYears(d, v)", "addYears(d, (0 - v))"),
    ("d + interval 1 month", "addMonths(d, 1)"), ("d - interval 2 year", "addYears(d, -2)"),
    ("ts + interval 5 minute", "addMinutes(ts, 5)"), ("ts - interval 1 day", "addDays(ts, -1)"),
    ("dateDiff('month', d, toDate(ts))", "(toRelativeMonthNum(toDate(ts)) - toRelativeMonthNum(d))"),
    ("dateDiff('second', ts, v)", "(v - ts)"), ("dateDiff('day', d, ts)", "(ts - d)"),
    ("dateDiff('hour', ts, v)", "(((toDate(v) * 24) + toHour(v)) - ((toDate(ts) * 24) + toHour(ts)))"),
    ("dateDiff('year', d, ts)", "(toYear(ts) - toYear(d))"),
]
NAME_TYPES = {"ts": "datetime", "d": "date", "v": "int64"}
