"""Edge operands of the expression semantics (include/nutexec.h nut_prog; csrc/prog_ops.hpp:
jmod, jdiv, jshl, jshr, jabs, jdatepart; the jit.cpp prelude's jfmod; the int -> f64 conversions, the
constants passed as kernel arguments), and the programs that read them.

tests/test_expr_edges_cpu.py pins the numpy oracle (oracle/expr.py) on these operands against
exact arithmetic (Python integers, math.fmod, Python float comparison, datetime) and compiles
every spec below with hipRTC; tests/test_gpu_expr_edges.py runs the same specs on the GPU
against the oracle.  Everything is bit-exact: no tolerance appears anywhere.

  E      28 int64 values around every boundary the integer helpers have
  EE     all 784 ordered pairs of E, as two columns
  F      f64 partners of E in mixed comparisons; EF = E x F (1036 pairs)
  FA, FB f64 MOD operands; FAB = FA x FB (130 pairs, no NaN result, 21 results -0.0)
  DAYS   day numbers: calendar edges of 21 years, the DATEPART clamp, the era boundary
  FMA    triples whose a * b + c differs between two roundings and one (contraction)
  DIVP   4096 pairs whose quotients and products run from subnormal to near overflow
"""
import datetime
import math
from fractions import Fraction

import numpy as np

MIN, MAX = -2**63, 2**63 - 1

E = [MIN, MIN + 1, -2**62, -2**53 - 1, -2**53, -2**32, -2**31 - 1, -65, -64, -63, -2, -1, 0, 1, 2, 3, 7, 63, 64, 65,
     127, 2**31, 2**32, 2**53, 2**53 + 1, 2**62, MAX - 1, MAX]
assert len(E) == 28 and len(set(E)) == 28


def i64(xs):
    return np.array(xs, dtype=np.int64)


def f64(xs):
    return np.array(xs, dtype=np.float64)


def bits(x):
    """the 8-byte words of an int64 / float64 array, as uint64"""
    return np.ascontiguousarray(x).view(np.uint64)


EE = (i64([a for a in E for _ in E]), i64([b for _ in E for b in E]))
assert len(EE[0]) == 784

DBL_MAX, DBL_MIN, DENORM_MIN = 1.7976931348623157e308, 2.2250738585072014e-308, 5e-324
F = [float(e) for e in E] + [2.0**63, -2.0**63, 0.5, -0.5, -0.0, math.inf, -math.inf, math.nan, DENORM_MIN]
EF = (i64([e for e in E for _ in F]), f64([f for _ in E for f in F]))
assert len(EF[0]) == 1036

FA = [1e300, -1e300, DENORM_MIN, -DENORM_MIN, 6.0, -6.0, DBL_MAX, 2.0**53 + 2, 0.1, 0.0, -0.0, DBL_MIN, 1e-310]
FB = [3.0, -3.0, 0.1, DENORM_MIN, 1e-310, DBL_MIN, DBL_MAX, 7.0, math.inf, 1.0]
FAB = (f64([a for a in FA for _ in FB]), f64([b for _ in FA for b in FB]))
FAB_WANT = f64([math.fmod(a, b) for a, b in zip(*FAB)])  # C fmod: exact
assert len(FAB_WANT) == 130 and not np.isnan(FAB_WANT).any()
assert int(np.sum(bits(FAB_WANT) == 0x8000000000000000)) == 21

# ------------------------------------------------------------------ day numbers
EPOCH = datetime.date(1970, 1, 1).toordinal()
YEARS = [1, 4, 100, 400, 1582, 1600, 1700, 1800, 1899, 1900, 1901, 1969, 1970, 1972, 1999, 2000, 2001, 2038, 2100, 2400,
         9999]


def _days():
    out = []
    for y in YEARS:
        md = [(1, 1), (2, 28), (3, 1), (6, 30), (12, 31)]
        if (y % 4 == 0 and y % 100 != 0) or y % 400 == 0:
            md.insert(2, (2, 29))
        out += [datetime.date(y, m, d).toordinal() - EPOCH for m, d in md]
    out += [MIN, MAX, 2**40, -2**40, 2**40 + 1, 2**40 - 1, -2**40 + 1, -2**40 - 1, -719469, -719468, -719467, -1, 0]
    return list(dict.fromkeys(out))  # (-1 and 0 are 1969-12-31 and 1970-01-01 already)


DAYS = _days()
FIRST_DAY, LAST_DAY = datetime.date(1, 1, 1).toordinal() - EPOCH, datetime.date(9999, 12, 31).toordinal() - EPOCH
IN_CALENDAR = [FIRST_DAY <= d <= LAST_DAY for d in DAYS]
assert len(DAYS) == 122 and sum(IN_CALENDAR) == 111


def calendar_parts(day):
    """the 8 nut_date_part values of an in-calendar day number, from datetime"""
    x = datetime.date.fromordinal(day + EPOCH)
    return [x.year, x.month, x.day, (x.month - 1) // 3 + 1, x.isoweekday(), x.timetuple().tm_yday,
            x.year * 100 + x.month, x.year * 10000 + x.month * 100 + x.day]


# ------------------------------------------------------------------ a * b + c: one rounding or two
def _fma():
    """(a, b, c, twice-rounded a * b + c) where the fused result differs: float(Fraction) is
    correctly rounded, so both answers are exact rational arithmetic rounded once or twice."""
    rng = np.random.default_rng(53)
    cand = [(1 + 2.0**-30, 1 - 2.0**-30, -1.0)]
    for _ in range(200):
        a, b = (1.0 + float(rng.integers(1, 2**52)) * 2.0**-52 for _ in range(2))
        p = float(Fraction(a) * Fraction(b))
        cand += [(a, b, -p), (a, -b, p), (a, b, -1.0 - float(rng.integers(0, 4)))]
    keep = []
    for a, b, c in cand:
        exact = Fraction(a) * Fraction(b) + Fraction(c)
        twice = float(Fraction(float(Fraction(a) * Fraction(b))) + Fraction(c))
        if float(exact) != twice:
            keep.append((a, b, c, twice))
    return tuple(f64(col) for col in zip(*keep))


FMA = _fma()
assert len(FMA[0]) >= 64
with np.errstate(all="ignore"):
    assert np.array_equal(bits(FMA[0] * FMA[1] + FMA[2]), bits(FMA[3]))  # the host rounds twice


# ------------------------------------------------------------------ correctly rounded / and *
def _divp(n=4096):
    """full 52-bit mantissas; the exponents' sum and difference are uniform over
    [-1070, 1020], so a * b and a / b both run from subnormal to near overflow"""
    rng = np.random.default_rng(4096)
    ea = np.zeros(0, dtype=np.int64)
    eb = np.zeros(0, dtype=np.int64)
    while len(ea) < n:
        s, d = rng.integers(-1070, 1021, 4 * n), rng.integers(-1070, 1021, 4 * n)
        ok = ((s + d) % 2 == 0) & (np.abs((s + d) // 2) <= 1020) & (np.abs((s - d) // 2) <= 1020)
        ea, eb = np.concatenate([ea, (s + d)[ok] // 2]), np.concatenate([eb, (s - d)[ok] // 2])
    ea, eb = ea[:n], eb[:n]

    def man():
        return (1.0 + rng.integers(0, 2**52, n).astype(np.float64) * 2.0**-52) * rng.choice([-1.0, 1.0], n)
    return np.ldexp(man(), ea), np.ldexp(man(), eb)


DIVP = _divp()
with np.errstate(all="ignore"):
    for _r in (DIVP[0] / DIVP[1], DIVP[0] * DIVP[1]):
        assert len(_r) == 4096 and np.isfinite(_r).all() and (_r != 0).all()
        assert (np.abs(_r) < DBL_MIN).any() and (np.abs(_r) > 2.0**1000).any()

# ------------------------------------------------------------------ programs
C0, C1, C2 = [("col", 0)], [("col", 1)], [("col", 2)]
NZ = C1 + [("i64", 0, 0), ("ne",)]  # col1 != 0
INT_BIN = ["add", "sub", "mul", "shl", "shr", "bitand", "bitor", "bitxor"]
CMP = ["lt", "le", "gt", "ge", "eq", "ne"]
DIVS = ["mod", "intdiv"]


def K(k):
    return [("i64", 0, int(k))]


def bin_(op, a=C0, b=C1):
    return a + b + [(op,)]


# nut_eval_rows specs: name -> (column types, [(value program, mask program or None)]), at most
# 8 programs each.  "i" = int64, "f" = float64.  The *_k specs take their right operand from
# konst(k): the generated source does not depend on k.
def eval_specs(k=-1):
    return {
        "int_bin": ("ii", [(bin_(op), None) for op in INT_BIN]),
        "int_cmp_unary": ("ii", [(bin_(op), None) for op in CMP] + [(C0 + [("abs",)], None),
                                                                    (C0 + [("bitnot",)], None)]),
        "int_div_masked": ("ii", [(bin_(op), NZ) for op in DIVS]),
        "int_mod_bare": ("ii", [(bin_("mod"), None)]),
        "int_intdiv_bare": ("ii", [(bin_("intdiv"), None)]),
        "int_bin_k": ("i", [(bin_(op, b=K(k)), None) for op in INT_BIN]),
        "int_cmp_k": ("i", [(bin_(op, b=K(k)), None) for op in CMP]),
        "int_div_k": ("i", [(bin_(op, b=K(k)), None) for op in DIVS]),
        # int (col 0) against f64 (col 1): the int converts, round to nearest even
        "mixed_a": ("if", [(C0 + [("to_f64",)], None), (bin_("add"), None), (bin_("mul"), None),
                           (bin_("gt", b=K(0)) + C0 + C1 + [("if",)], None)] + [(bin_(op), None) for op in CMP[:4]]),
        "mixed_b": ("if", [(bin_("eq"), None), (bin_("ne"), None), (bin_("lt", C1, C0), None),
                           (bin_("ge", C1, C0), None), (bin_("sub", C1, C0), None),
                           (bin_("eq", C1, C1) + C1 + C0 + [("if",)], None)]),
        "int_div_f64": ("ii", [(bin_("div"), None)]),
        # f64 arithmetic over three f64 columns
        "f64_arith": ("fff", [(bin_("mod"), None), (bin_("mul") + C2 + [("add",)], None), (bin_("div"), None),
                              (bin_("mul"), None)]),
        "datepart": ("i", [(C0 + [("datepart", p)], None) for p in range(8)]),
    }


# nut_select_rows: where = (col0 OP col1) CMP k over EE; k chosen so that some rows pass and
# some do not (asserted where they run)
SELECT_SPECS = {
    "add_lt": ("ii", bin_("add") + K(-2**62) + [("lt",)]),
    "shr_eq": ("ii", bin_("shr") + K(-1) + [("eq",)]),
    "mul_ge": ("ii", bin_("mul") + K(2**62) + [("ge",)]),
    "moddiv_ne": ("ii", NZ + bin_("mod") + bin_("intdiv") + [("bitxor",)] + K(0) + [("if",)] + K(0) + [("ne",)]),
}

# nut_groupby over EE plus an f64 column (col 2) and a group column (col 3): int programs of
# eval_specs under SUM (wrapping) / COUNT / MIN / MAX, fmod and int + f64 under MIN and MAX,
# the divisions behind the aggregate mask col1 != 0
F0, F1 = C0 + [("to_f64",)], C1 + [("to_f64",)]
GROUPBY_AGGS = [
    ("sum", bin_("mul"), None), ("count", None, NZ), ("min", bin_("mod"), NZ), ("max", bin_("intdiv"), NZ),
    ("min", bin_("mod", F0, F1), NZ), ("max", bin_("mod", F0, F1), NZ),
    # (the mask drops the NaN rows of col 2, and no sum of a finite int and an f64 makes one)
    ("min", bin_("add", C0, C2), bin_("le", C0, C2)), ("max", bin_("add", C0, C2), bin_("le", C0, C2)),
]
# computed keys: abs(MIN) = MIN, 1 shl 63 = MIN and MIN intdiv 1 = MIN are the hash table's
# empty marker; -1 and MAX are keys too
KEY_SPECS = {
    "abs_shl": ([C0 + [("abs",)], bin_("shl")], None),
    "intdiv": ([bin_("intdiv")], NZ),
}
KEY_AGGS = [("count", None, None), ("sum", C1, None), ("min", C0, None), ("max", bin_("bitxor"), None)]

# ------------------------------------------------------------------ SQL
DATE_FNS = ["toYear", "toMonth", "toDayOfMonth", "toQuarter", "toDayOfWeek", "toDayOfYear", "toYYYYMM", "toYYYYMMDD"]
FOLD_DAYS = [-719469, -719468, 11016, 2**40 + 1]  # toYYYYMMDD(<literal>) folds on the host (const_eval calls prog_ops.hpp jdatepart)
A, FC, D = [("col", 0)], [("col", 1)], [("col", 2)]  # columns a (int64), f (float64), d (int64 days)
# (output name, SQL item, the program it lowers to)
SQL_ITEMS = [
    ("m1", "a % -1", A + K(-1) + [("mod",)]),
    ("d1", "intDiv(a, -1)", A + K(-1) + [("intdiv",)]),
    ("mo", "modulo(a, -1)", A + K(-1) + [("mod",)]),
    ("ab", "abs(a)", A + [("abs",)]),
    ("pm", "a + 9223372036854775807", A + K(MAX) + [("add",)]),
    ("tm", "a * -9223372036854775808", A + K(MIN) + [("mul",)]),
    ("l64", "a << 64", A + K(64) + [("shl",)]),
    ("r70", "a >> 70", A + K(70) + [("shr",)]),
    ("r63", "a >> 63", A + K(63) + [("shr",)]),
    ("q3", "a / 3", A + K(3) + [("div",)]),
    ("tf", "toFloat64(a)", A + [("to_f64",)]),
    ("fe", "f = 9007199254740993", FC + K(2**53 + 1) + [("eq",)]),
] + [(f"dp{p}", f"{fn}(d)", D + [("datepart", p)]) for p, fn in enumerate(DATE_FNS)]
SQL_EDGES = "select " + ", ".join(f"{sql} as {name}" for name, sql, _ in SQL_ITEMS) + \
    "".join(f", toYYYYMMDD({d}) as fold{i}" for i, d in enumerate(FOLD_DAYS)) + " from t"
SQL_TYPES = {"a": "int64", "f": "float64", "d": "int64"}

# ------------------------------------------------------------------ WHERE constants (resolve_i64)
BIG = "1" + "0" * 30 + ".0"  # 1e30: the tokenizer (the reference's) takes no exponent notation
WHERE_CONSTS = ["-9223372036854775809", "-9223372036854775808.5", "-9223372036854775808", "-9223372036854775807.5",
                "-3", "-2.5", "-0.5", "-0.0", "0.5", "2.5", "9007199254740992.5", "9223372036854775806.5",
                "9223372036854775807", "9223372036854775807.5", "9223372036854775808", BIG, "-" + BIG]
SQL_CMP = {"<": "lt", "<=": "le", ">": "gt", ">=": "ge", "=": "eq", "!=": "ne"}
MIRROR = {"<": ">", "<=": ">=", ">": "<", ">=": "<=", "=": "=", "!=": "!="}
BETWEENS = [("-2.5", "2.5"), ("-9223372036854775808.5", "-3"), ("0.5", "9223372036854775807.5"), ("-" + BIG, "-0.5"),
            ("9007199254740992.5", BIG), ("2.5", "-2.5"), ("-9223372036854775809", "9223372036854775808")]
# forced onto the compiled route by `and col % 1 = 0` (true for every int): a decimal constant
# is an f64 node, an integer constant inside int64 an i64 node
COMPILED_CONSTS = {"<": ["-2.5", "9007199254740992.5", "9223372036854775807.5", "-9223372036854775808.5", BIG],
                   ">=": ["-0.5", "0.5", "9223372036854775806.5", "-9223372036854775807.5", "-" + BIG],
                   "=": ["-0.0", "2.5", "9007199254740992.5", "9223372036854775807.5"],
                   "<=": ["-3", "9223372036854775807", "-9223372036854775808"],
                   "!=": ["-3", "9223372036854775807", "-9223372036854775808"]}


def exact_compare(v, op, const):
    """int v <op> the decimal constant `const`, in exact rational arithmetic"""
    k = Fraction(const)
    return {"<": v < k, "<=": v <= k, ">": v > k, ">=": v >= k, "=": v == k, "!=": v != k}[op]


def where_column():
    """4099 rows (more than one 4096-row tile) holding every value of E among random int64s"""
    rng = np.random.default_rng(4099)
    col = rng.integers(MIN, MAX, 4099, endpoint=True).astype(np.int64)
    col[rng.choice(4099, 512, replace=False)] = rng.integers(-4, 5, 512)
    col[rng.choice(4099, len(E), replace=False)] = E
    assert set(E) <= set(col.tolist())
    return col
