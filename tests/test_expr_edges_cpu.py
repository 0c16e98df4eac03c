"""CPU: the numpy expression oracle (oracle/expr.py) on the edge operands of
tests/expr_edges.py, against EXACT arithmetic rather than numpy — Python integers with
explicit wrap and truncation, math.fmod, Python float comparison, datetime — so that
tests/test_gpu_expr_edges.py may take the oracle as its reference; and every kernel that GPU
file runs, compiled here with hipRTC (no GPU needed), so a malformed spec shows before a GPU
does.  Every test asserts how many cells it compared."""
import ctypes as C

import numpy as np
import pytest
import torch

import expr_edges as X
from expr_edges import E, MAX, MIN, bits
from nutdb_amd import _lib as L
from nutdb_amd import NutError, ProgQuery
from nutdb_amd.sql import Plan
from oracle.expr import BOOL, F64, I64, date_part, eval_prog


def wrap(x):
    """two's-complement int64 of a Python integer"""
    return (x + 2**63) % 2**64 - 2**63


def tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def shl(a, b):
    return wrap(a << b) if 0 <= b < 64 else 0


def shr(a, b):
    return a >> b if 0 <= b < 64 else (-1 if a < 0 else 0)


EXACT = {
    "add": lambda a, b: wrap(a + b), "sub": lambda a, b: wrap(a - b), "mul": lambda a, b: wrap(a * b),
    "mod": lambda a, b: 0 if b == 0 else a - tdiv(a, b) * b, "intdiv": lambda a, b: 0 if b == 0 else wrap(tdiv(a, b)),
    "shl": shl, "shr": shr,
    "bitand": lambda a, b: a & b, "bitor": lambda a, b: a | b, "bitxor": lambda a, b: a ^ b,
    "lt": lambda a, b: int(a < b), "le": lambda a, b: int(a <= b), "gt": lambda a, b: int(a > b),
    "ge": lambda a, b: int(a >= b), "eq": lambda a, b: int(a == b), "ne": lambda a, b: int(a != b),
}


@pytest.mark.parametrize("op", sorted(EXACT))
def test_oracle_int_binary_ops_exact(op):
    a, b = X.EE
    got, t, err = eval_prog(X.bin_(op), [a, b])
    want = [EXACT[op](int(x), int(y)) for x, y in zip(a, b)]
    assert len(want) == 784 and got.dtype == np.int64 and t == (BOOL if op in X.CMP else I64)
    assert got.tolist() == want
    assert err.tolist() == ([int(y) == 0 for y in b] if op in X.DIVS else [False] * 784)
    assert int(err.sum()) == (28 if op in X.DIVS else 0)


def test_oracle_promised_edges():
    """the rules include/nutexec.h spells out, by name"""
    assert EXACT["mod"](MIN, -1) == 0 and EXACT["intdiv"](MIN, -1) == MIN
    assert EXACT["mod"](-7, 2) == -1 and EXACT["intdiv"](-7, 2) == -3
    assert shl(1, 63) == MIN and shl(1, 64) == 0 and shl(1, -1) == 0 and shr(-8, 64) == -1 and shr(-8, MIN) == -1
    assert shr(MAX, 64) == 0 and shr(MIN, 63) == -1


def test_oracle_int_unary_exact():
    e = X.i64(E)
    assert eval_prog(X.C0 + [("abs",)], [e])[0].tolist() == [wrap(abs(x)) for x in E]
    assert eval_prog(X.C0 + [("bitnot",)], [e])[0].tolist() == [~x for x in E]
    got, t, _ = eval_prog(X.C0 + [("to_f64",)], [e])
    assert t == F64 and len(got) == 28
    assert bits(got).tolist() == bits(X.f64([float(x) for x in E])).tolist()  # int.__float__ rounds to nearest even
    assert float(2**53 + 1) == 2.0**53 and float(-2**53 - 1) == -2.0**53 and float(MAX) == 2.0**63 == float(MAX - 1)


def test_oracle_fmod_exact():
    got, t, err = eval_prog(X.bin_("mod"), list(X.FAB))
    assert t == F64 and len(got) == 130 and not err.any()
    assert bits(got).tolist() == bits(X.FAB_WANT).tolist()
    assert int(np.sum(bits(got) == 0x8000000000000000)) == 21


def test_oracle_mixed_compare_exact():
    """int <cmp> f64: the int converts to f64 first, then IEEE comparison (Python's float
    operators).  An exact rational comparison would differ above 2^53: that is not the rule."""
    i, f = X.EF
    py = {"lt": lambda a, b: a < b, "le": lambda a, b: a <= b, "gt": lambda a, b: a > b, "ge": lambda a, b: a >= b,
          "eq": lambda a, b: a == b, "ne": lambda a, b: a != b}
    cells = 0
    for op in X.CMP:
        got, t, _ = eval_prog(X.bin_(op), [i, f])
        want = [int(py[op](float(int(a)), float(b))) for a, b in zip(i, f)]
        assert t == BOOL and got.tolist() == want, op
        back, _, _ = eval_prog(X.bin_(op, X.C1, X.C0), [i, f])
        assert back.tolist() == [int(py[op](float(b), float(int(a)))) for a, b in zip(i, f)], op
        cells += len(want)
    assert cells == 6 * 1036
    nan = np.isnan(f)
    assert int(nan.sum()) == 28 and eval_prog(X.bin_("ne"), [i, f])[0][nan].all()
    assert not eval_prog(X.bin_("eq"), [i, f])[0][nan].any()


def test_oracle_date_parts_exact():
    days = X.i64(X.DAYS)
    got = np.stack([date_part(days, p) for p in range(8)], axis=1)
    cal = np.array(X.IN_CALENDAR)
    want = [X.calendar_parts(d) for d, c in zip(X.DAYS, X.IN_CALENDAR) if c]
    assert len(want) == 111 and got[cal].tolist() == want
    # the program op is the same function
    for p in range(8):
        assert eval_prog(X.C0 + [("datepart", p)], [days])[0].tolist() == got[:, p].tolist()
    # the clamp: everything beyond +-2^40 days reads as +-2^40
    at = {d: got[i].tolist() for i, d in enumerate(X.DAYS)}
    assert at[MIN] == at[-2**40 - 1] == at[-2**40] != at[-2**40 + 1]
    assert at[MAX] == at[2**40 + 1] == at[2**40] != at[2**40 - 1]
    # the era boundary (day -719468 is 0000-03-01, the first day of era 0) continues the
    # proleptic calendar backwards: year 0 is a leap year
    assert at[-719468][7] == 301 and at[-719469][7] == 229 and at[-719467][7] == 302
    assert at[-719468][4] == datetime_weekday(-719468)


def datetime_weekday(day):
    return (day + 3) % 7 + 1  # Python % floors: 1970-01-01 (day 0) is a Thursday (4)


def test_operand_sets():
    """what the issue counts: 28 values, 784 pairs, 1036 mixed pairs, 130 fmod pairs (21 of
    them -0.0), 122 days (111 in the calendar), >= 64 contraction-sensitive triples, 4096
    pairs — the module asserts the rest on import"""
    assert (len(E), len(X.EE[0]), len(X.EF[0]), len(X.FAB[0]), len(X.DAYS)) == (28, 784, 1036, 130, 122)
    assert len(X.FMA[0]) >= 64 and len(X.DIVP[0]) == 4096
    a, b, c, twice = X.FMA
    assert a[0] == 1 + 2.0**-30 and b[0] == 1 - 2.0**-30 and c[0] == -1 and twice[0] == 0  # fused: -2^-60
    assert len(X.where_column()) == 4099 and set(E) <= set(X.where_column().tolist())


# ------------------------------------------------------------------ hipRTC: every spec of the GPU file
class FakeCol:
    """stands in for a device column when only its type matters (no pointer is read)"""

    def __init__(self, kind):
        self.dtype = torch.int64 if kind == "i" else torch.float64
        self.device = None

    def numel(self):
        return 0

    def is_contiguous(self):
        return True

    def dim(self):
        return 1

    def data_ptr(self):
        return 0


def compile_(fn, q):
    st = fn(C.byref(q.to_spec(None)))
    assert st == 0, L.lib.nut_last_error()


@pytest.mark.parametrize("name", sorted(X.eval_specs()))
def test_eval_specs_compile(name):
    types, progs = X.eval_specs()[name]
    assert 1 <= len(progs) <= 8
    compile_(L.lib.nut_eval_jit_compile,
             ProgQuery(keys=[], cols=[FakeCol(t) for t in types], aggs=[("sum", v, m) for v, m in progs]))


def test_constant_specs_share_one_source():
    """the *_k specs read their constant from the kernel arguments: MIN, MAX, -1 and 0 give
    the same source, so sweeping k costs no compile"""
    from test_expr_cpu import jit_source
    for name in ("int_bin_k", "int_cmp_k", "int_div_k"):
        src = set()
        for k in (MIN, MAX, -1, 0, 64):
            types, progs = X.eval_specs(k)[name]
            q = ProgQuery(keys=[], cols=[FakeCol(t) for t in types], aggs=[("sum", v, m) for v, m in progs])
            src.add(jit_source(q))
        assert len(src) == 1, name


@pytest.mark.parametrize("name", sorted(X.SELECT_SPECS))
def test_select_specs_compile(name):
    types, where = X.SELECT_SPECS[name]
    compile_(L.lib.nut_select_jit_compile, ProgQuery(keys=[], cols=[FakeCol(t) for t in types], aggs=[], where=where))


@pytest.mark.parametrize("name", ["aggs_nk0", "aggs_nk1"] + sorted(X.KEY_SPECS))
def test_groupby_specs_compile(name):
    cols = [FakeCol(t) for t in "iifi"]
    if name.startswith("aggs"):  # (a key column and the key program [col] make the same value programs)
        q = ProgQuery(keys=[] if name == "aggs_nk0" else [[("col", 3)]], cols=cols, aggs=X.GROUPBY_AGGS)
    else:
        keys, where = X.KEY_SPECS[name]
        q = ProgQuery(keys=keys, cols=cols, where=where, aggs=X.KEY_AGGS)
    compile_(L.lib.nut_groupby_jit_compile, q)


def test_sql_edges_compile():
    p = Plan(X.SQL_EDGES)
    d = p.describe()
    assert d["mode"] == "compiled" and len(d["project"]) == len(X.SQL_ITEMS) + len(X.FOLD_DAYS)
    p.prepare(X.SQL_TYPES)
    # the date function of a literal folds on the host: the twin of the device's jdatepart
    want = date_part(X.i64(X.FOLD_DAYS), 7).tolist()
    assert [str(w) for w in want] == d["project"][-len(X.FOLD_DAYS):]
    with pytest.raises(NutError, match="outside int64"):
        Plan("select a + 9223372036854775808 from t").prepare({"a": "int64"})


@pytest.mark.parametrize("op", sorted(X.COMPILED_CONSTS))
def test_where_constant_routes(op):
    """`col <cmp> k` alone is the fused filter (resolve_i64 decides it exactly); with
    `and col % 1 = 0` it is compiled, and compiles"""
    k = X.COMPILED_CONSTS[op][0]
    assert Plan(f"select col from t where col {op} {k}").describe()["mode"] == "fused"
    p = Plan(f"select col from t where col {op} {k} and col % 1 = 0")
    assert p.describe()["mode"] == "compiled"
    p.prepare({"col": "int64"})
