"""GPU: expression mode — programs compiled per query (csrc/jit.cpp, hipRTC) into the
streaming group-by kernel, checked against the numpy expression oracle (oracle/expr.py)
and the C group-by oracle.

  * a seeded fuzz of random typed expression trees (int / f64 / bool, every op) as WHERE,
    aggregate arguments and aggregate row masks, 0-2 keys, private and shared tables:
    bit-exact (SUM only over int programs, MIN/MAX/COUNT over all types);
  * the integer division-by-zero error rule (WHERE / mask scoping);
  * SQL: the reference fixture tests/sql/5.sql shape (integer codes for its strings),
    CASE without ELSE as an aggregate mask (sum/avg/count/min), > 16 IN values,
    column-vs-column predicates, and the compiled form of TPC-H Q1 against the fused
    kernel (counts exact, f64 sums <= 1e-12 relative).
Semantics are this build's (the reference executes no expressions): parity unpinned with
respect to the reference, pinned here against the independent numpy restatement.
"""
import numpy as np
import pytest
import torch

from helpers import F64_SUM_RTOL, rel_err
from nutdb_amd import NutError, ProgQuery
from oracle.expr import F64, DivisionByZero, groupby_prog

pytestmark = pytest.mark.gpu


def dev(x, ex):
    return torch.from_numpy(np.ascontiguousarray(x)).to(ex.device)


# ------------------------------------------------------------------ random programs
class Gen:
    """Random typed expression trees as RPN.  Divisors are made non-zero (x | 1,
    abs(y) + 1.0) so the fuzz compares values; zero divisors have their own test.
    No op can produce NaN (values stay finite), so f64 MIN/MAX compare bit-exactly.
    What this excludes — f64 division and fmod by zero, NaN / inf / subnormal operands,
    comparisons with a NaN, IF with a NaN branch — is tests/test_gpu_nonfinite.py's."""

    def __init__(self, rng, icols, fcols):
        self.r, self.ic, self.fc = rng, icols, fcols

    def pick(self, xs):
        return xs[int(self.r.integers(len(xs)))]

    def int_(self, d):
        r = self.r
        if d == 0 or r.random() < 0.2:
            return [("col", self.pick(self.ic))] if r.random() < 0.7 else [("i64", 0, int(r.integers(-9, 10)))]
        op = self.pick(["add", "sub", "mul", "mod", "intdiv", "bitand", "bitor", "bitxor", "shl", "shr", "abs",
                        "bitnot", "if"])
        if op in ("abs", "bitnot"):
            return self.int_(d - 1) + [(op,)]
        if op == "if":
            return self.bool_(d - 1) + self.int_(d - 1) + self.int_(d - 1) + [("if",)]
        a, b = self.int_(d - 1), self.int_(d - 1)
        if op in ("mod", "intdiv"):
            b = b + [("i64", 0, 1), ("bitor",)]
        if op in ("shl", "shr"):
            b = b + [("i64", 0, 63 if r.random() < 0.5 else 127), ("bitand",)]  # some counts >= 64
        return a + b + [(op,)]

    def f64_(self, d):
        r = self.r
        if d == 0 or r.random() < 0.2:
            k = r.random()
            if k < 0.6:
                return [("col", self.pick(self.fc))]
            if k < 0.8:
                return [("f64", 0, float(r.integers(-64, 64)) / 8.0)]
            return self.int_(0) + [("to_f64",)]
        op = self.pick(["add", "sub", "mul", "div", "mod", "abs", "if", "mix"])
        if op == "abs":
            return self.f64_(d - 1) + [("abs",)]
        if op == "if":
            return self.bool_(d - 1) + self.f64_(d - 1) + self.f64_(d - 1) + [("if",)]
        if op == "mix":  # int (+|*) f64: the int converts
            return self.int_(d - 1) + self.f64_(d - 1) + [(self.pick(["add", "mul", "sub"]),)]
        a, b = self.f64_(d - 1), self.f64_(d - 1)
        if op in ("div", "mod"):
            b = b + [("abs",), ("f64", 0, 1.0), ("add",)]
        return a + b + [(op,)]

    def bool_(self, d):
        r = self.r
        op = self.pick(["cmp", "cmp", "cmp", "and", "or", "xor", "not"])
        if d == 0 or op == "cmp":
            c = self.pick(["lt", "le", "gt", "ge", "eq", "ne"])
            kind = int(r.integers(3))
            dd = max(d - 1, 0)
            a = self.int_(dd) if kind != 1 else self.f64_(dd)
            b = self.int_(dd) if kind == 0 else self.f64_(dd)
            return a + b + [(c,)]
        if op == "not":
            return self.bool_(d - 1) + [("not",)]
        return self.bool_(d - 1) + self.bool_(d - 1) + [(op,)]


def make_table(rng, n):
    i0 = rng.integers(-50, 51, n).astype(np.int64)
    i1 = rng.integers(-2**40, 2**40, n).astype(np.int64)
    i2 = rng.integers(0, 1000, n).astype(np.int64)
    f0 = rng.integers(-4096, 4096, n).astype(np.float64) / 64.0
    f1 = rng.random(n)
    return [i0, i1, i2, f0, f1], [0, 1, 2], [3, 4]


def run_both(ex, keys, cols, where, aggs, hint):
    q = ProgQuery(keys=[dev(k, ex) for k in keys], cols=[dev(c, ex) for c in cols], where=where, aggs=aggs)
    g = ex.groupby(q, group_hint=hint)
    gk, gw = g.to_host_words()
    ok, ow, types = groupby_prog(keys, cols, where, [({"sum": 0, "count": 1, "min": 2, "max": 3}[o], v, m)
                                                      for o, v, m in aggs])
    return gk, gw, ok, ow, types


@pytest.mark.parametrize("seed", range(12))
def test_prog_fuzz(ex, seed):
    rng = np.random.default_rng(1000 + seed)
    n = 200_003 + seed
    cols, ic, fc = make_table(rng, n)
    g = Gen(rng, ic, fc)
    nk = seed % 3
    keys = [rng.integers(0, [1, 5, 40][seed % 3] + 1, n).astype(np.int64) for _ in range(nk)]
    if nk == 2:
        keys[1] = rng.integers(0, 3, n).astype(np.int64)
    where = g.bool_(2) if seed % 4 != 3 else None
    aggs = [("sum", g.int_(3), None), ("min", g.f64_(3), None), ("max", g.int_(2), None),
            ("count", None, g.bool_(2)), ("sum", g.int_(2), g.bool_(1)), ("max", g.f64_(2), g.bool_(1))]
    hint = [0, 4, 64][seed % 3]
    gk, gw, ok, ow, types = run_both(ex, keys, cols, where, aggs, hint)
    assert gk.shape[0] == ok.shape[0], (gk.shape, ok.shape)
    if nk:
        assert np.array_equal(gk, ok)
    assert np.array_equal(gw, ow), (seed, np.argwhere(gw != ow)[:5])
    assert types[1] == F64


def test_prog_division_by_zero(ex):
    n = 100_000
    a = np.arange(n, dtype=np.int64)
    b = (np.arange(n, dtype=np.int64) % 7)          # zero every 7th row
    k = (np.arange(n, dtype=np.int64) % 3)
    val = [("col", 0), ("col", 1), ("mod",)]
    with pytest.raises(NutError) as e:
        ex.groupby(ProgQuery(keys=[dev(k, ex)], cols=[dev(a, ex), dev(b, ex)], aggs=[("sum", val, None)]))
    assert "division by zero" in str(e.value)
    with pytest.raises(DivisionByZero):
        groupby_prog([k], [a, b], None, [(0, val, None)])
    # rows failing WHERE, or outside the aggregate's mask, never raise
    nz = [("col", 1), ("i64", 0, 0), ("ne",)]
    for where, mask in ((nz, None), (None, nz)):
        q = ProgQuery(keys=[dev(k, ex)], cols=[dev(a, ex), dev(b, ex)], where=where,
                      aggs=[("sum", val, mask), ("count", None, mask)])
        gk, gw = ex.groupby(q).to_host_words()
        ok, ow, _ = groupby_prog([k], [a, b], where, [(0, val, mask), (1, None, mask)])
        assert np.array_equal(gk, ok) and np.array_equal(gw, ow)
    # intDiv too; the error of the untaken IF branch does not count
    q = ProgQuery(keys=[], cols=[dev(a, ex), dev(b, ex)],
                  aggs=[("sum", nz + [("col", 0), ("col", 1), ("intdiv",), ("i64", 0, 0), ("if",)], None)])
    gk, gw = ex.groupby(q).to_host_words()
    _, ow, _ = groupby_prog([], [a, b], None, [(0, q.aggs[0][1], None)])
    assert np.array_equal(gw, ow)


# ------------------------------------------------------------------ SQL
def test_sql_fixture5_shape(ex):
    """tests/sql/5.sql of the reference (TPC-H Q12 shape) with integer codes standing in
    for its string constants: column-vs-column predicates, IN, CASE inside SUM."""
    rng = np.random.default_rng(5)
    n = 1_000_003
    okey = rng.integers(0, 50, n).astype(np.int64)
    lkey = np.where(rng.random(n) < 0.7, okey, rng.integers(0, 50, n)).astype(np.int64)
    mode = rng.integers(0, 7, n).astype(np.int64)
    prio = rng.integers(1, 6, n).astype(np.int64)
    ship = rng.integers(8000, 10000, n).astype(np.int64)
    commit = ship + rng.integers(-30, 30, n)
    receipt = ship + rng.integers(-30, 30, n)
    cols = {"o_orderkey": okey, "l_orderkey": lkey, "l_shipmode": mode, "o_orderpriority": prio,
            "l_shipdate": ship, "l_commitdate": commit, "l_receiptdate": receipt}
    sql = """select l_shipmode,
        sum(case when o_orderpriority = 1 or o_orderpriority = 2 then 1 else 0 end) as high_line_count,
        sum(case when o_orderpriority <> 1 and o_orderpriority <> 2 then 1 else 0 end) as low_line_count
      from orders
      where o_orderkey = l_orderkey and l_shipmode in (3, 5) and l_commitdate < l_receiptdate
        and l_shipdate < l_commitdate
      group by l_shipmode order by l_shipmode"""
    got = ex.sql(sql, {k: dev(v, ex) for k, v in cols.items()})
    m = (okey == lkey) & np.isin(mode, [3, 5]) & (commit < receipt) & (ship < commit)
    modes = np.unique(mode[m])
    assert got["l_shipmode"].tolist() == modes.tolist()
    hi = [int(np.sum(m & (mode == s) & ((prio == 1) | (prio == 2)))) for s in modes]
    lo = [int(np.sum(m & (mode == s) & (prio != 1) & (prio != 2))) for s in modes]
    assert got["high_line_count"].tolist() == hi and got["low_line_count"].tolist() == lo


def test_sql_case_without_else(ex):
    rng = np.random.default_rng(7)
    n = 500_000
    k = rng.integers(0, 6, n).astype(np.int64)
    v = (rng.integers(-1000, 1000, n) / 16.0).astype(np.float64)
    w = rng.integers(-100, 100, n).astype(np.int64)
    sql = """select k, sum(case when v > 0 then v end) as sp, avg(case when v > 0 then v end) as ap,
        count(case when w % 3 = 0 then 1 end) as c3, min(case w when 1 then v when 2 then null else w end) as mn,
        count(v) as cv
      from t where k != 2 group by k order by k"""
    got = ex.sql(sql, {"k": dev(k, ex), "v": dev(v, ex), "w": dev(w, ex)})
    keys = [0, 1, 3, 4, 5]
    assert got["k"].tolist() == keys
    for i, g in enumerate(keys):
        r = k == g
        pos = r & (v > 0)
        assert got["sp"][i] == np.sum(v[pos])                      # dyadic: exact
        assert got["ap"][i] == np.sum(v[pos]) / np.sum(pos)
        assert got["c3"][i] == np.sum(r & (w % 3 == 0))
        sel = r & (w != 2)
        mn = np.min(np.where(w[sel] == 1, v[sel], w[sel].astype(np.float64)))
        assert got["mn"][i] == mn
        assert got["cv"][i] == np.sum(r)


def test_sql_long_in_list_and_or(ex):
    rng = np.random.default_rng(9)
    n = 300_001
    k = rng.integers(0, 40, n).astype(np.int64)
    x = rng.integers(0, 100, n).astype(np.int64)
    lst = list(range(0, 60, 3))  # 20 values: beyond the fused kernel's 16
    sql = f"select k, count(*) as c, sum(x) as s from t where x in ({', '.join(map(str, lst))}) or k > 35 group by k"
    got = ex.sql(sql, {"k": dev(k, ex), "x": dev(x, ex)}, group_hint=40)
    m = np.isin(x, lst) | (k > 35)
    keys = np.unique(k[m])
    assert got["k"].tolist() == keys.tolist()
    assert got["c"].tolist() == [int(np.sum(m & (k == g))) for g in keys]
    assert got["s"].tolist() == [int(np.sum(x[m & (k == g)])) for g in keys]


def test_sql_compiled_q1_matches_fused(ex):
    from nutdb_amd.workloads import Q1_COLS, gen
    n = 4_000_037
    cols = {s[0]: gen(ex, s, n) for s in Q1_COLS}
    body = """select l_returnflag, l_linestatus, sum(l_quantity) as q, sum(l_extendedprice) as p,
        sum(l_extendedprice * (1 - l_discount)) as d, count(*) as c
      from lineitem where {} group by l_returnflag, l_linestatus"""
    fused = ex.sql(body.format("l_shipdate <= 10471"), cols, group_hint=6)
    comp = ex.sql(body.format("l_shipdate <= 10471 or l_quantity < 0"), cols, group_hint=6)
    assert fused["c"].tolist() == comp["c"].tolist()
    assert fused["l_returnflag"].tolist() == comp["l_returnflag"].tolist()
    for c in ("q", "p", "d"):
        assert rel_err(comp[c], fused[c]) <= F64_SUM_RTOL


def test_sql_compiled_global_aggregate(ex):
    n = 1000
    a = np.arange(n, dtype=np.int64)
    got = ex.sql("select sum(a * a), count(case when a % 2 = 0 then 1 end), max(a / 4) from t where a >= 10 or a < 0",
                 {"a": dev(a, ex)})
    vals = list(got.values())
    sel = a[a >= 10]
    assert vals[0].tolist() == [int(np.sum(sel * sel))]
    assert vals[1].tolist() == [int(np.sum(sel % 2 == 0))]
    assert vals[2].tolist() == [np.max(sel / 4)]
    empty = ex.sql("select count(*), sum(a) from t where a > 5000 or a < -1", {"a": dev(a, ex)})
    assert [v.tolist() for v in empty.values()] == [[0], [0]]


def test_bench_q12_programs_match_sql(ex):
    """bench.py q12expr's CPU baseline evaluates hand-written programs (workloads.py):
    they must be the query the SQL path runs."""
    from nutdb_amd.workloads import Q12_AGGS, Q12_COLS, Q12_SQL, Q12_WHERE, gen
    n = 2_000_003
    cols = {s[0]: gen(ex, s, n) for s in Q12_COLS}
    got = ex.sql(Q12_SQL, cols, group_hint=8)
    host = [cols[s[0]].cpu().numpy() for s in Q12_COLS]
    ok, ow, _ = groupby_prog([host[2]], host, Q12_WHERE, Q12_AGGS)
    assert got["l_shipmode"].tolist() == ok[:, 0].tolist() == [3, 5]
    assert got["high_line_count"].tolist() == ow[:, 0].astype(np.int64).tolist()
    assert got["low_line_count"].tolist() == ow[:, 1].astype(np.int64).tolist()


# ------------------------------------------------------------------ expression-mode scans
@pytest.mark.parametrize("seed", range(8))
def test_select_rows_fuzz(ex, seed):
    """nut_select_rows (select_kernel.hpp, WHERE compiled per query) against the numpy
    expression oracle: the selected row ids, in order, bit-exact."""
    from oracle.expr import eval_prog
    rng = np.random.default_rng(2000 + seed)
    n = [1, 4095, 4097, 300_007, 1_000_003, 77, 65536, 250_000][seed]
    cols, ic, fc = make_table(rng, n)
    where = Gen(rng, ic, fc).bool_(3) if seed != 5 else None
    got = ex.select_rows([dev(c, ex) for c in cols], where).cpu().numpy()
    if where is None:
        want = np.arange(n)
    else:
        w, _, e = eval_prog(where, cols, n)
        want = np.nonzero(w != 0)[0]
    assert np.array_equal(got, want), (seed, len(got), len(want))


def test_select_rows_division_by_zero(ex):
    a = np.arange(10_000, dtype=np.int64)
    b = a % 5
    with pytest.raises(NutError, match="division by zero"):
        ex.select_rows([dev(a, ex), dev(b, ex)], [("col", 0), ("col", 1), ("mod",), ("i64", 0, 1), ("eq",)])


def test_sql_expression_scans(ex):
    rng = np.random.default_rng(17)
    n = 500_003
    x = rng.integers(-1000, 1000, n).astype(np.int64)
    y = rng.integers(-1000, 1000, n).astype(np.int64)
    f = rng.random(n)
    cols = {"x": dev(x, ex), "y": dev(y, ex), "f": dev(f, ex)}
    got = ex.sql("select x from t where x < y and f > 0.25", cols)
    assert got["x"].tolist() == x[(x < y) & (f > 0.25)].tolist()
    got = ex.sql("select x from t where x in (1, 2, 3, 500) or y % 7 = 0", cols)
    assert got["x"].tolist() == x[np.isin(x, [1, 2, 3, 500]) | (y % 7 == 0)].tolist()
    got = ex.sql("select x from t where x * 2 > y order by x desc limit 10 offset 3", cols)
    assert got["x"].tolist() == np.sort(x[x * 2 > y])[::-1][3:13].tolist()
    got = ex.sql("select y from t where f between 0.1 and 0.2 order by y", cols)
    assert got["y"].tolist() == np.sort(y[(f >= 0.1) & (f <= 0.2)]).tolist()
    assert ex.sql("select x from t where x > 5000 or y > 5000", cols)["x"].tolist() == []


def test_sql_scan_several_columns(ex):
    """expression-mode scans project several int64 / float64 columns (one gather each)"""
    rng = np.random.default_rng(23)
    n = 300_001
    x = rng.integers(-100, 100, n).astype(np.int64)
    f = rng.random(n)
    y = rng.integers(0, 1000, n).astype(np.int64)
    cols = {"x": dev(x, ex), "f": dev(f, ex), "y": dev(y, ex)}
    got = ex.sql("select y, f as ff, x from t where x > 10 and f < 0.5 limit 1000 offset 7", cols)
    m = (x > 10) & (f < 0.5)
    assert list(got) == ["y", "ff", "x"]
    assert got["y"].tolist() == y[m][7:1007].tolist() and got["x"].tolist() == x[m][7:1007].tolist()
    assert got["ff"].dtype == np.float64 and np.array_equal(got["ff"], f[m][7:1007])
    got = ex.sql("select x, y from t", cols)
    assert np.array_equal(got["x"], x) and np.array_equal(got["y"], y)


def test_sql_select_distinct(ex):
    rng = np.random.default_rng(29)
    n = 400_003
    k = rng.integers(0, 50, n).astype(np.int64)
    j = rng.integers(-3, 3, n).astype(np.int64)
    x = rng.random(n)
    cols = {"k": dev(k, ex), "j": dev(j, ex), "x": dev(x, ex)}
    got = ex.sql("select distinct k from t where x > 0.5", cols)
    assert got["k"].tolist() == np.unique(k[x > 0.5]).tolist()
    got = ex.sql("select distinct k, j from t where k < 10 or x < 0.01 order by k desc", cols)
    m = (k < 10) | (x < 0.01)
    gk = got["k"].tolist()
    assert gk == sorted(gk, reverse=True)
    assert sorted(zip(gk, got["j"].tolist())) == sorted(set(zip(k[m].tolist(), j[m].tolist())))
