"""GPU: the math program ops (FLOOR CEIL TRUNC ROUND, MATH, POW, SIGN, LEAST, GREATEST, CAST:
csrc/prog_ops.hpp and the jit.cpp prelude) and the SQL built on them, on the operands of
tests/math_edges.py.  The exactly defined ops (rounding, sign, least / greatest, casts, sqrt) are
bit-exact against that file's restatement, which tests/test_math_edges_cpu.py holds to exact
arithmetic.  exp, ln, log2, log10 and pow are checked against `decimal` at 60 digits: the class
of every result exactly, every finite result within the device math library's contract (3 ulp;
pow 16 ulp); each test prints the maximum it measured (DESIGN.md §3.13 records them).  Inputs are a few thousand rows: the cost is the
hipRTC compiles (about 25 in this file)."""
import collections
import math

import numpy as np
import pytest
import torch

import math_edges as M
from expr_edges import MAX, MIN
from nutdb_amd import ProgQuery
from nutdb_amd.sql import Plan
from nutdb_amd.table import Table

pytestmark = pytest.mark.gpu


def dev(x, ex):
    return torch.from_numpy(np.ascontiguousarray(x)).to(ex.device)


def run_eval(ex, cols, progs):
    out, valid = ex.eval_rows([dev(c, ex) for c in cols], [(p, None) for p in progs])
    assert all(bool(v.all()) for v in valid)
    return np.stack([o.cpu().numpy() for o in out], axis=1).view(np.uint64)  # [rows, programs] words


# ------------------------------------------------------------------ 1. nut_eval_rows over the edge lists
@pytest.mark.parametrize("name", sorted(M.EVAL_SPECS))
def test_exact_ops_bit_for_bit(ex, name):
    src, progs = M.EVAL_SPECS[name]
    cols, rows = M.operands(src)
    got = run_eval(ex, cols, progs).tolist()
    want = M.eval_want(name)
    assert len(got) == len(rows) and len(rows) % 64 != 0 and len(got[0]) == len(progs)
    bad = [(r, rows[r], j, hex(got[r][j]), hex(want[r][j])) for r in range(len(rows)) for j in range(len(progs))
           if got[r][j] != want[r][j]]
    assert not bad, f"{len(bad)} cells differ; first (row, operands, program, got, want): {bad[:5]}"


@pytest.mark.parametrize("name", sorted(M.TR_SPECS))
def test_transcendentals_within_the_library_bounds(ex, name):
    src, progs, fns = M.TR_SPECS[name]
    cols, rows = M.operands(src)
    got = run_eval(ex, cols, progs)
    assert got.shape == (len(rows), len(fns)) and len(rows) % 64 != 0
    xs = [r[0] for r in rows]
    ys = [r[1] for r in rows] if src == "pow" else None
    for j, fn in enumerate(fns):
        worst, bad = M.check_transcendental(fn, got[:, j].tolist(), xs, ys)
        print(f"{fn}: max {worst:.3f} ulp over {len(rows)} operands (bound {M.ULP_BOUND[fn]})")
        assert not bad, f"{fn}: {len(bad)} of {len(rows)} operands miss; max {worst} ulp; first: {bad[:5]}"
        assert 0 < worst <= M.ULP_BOUND[fn]


# ------------------------------------------------------------------ 2. where, aggregate argument, computed key
GB_ROWS = 5003


def _gb_cols():
    rng = np.random.default_rng(5003)
    f = np.round(rng.uniform(-400, 400, GB_ROWS), 3)
    f[rng.choice(GB_ROWS, 40, replace=False)] = np.resize(np.array([-0.0, 0.0, 9.999, -9.999, 10.0, -10.0, 399.9996, 0.5]), 40)
    i = rng.integers(-2000, 2001, GB_ROWS).astype(np.int64)
    i[rng.choice(GB_ROWS, 30, replace=False)] = np.resize(np.array([50, -50, 150, -150, 49, -49, 0, 1950, -1950, 2000]), 30)
    return f, i


@pytest.mark.parametrize("hint", [4, 4096], ids=["private", "shared"])
@pytest.mark.parametrize("key", ["toInt64(f / 10)", "round(i, -2)"])
def test_groupby_paths(ex, key, hint):
    """WHERE sign(i) != 0 and greatest(f, i) > -300; COUNT, SUM(round(f, 2)) (compared to 1e-12,
    the suite's rule for f64 sums), MIN(least(i, 7)), MAX(toInt8(i)) per computed key, through the
    private-table kernel and the shared-table one"""
    f, i = _gb_cols()
    kp = M.KEY_F if key.startswith("toInt64") else M.KEY_I
    where = M.C1 + [("sign",), ("i64", 0, 0), ("ne",)] + M.C0 + M.C1 + [("greatest",), ("f64", 0, -300.0), ("gt",), ("and",)]
    aggs = [("count", None, None), ("sum", M.C0 + [("round", 2)], None), ("min", M.C1 + [("i64", 0, 7), ("least",)], None),
            ("max", M.C1 + [("cast", 3)], None)]
    q = ProgQuery(keys=[kp], cols=[dev(f, ex), dev(i, ex)], where=where, aggs=aggs)
    gk, gw = ex.groupby(q, group_hint=hint).to_host_words()
    want = collections.defaultdict(lambda: [0, [], MAX, MIN])
    for x, y in zip(f.tolist(), i.tolist()):
        if M.sign(y) != 0 and M.least(x, y, True) > -300.0:
            acc = want[M.model(kp, (x, y))]
            acc[0] += 1
            acc[1].append(M.round_f(x, 3, 2))
            acc[2] = min(acc[2], M.least(y, 7))
            acc[3] = max(acc[3], M.cast(y, 3))
    order = sorted(want)
    assert GB_ROWS % 64 and len(order) >= 40 and [k[0] for k in gk.tolist()] == order
    gi = gw.view(np.int64)
    assert gi[:, 0].tolist() == [want[k][0] for k in order] and 0 < int(gi[:, 0].sum()) < GB_ROWS
    assert gi[:, 2].tolist() == [want[k][2] for k in order] and gi[:, 3].tolist() == [want[k][3] for k in order]
    sums = gw[:, 1].view(np.float64)
    for k, s in zip(order, sums.tolist()):
        w = math.fsum(want[k][1])
        assert abs(s - w) <= 1e-12 * max(math.fsum(abs(v) for v in want[k][1]), 1e-300), (k, s, w)


# ------------------------------------------------------------------ 3. SQL
N = 6007


def _table():
    rng = np.random.default_rng(6007)
    price = np.round(rng.uniform(0.01, 2500.0, N), 2)
    a = rng.integers(-9, 10, N).astype(np.int64)
    b = rng.integers(-9, 10, N).astype(np.int64)
    x = rng.integers(-300, 301, N).astype(np.int64)
    x[:8] = [127, 128, -128, -129, 255, 256, 0, -1]
    g = np.round(rng.normal(0, 50, N), 3)
    g[:8] = [np.nan, np.inf, -np.inf, 1e19, -1e19, -0.5, 0.05, 2.5]
    return {"price": price, "a": a, "b": b, "x": x, "g": g}


COLS = _table()


def f64_words(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64).tolist()


def run_queries(execute):
    """the issue's five query shapes through execute(sql) -> {name: array}; returns the cells
    compared"""
    price, a, b, x, g = (COLS[k] for k in ("price", "a", "b", "x", "g"))
    cells = 0
    # a bucketed float column: key, count, round(avg), sqrt over a sum
    got = execute("select toInt64(price / 100) as b, count() as c, round(avg(price), 2) as r, "
                  "sqrt(sum(price * price) / count()) as q from t group by b order by b")
    bucket = [M.to_i64(p / 100.0) for p in price.tolist()]
    keys = sorted(set(bucket))
    assert got["b"].tolist() == keys and len(keys) == 25
    for j, k in enumerate(keys):
        v = [p for p, kk in zip(price.tolist(), bucket) if kk == k]
        assert got["c"][j] == len(v)
        # (the device sums in another order, to 1e-12: the same multiple of 10^-2 unless the
        # average sits within that of a tie, which no bucket's does)
        avg = math.fsum(v) / len(v)
        assert abs(avg * 100 % 1 - 0.5) > 1e-6
        assert M.fbits(float(got["r"][j])) == M.fbits(M.round_f(avg, 3, 2)), (k, got["r"][j], avg)
        q = math.sqrt(math.fsum(p * p for p in v) / len(v))
        assert abs(got["q"][j] - q) <= 1e-12 * q
        cells += 3
    # a scan: floor / ceil / round(x, 1) projections behind sign and greatest in WHERE
    got = execute("select floor(g) as fl, ceil(g) as ce, round(g, 1) as r1, trunc(g, -1) as t1, sign(g) as sg, toFloat32(g) as f32 "
                  "from t where sign(a) = -1 and greatest(a, b) > 3")
    keep = [r for r in range(N) if a[r] < 0 and max(a[r], b[r]) > 3]
    assert 100 < len(keep) < N // 4
    for name, fn in (("fl", lambda v: M.round_f(v, 0, 0)), ("ce", lambda v: M.round_f(v, 1, 0)), ("r1", lambda v: M.round_f(v, 3, 1)),
                     ("t1", lambda v: M.round_f(v, 2, -1)), ("f32", lambda v: M.cast(v, 7))):
        assert f64_words(got[name]) == [M.fbits(fn(float(g[r]))) for r in keep], name
        cells += len(keep)
    assert got["sg"].dtype == np.int64 and got["sg"].tolist() == [M.sign(float(g[r])) for r in keep]
    # HAVING and ORDER BY over round(sum / count, 1)
    got = execute("select a, round(sum(price) / count(), 1) as m, greatest(min(x), 0) as gm, toInt64(avg(price)) as ia from t "
                  "group by a having round(sum(price) / count(), 1) > 1240 order by round(sum(price) / count(), 1) desc, a")
    per = {}
    for k in sorted(set(a.tolist())):
        v = [p for p, kk in zip(price.tolist(), a.tolist()) if kk == k]
        mean = math.fsum(v) / len(v)
        per[k] = (M.round_f(mean, 3, 1), max(min(xx for xx, kk in zip(x.tolist(), a.tolist()) if kk == k), 0), M.to_i64(mean), mean)
    assert all(abs(p[3] * 10 % 1 - 0.5) > 1e-6 and abs(p[3] % 1) > 1e-6 for p in per.values())  # (no mean sits on a tie)
    want = sorted((k for k in per if per[k][0] > 1240), key=lambda k: (-per[k][0], k))
    assert 2 <= len(want) < len(per) and got["a"].tolist() == want
    assert f64_words(got["m"]) == [M.fbits(per[k][0]) for k in want]
    assert got["gm"].tolist() == [per[k][1] for k in want] and got["ia"].tolist() == [per[k][2] for k in want]
    cells += 4 * len(want)
    # toInt8 wraps at 127 / 128; toInt64 of NaN / +-inf / 1e19
    got = execute("select toInt8(x) as i8, toUInt8(x) as u8, toInt64(g) as i, toInt32(g * 100000000) as w, round(x, -2) as rx from t")
    assert got["i8"][:6].tolist() == [127, -128, -128, 127, -1, 0] and got["u8"][:6].tolist() == [127, 128, 128, 127, 255, 0]
    assert got["i"][:6].tolist() == [0, MAX, MIN, MAX, MIN, 0]
    assert got["i8"].tolist() == [M.cast(v, 3) for v in x.tolist()] and got["u8"].tolist() == [M.cast(v, 6) for v in x.tolist()]
    assert got["i"].tolist() == [M.to_i64(v) for v in g.tolist()]
    assert got["w"].tolist() == [M.cast(v * 100000000.0, 1) for v in g.tolist()]
    assert got["rx"].tolist() == [M.round_i(v, 3, -2) for v in x.tolist()]
    cells += 5 * N
    # a rounded integer as the key
    got = execute("select round(x, -2) as k, count() as c, sum(pow(a, 2)) as s2 from t group by k order by k")
    cnt = collections.Counter(M.round_i(v, 3, -2) for v in x.tolist())
    assert got["k"].tolist() == sorted(cnt) == [-300, -200, -100, 0, 100, 200, 300] and got["c"].tolist() == [cnt[k] for k in sorted(cnt)]
    s2 = collections.defaultdict(float)
    for v, aa in zip(x.tolist(), a.tolist()):
        s2[M.round_i(v, 3, -2)] += float(aa * aa)
    assert all(abs(s - s2[k]) <= 1e-12 * s2[k] for k, s in zip(sorted(cnt), got["s2"].tolist()))
    return cells + 3 * len(cnt)


@pytest.mark.parametrize("narrow", [False, True], ids=["wide", "narrow"])
def test_sql_typed_table(ex, narrow):
    t = Table(ex, "CREATE TABLE t (price Float64, a Int8, b Int8, x Int16, g Float64)", narrow=narrow)
    t.append(**COLS)
    assert t.nrows == N and N % 64
    assert run_queries(lambda sql: t.execute(Plan(sql))) > 5 * N


def test_sql_raw_columns(ex):
    cols = {k: dev(v, ex) for k, v in COLS.items()}
    assert run_queries(lambda sql: Plan(sql).execute(ex, cols)) > 5 * N
