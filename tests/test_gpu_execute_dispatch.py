"""The entry point x plan shape matrix of the plan / table execute functions, on the GPU.

Six C entry points run a plan (nut_plan_execute, nut_plan_execute2, nut_plan_executen over
raw columns; nut_table_execute, nut_table_execute2, nut_table_executen over typed tables).
The other suites drive each SQL feature along its usual route; this one drives ten plan
shapes through every Python method that reaches a distinct entry point (and through the
n-table ones with 1, 2 and 3 tables) and pins, per cell, either the result (equal across the
entry points that accept the shape, column order included, and equal to pandas) or the
rejection (status code and a stable part of the message).

Tables of about 1000 int64 rows; each has a typed twin from a CREATE TABLE with one String
column more.  A rejection names the status and the text the caller sees:

  (f) through execute                    -> "has a JOIN"
  (h) through execute_join               -> "joins several tables"   (raw columns)
  (h) through execute_tables, 2 tables   -> "joins 3 tables, got 2"
  (a) through execute_tables, 3 tables   -> "joins fewer tables"
  (e) through execute_tables, 3 tables   -> "takes one table per branch"

Cells where the typed-table entry points answer differently from the raw-column ones (they
are recorded as they are): a JOIN plan through Table.execute, or through execute_joins with
the one table, is not refused as a JOIN but fails to bind the other table's first column
("has no column", NUT_ERR_PLAN); a two-JOIN chain through Table.execute_join reaches the
chain executor, which counts the tables ("joins 3 tables, got 2")."""
import numpy as np
import pandas as pd
import pytest
import torch

from nutdb_amd import NutError
from nutdb_amd.sql import Plan
from nutdb_amd.table import Table

pytestmark = pytest.mark.gpu

INVALID_ARG, PLAN = 1, 7  # nut_status

SHAPES = {
    "a_groupby": "select k, count(*) as n, sum(a) as sa from t group by k order by k",
    "b_star_scan": "select * from t where a > 500",
    "c_scalar_subquery": "select a, b from t where a > (select avg(a) from t)",
    "d_derived": "select n, count(*) as c from (select k, count(*) as n from t group by k) as d group by n order by n",
    "e_union": "select a, b from t where a > 900 union all select a, b from t2 where b < 5",
    "f_join": "select k, count(*) as n, sum(c) as sc from t join u on k = uk group by k order by k",
    "g_join_on_filter": "select k, count(*) as n, sum(c) as sc from t join u on k = uk and c < 50 group by k order by k",
    "h_chain": ("select k, count(*) as n, sum(c) as sc, sum(d) as sd from t join u on k = uk join w on k = wk "
                "group by k order by k"),
    "i_join_subquery": ("select k, count(*) as n, sum(c) as sc from t join u on k = uk "
                        "where a > (select avg(a) from t) group by k order by k"),
    "j_cte_left_join": ("with d as (select k, count(uk) as n from t left join u on k = uk group by k) "
                        "select n, count(*) as c from d group by n order by n"),
}

# the Python methods and table counts that reach distinct C entry points: raw columns, typed tables
RAW = ["execute", "execute_join", "execute_tables_1", "execute_tables_2", "execute_tables_3"]
TYPED = ["Table.execute", "Table.execute_join", "Table.execute_joins_1", "Table.execute_joins_2", "Table.execute_joins_3"]

OK, OK2 = "ok", "ok2"  # OK2: the UNION's second branch runs over the second table
FEWER = (INVALID_ARG, "joins fewer tables")
HAS_JOIN = (INVALID_ARG, "has a JOIN")
NO_COLUMN = (PLAN, "has no column")


def got_n(have, want):
    return (INVALID_ARG, f"joins {want} tables, got {have}")


ONE_TABLE = {"raw": [OK, OK, OK, OK, FEWER], "typed": [OK, OK, OK, OK, FEWER]}
PER_BRANCH = (INVALID_ARG, "takes one table per branch")
TWO_TABLES = {"raw": [HAS_JOIN, OK, HAS_JOIN, OK, FEWER], "typed": [NO_COLUMN, OK, NO_COLUMN, OK, FEWER]}
MATRIX = {
    "a_groupby": ONE_TABLE,
    "b_star_scan": ONE_TABLE,
    "c_scalar_subquery": ONE_TABLE,
    "d_derived": ONE_TABLE,
    "e_union": {"raw": [OK, OK2, OK, OK2, PER_BRANCH], "typed": [OK, OK2, OK, OK2, PER_BRANCH]},
    "f_join": TWO_TABLES,
    "g_join_on_filter": {"raw": [HAS_JOIN, OK, got_n(1, 2), OK, got_n(3, 2)],
                         "typed": [NO_COLUMN, OK, got_n(1, 2), OK, got_n(3, 2)]},
    "h_chain": {"raw": [HAS_JOIN, (INVALID_ARG, "joins several tables"), got_n(1, 3), got_n(2, 3), OK],
                "typed": [NO_COLUMN, got_n(2, 3), got_n(1, 3), got_n(2, 3), OK]},
    "i_join_subquery": TWO_TABLES,
    "j_cte_left_join": {"raw": [(INVALID_ARG, "derived table has a JOIN"), OK, HAS_JOIN, OK, FEWER],
                        "typed": [(INVALID_ARG, "derived table has a JOIN"), OK, NO_COLUMN, OK, FEWER]},
}


def make_data():
    rng = np.random.default_rng(2024)
    i64 = lambda x: np.ascontiguousarray(x, dtype=np.int64)  # noqa: E731
    t = {"a": i64(rng.integers(0, 1000, 1000)), "b": i64(rng.integers(0, 100, 1000)), "k": i64(rng.integers(0, 50, 1000))}
    t2 = {"a": i64(rng.integers(0, 1000, 700)), "b": i64(rng.integers(0, 100, 700)), "k": i64(rng.integers(0, 50, 700))}
    u = {"uk": i64(rng.integers(0, 60, 120)), "c": i64(rng.integers(0, 100, 120))}
    w = {"wk": i64(rng.integers(0, 45, 60)), "d": i64(rng.integers(0, 100, 60))}
    strs = {"t": ("s", np.array([f"s{v}" for v in t["b"]], dtype=object)),
            "t2": ("s", np.array([f"z{v}" for v in t2["b"]], dtype=object)),
            "u": ("us", np.array([f"u{v}" for v in u["c"]], dtype=object)),
            "w": ("ws", np.array([f"w{v}" for v in w["d"]], dtype=object))}
    return {"t": t, "t2": t2, "u": u, "w": w}, strs


def answers(raw, strs):
    """{shape: {OK / OK2: DataFrame}} from pandas; typed `*` answers carry the String column"""
    t, t2, u, w = (pd.DataFrame(raw[n]) for n in ("t", "t2", "u", "w"))
    out = {}
    out["a_groupby"] = {OK: t.groupby("k").agg(n=("a", "size"), sa=("a", "sum")).reset_index()}
    out["b_star_scan"] = {OK: t[t.a > 500]}
    out["c_scalar_subquery"] = {OK: t[t.a > t.a.mean()][["a", "b"]]}
    per = t.groupby("k").size().value_counts().sort_index()
    out["d_derived"] = {OK: pd.DataFrame({"n": per.index.to_numpy(), "c": per.to_numpy()})}
    out["e_union"] = {OK: pd.concat([t[t.a > 900][["a", "b"]], t[t.b < 5][["a", "b"]]]),
                      OK2: pd.concat([t[t.a > 900][["a", "b"]], t2[t2.b < 5][["a", "b"]]])}

    def joined(left, right):
        m = left.merge(right, left_on="k", right_on="uk")
        return m.groupby("k").agg(n=("c", "size"), sc=("c", "sum")).reset_index()

    out["f_join"] = {OK: joined(t, u)}
    out["g_join_on_filter"] = {OK: joined(t, u[u.c < 50])}
    m = t.merge(u, left_on="k", right_on="uk").merge(w, left_on="k", right_on="wk")
    out["h_chain"] = {OK: m.groupby("k").agg(n=("c", "size"), sc=("c", "sum"), sd=("d", "sum")).reset_index()}
    out["i_join_subquery"] = {OK: joined(t[t.a > t.a.mean()], u)}
    lj = t.merge(u, left_on="k", right_on="uk", how="left")
    per = lj.groupby("k").uk.count().value_counts().sort_index()
    out["j_cte_left_join"] = {OK: pd.DataFrame({"n": per.index.to_numpy(), "c": per.to_numpy()})}
    star_typed = out["b_star_scan"][OK].assign(s=strs["t"][1][(t.a > 500).to_numpy()])
    return out, star_typed


@pytest.fixture(scope="module")
def world(ex):
    raw, strs = make_data()
    dev = {n: {k: torch.from_numpy(v).to(ex.device) for k, v in cols.items()} for n, cols in raw.items()}
    typed = {}
    for n, cols in raw.items():
        sname, svals = strs[n]
        tab = Table(ex, "CREATE TABLE %s (%s, %s String)" % (n, ", ".join(f"{c} Int64" for c in cols), sname))
        tab.append(**cols, **{sname: svals})
        typed[n] = tab
    want, star_typed = answers(raw, strs)
    yield {"raw": raw, "dev": dev, "typed": typed, "want": want, "star_typed": star_typed}
    for tab in typed.values():
        tab.free()


def run(ex, world, family, entry, shape):
    """`shape` through `entry`: the FROM table first, then t2 (UNION) or u, then w"""
    plan = Plan(SHAPES[shape])
    second = "t2" if shape == "e_union" else "u"
    if family == "raw":
        d = world["dev"]
        tabs = [d["t"], d[second], d["w"]]
        if entry == "execute":
            return plan.execute(ex, tabs[0])
        if entry == "execute_join":
            return plan.execute_join(ex, tabs[0], tabs[1])
        return plan.execute_tables(ex, tabs[:int(entry[-1])])
    d = world["typed"]
    tabs = [d["t"], d[second], d["w"]]
    if entry == "Table.execute":
        return tabs[0].execute(plan)
    if entry == "Table.execute_join":
        return tabs[0].execute_join(plan, tabs[1])
    return tabs[0].execute_joins(plan, tabs[1:int(entry[-1])])


def same(got, want):
    assert list(got) == list(want.columns), (list(got), list(want.columns))
    for name in want.columns:
        g, w = got[name], want[name].to_numpy()
        assert not isinstance(g, np.ma.MaskedArray), name
        if w.dtype == object:
            assert list(g) == list(w), name
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), name


@pytest.mark.parametrize("family", ["raw", "typed"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_entry_point_accepts_or_rejects_the_shape_as_recorded(ex, world, family, shape):
    entries = RAW if family == "raw" else TYPED
    results = {}
    for entry, expect in zip(entries, MATRIX[shape][family]):
        if isinstance(expect, tuple):
            status, text = expect
            with pytest.raises(NutError) as e:
                run(ex, world, family, entry, shape)
            assert e.value.status == status and text in str(e.value), (entry, str(e.value))
            continue
        got = run(ex, world, family, entry, shape)
        want = world["want"][shape][expect]
        if shape == "b_star_scan" and family == "typed":
            want = world["star_typed"]
        same(got, want)
        results.setdefault(expect, []).append((entry, got))
    # the accepting entry points agree with each other, values and column order
    for group in results.values():
        first_entry, first = group[0]
        for entry, got in group[1:]:
            assert list(got) == list(first), (first_entry, entry)
            for name in first:
                assert list(got[name]) == list(first[name]), (first_entry, entry, name)
    assert results, "no entry point accepts the shape"


def test_a_ragged_typed_table_is_rejected_by_every_table_entry_point(ex, world):
    t = Table(ex, "CREATE TABLE t (a Int64, b Int64, k Int64)")
    r = world["raw"]["t"]
    t.append(a=r["a"], b=r["b"], k=r["k"][:-1])
    u = world["typed"]["u"]
    a, f = Plan(SHAPES["a_groupby"]), Plan(SHAPES["f_join"])
    for call in (lambda: t.execute(a), lambda: t.execute_join(a, u), lambda: t.execute_joins(a, []),
                 lambda: t.execute_join(f, u), lambda: t.execute_joins(f, [u])):
        with pytest.raises(NutError) as e:
            call()
        assert e.value.status == INVALID_ARG and "ragged" in str(e.value)
    t.free()


def test_a_missing_column_is_a_plan_error_for_a_table_and_an_unbound_one_for_raw_columns(ex, world):
    plan = Plan("select zz from t where a > 3")
    tt, tu = world["typed"]["t"], world["typed"]["u"]
    for call in (lambda: tt.execute(plan), lambda: tt.execute_join(plan, tu), lambda: tt.execute_joins(plan, []),
                 lambda: tt.execute_joins(plan, [tu])):
        with pytest.raises(NutError) as e:
            call()
        assert e.value.status == PLAN and "has no column 'zz'" in str(e.value)
    dt, du = world["dev"]["t"], world["dev"]["u"]
    for call in (lambda: plan.execute(ex, dt), lambda: plan.execute_join(ex, dt, du),
                 lambda: plan.execute_tables(ex, [dt]), lambda: plan.execute_tables(ex, [dt, du])):
        with pytest.raises(NutError) as e:
            call()
        assert e.value.status == INVALID_ARG and "'zz' is not bound" in str(e.value)
