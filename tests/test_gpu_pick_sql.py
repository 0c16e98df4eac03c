"""GPU: any / anyLast / argMin / argMax through SQL, against pandas / numpy
over about 3e5 rows: the picked row is the one with the extreme order value among the group's
rows passing WHERE, ties to the lowest row; any / anyLast are the first / last such row.  Every
value is a value of one row, so every comparison is exact (float64 by bits)."""
import numpy as np
import pandas as pd
import pytest
import torch

from nutdb_amd import NutError
from nutdb_amd.sql import Plan
from nutdb_amd.table import Table

pytestmark = pytest.mark.gpu

N = 300_007


def make():
    rng = np.random.default_rng(314)
    c = dict(
        k=rng.integers(-20, 20, N), j=rng.integers(0, 5, N), l=rng.integers(0, 3, N),
        a=rng.integers(-10**12, 10**12, N), af=rng.integers(-10**6, 10**6, N) / 64.0,
        b=rng.integers(0, 2000, N),              # many ties per group
        bf=rng.integers(-4000, 4000, N) / 8.0,
        d=rng.integers(9000, 9400, N),           # day numbers
        c=rng.integers(0, 1000, N),
        z=np.where(rng.random(N) < 0.001, 0, rng.integers(1, 9, N)),  # a divisor, rarely zero
        one=np.ones(N, np.int64),
        fk=rng.integers(-6, 6, N) / 4.0,         # a Float64 key
    )
    return {n: np.ascontiguousarray(v, dtype=np.float64 if v.dtype.kind == "f" else np.int64) for n, v in c.items()}


@pytest.fixture(scope="module")
def data(ex):
    host = make()
    dev = {n: torch.from_numpy(v).to(ex.device) for n, v in host.items()}
    df = pd.DataFrame(host)
    df["pos"] = np.arange(N)
    return host, dev, df


def picked(df, keys, order, want_max):
    """per group (sorted by key tuple) the position of the row of extreme `order`, ties to the
    lowest position; order None: the first / last row.  No keys: one position."""
    if order is None:
        d = df
        agg = "last" if want_max else "first"
    else:
        d = df.sort_values([order, "pos"], ascending=[not want_max, True], kind="stable")
        agg = "first"
    if not keys:
        return np.array([getattr(d["pos"], "iloc")[-1 if (order is None and want_max) else 0]])
    return getattr(d.groupby(keys, sort=True)["pos"], agg)().to_numpy()


def bits(x):
    return np.ascontiguousarray(x).view(np.int64) if x.dtype == np.float64 else x


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want)), (got[:6], want[:6])


@pytest.mark.parametrize("a", ["a", "af"])
@pytest.mark.parametrize("b", ["b", "bf", "d"])
def test_all_four_next_to_sum_and_count(ex, data, a, b):
    host, dev, df = data
    got = Plan(f"select k, argMax({a}, {b}) as amax, argMin({a}, {b}) as amin, any({a}) as fst, anyLast({a}) as lst, "
               f"sum(a) as s, count() as n from t where c > 100 group by k").execute(ex, dev, types={"d": "date"})
    w = df[df.c > 100]
    g = w.groupby("k", sort=True)
    same(got["k"], np.array(sorted(w.k.unique())))
    same(got["amax"], host[a][picked(w, ["k"], b, True)])
    same(got["amin"], host[a][picked(w, ["k"], b, False)])
    same(got["fst"], host[a][picked(w, ["k"], None, False)])
    same(got["lst"], host[a][picked(w, ["k"], None, True)])
    same(got["s"], g.a.sum().to_numpy())
    same(got["n"], g.size().to_numpy())


def test_no_keys(ex, data):
    host, dev, df = data
    got = ex.sql("select argMax(af, b) as x, argMin(a, bf) as y, any(a) as f, anyLast(af) as l from t where c >= 500", dev)
    w = df[df.c >= 500]
    same(got["x"], host["af"][picked(w, [], "b", True)])
    same(got["y"], host["a"][picked(w, [], "bf", False)])
    same(got["f"], host["a"][picked(w, [], None, False)])
    same(got["l"], host["af"][picked(w, [], None, True)])
    got = ex.sql("select argMax(af, b) as x, any(a) as f, count() as n from t", dev)  # no WHERE: no row-id pass
    same(got["x"], host["af"][picked(df, [], "b", True)])
    same(got["f"], host["a"][:1])


def test_no_rows(ex, data):
    """a WHERE selecting no rows: a global aggregate is one row of defaults, a grouped one empty"""
    host, dev, df = data
    got = ex.sql("select argMax(af, b) as x, argMin(a, bf) as y, any(a) as f, count() as n from t where c > 5000", dev)
    same(got["x"], np.array([0.0]))
    same(got["y"], np.array([0]))
    same(got["f"], np.array([0]))
    same(got["n"], np.array([0]))
    got = ex.sql("select k, any(a) as f from t where c > 5000 group by k", dev)
    assert len(got["k"]) == 0 and len(got["f"]) == 0


def test_three_packed_keys(ex, data):
    host, dev, df = data
    got = ex.sql("select k, j, l, argMax(a, bf) as x, anyLast(af) as y from t where c < 700 group by k, j, l", dev)
    w = df[df.c < 700]
    same(got["x"], host["a"][picked(w, ["k", "j", "l"], "bf", True)])
    same(got["y"], host["af"][picked(w, ["k", "j", "l"], None, True)])
    assert len(got["x"]) == 40 * 5 * 3


def test_computed_key(ex, data):
    host, dev, df = data
    got = ex.sql("select k % 7 as r, argMin(af, b * 2 + j) as x, any(a) as y from t group by k % 7", dev)
    w = df.assign(r=np.fmod(df.k, 7), o=df.b * 2 + df.j)
    same(got["r"], np.array(sorted(w.r.unique())))
    same(got["x"], host["af"][picked(w, ["r"], "o", False)])
    same(got["y"], host["a"][picked(w, ["r"], None, False)])


def test_float64_key(ex, data):
    host, dev, df = data
    got = ex.sql("select fk, argMax(a, b) as x, argMin(af, d) as y from t where c != 3 group by fk", dev)
    w = df[df.c != 3]
    same(got["fk"], np.array(sorted(w.fk.unique())))
    same(got["x"], host["a"][picked(w, ["fk"], "b", True)])
    same(got["y"], host["af"][picked(w, ["fk"], "d", False)])


def test_typed_table_strings_datetime_narrow(ex):
    rng = np.random.default_rng(77)
    n = 120_011
    names = np.array([f"supplier#{i:04d}" for i in range(300)], dtype=object)
    regions = np.array(["ASIA", "EUROPE", "AFRICA", "AMERICA"], dtype=object)
    cols = dict(s_name=names[rng.integers(0, 300, n)], region=regions[rng.integers(0, 4, n)],
                ts=rng.integers(1_500_000_000, 1_500_000_000 + 86400 * 30, n),
                cost=rng.integers(-2**31, 2**31, n).astype(np.int32), q=rng.integers(0, 200, n).astype(np.uint8))
    t = Table(ex, "CREATE TABLE ps (s_name String, region Dictionary(String), ts Datetime, cost Int32, q UInt8)",
              narrow=True)
    t.append(**cols)
    df = pd.DataFrame(dict(cols, pos=np.arange(n)))
    df["hour"] = (cols["ts"] // 3600) % 24
    got = t.sql("select region, argMax(s_name, ts) as latest, argMin(s_name, cost) as cheapest, any(s_name) as f, "
                "anyLast(q) as lq, argMax(cost, toHour(ts)) as ch, max(ts) as mts from ps where q > 10 group by region "
                "order by region")
    w = df[df.q > 10]
    assert got["region"].tolist() == sorted(regions.tolist())
    assert got["latest"].tolist() == cols["s_name"][picked(w, ["region"], "ts", True)].tolist()
    assert got["cheapest"].tolist() == cols["s_name"][picked(w, ["region"], "cost", False)].tolist()
    assert got["f"].tolist() == cols["s_name"][picked(w, ["region"], None, False)].tolist()
    assert got["lq"].tolist() == cols["q"][picked(w, ["region"], None, True)].astype(np.int64).tolist()
    assert got["ch"].tolist() == cols["cost"][picked(w, ["region"], "hour", True)].astype(np.int64).tolist()
    # a string result: no keys, no rows ('' by default), ORDER BY it, and the refusals of a string key
    got = t.sql("select argMax(s_name, ts) as s, any(region) as r from ps where q > 250")
    assert got["s"].tolist() == [""] and got["r"].tolist() == [""]
    got = t.sql("select region, argMin(s_name, ts) as s from ps group by region order by s desc")
    want = sorted(cols["s_name"][picked(df, ["region"], "ts", False)].tolist(), reverse=True)
    assert got["s"].tolist() == want
    for sql, frag in (("select region, argMax(s_name, ts) + 1 from ps group by region", "arithmetic on the string"),
                      ("select region from ps group by region having any(s_name) > 1", "HAVING on the string"),
                      ("select region, argMax(q, s_name) from ps group by region", "argMax: the order 's_name' is a string"),
                      ("select argMin(q, region) from ps", "argMin: the order 'region' is a string")):
        with pytest.raises(NutError) as e:
            t.sql(sql)
        assert e.value.status == 7 and frag in str(e.value), str(e.value)


def test_having_order_by_arithmetic(ex, data):
    host, dev, df = data
    got = ex.sql("select k, argMax(a, b) as x, argMax(a, b) - min(a) as spread from t where c > 50 group by k "
                 "having argMax(a, b) > 0 and anyLast(j) < 4 order by argMax(a, b) desc, k", dev)
    w = df[df.c > 50]
    ks = np.array(sorted(w.k.unique()))
    x = host["a"][picked(w, ["k"], "b", True)]
    lj = host["j"][picked(w, ["k"], None, True)]
    mn = w.groupby("k", sort=True).a.min().to_numpy()
    keep = (x > 0) & (lj < 4)
    order = np.lexsort((ks[keep], -x[keep]))
    assert 0 < keep.sum() < len(ks)
    same(got["k"], ks[keep][order])
    same(got["x"], x[keep][order])
    same(got["spread"], (x - mn)[keep][order])
    assert set(got) == {"k", "x", "spread"}  # the HAVING-only outputs stay hidden


def test_union_derived_cte_scalar_subquery(ex, data):
    host, dev, df = data
    got = ex.sql("select k, argMax(a, b) as v from t where c < 300 group by k union all "
                 "select j, anyLast(a) from t group by j", dev)
    w = df[df.c < 300]
    want = np.concatenate([host["a"][picked(w, ["k"], "b", True)], host["a"][picked(df, ["j"], None, True)]])
    same(got["v"], want)
    per_k = host["af"][picked(df, ["k"], "d", False)]
    got = ex.sql("select count() as n, max(v) as s from (select k, argMin(af, d) as v from t group by k) as q where v > 0", dev)
    same(got["n"], np.array([int((per_k > 0).sum())]))
    same(got["s"], np.array([per_k[per_k > 0].max()]))
    got = ex.sql("with q as (select k, argMin(af, d) as v from t group by k) select k, v from q where v <= 0 order by k", dev)
    same(got["v"], per_k[per_k <= 0])
    top = int(host["a"][picked(df, [], "b", True)][0])
    got = ex.sql("select count() as n from t where a > (select argMax(a, b) from t)", dev)
    same(got["n"], np.array([int((host["a"] > top).sum())]))


def test_division_by_zero(ex, data):
    host, dev, df = data
    assert (host["z"] == 0).sum() > 50
    # in the value: only a picked row matters.  Order by a column that puts a z != 0 row first ...
    o = np.where(host["z"] == 0, 0, host["b"] + 1)
    dev2 = dict(dev, o=torch.from_numpy(o).to(ex.device))
    got = ex.sql("select k, argMax(intDiv(a, z), o) as q from t group by k", dev2)
    rows = picked(df.assign(o=o), ["k"], "o", True)
    assert (host["z"][rows] != 0).all()
    same(got["q"], np.sign(host["a"][rows]) * (np.abs(host["a"][rows]) // host["z"][rows]))  # intDiv truncates
    # ... and one that picks a zero divisor in some group
    with pytest.raises(NutError) as e:
        ex.sql("select k, argMin(intDiv(a, z), o) as q from t group by k", dev2)
    assert e.value.status == 1 and "division by zero" in str(e.value)
    # in the order: any row passing WHERE fails the query, no row failing it does
    with pytest.raises(NutError) as e:
        ex.sql("select k, argMax(a, intDiv(b, z)) as q from t group by k", dev)
    assert e.value.status == 1 and "division by zero" in str(e.value)
    got = ex.sql("select k, argMax(a, intDiv(b, z)) as q from t where z != 0 group by k", dev)
    w = df[df.z != 0]
    same(got["q"], host["a"][picked(w.assign(o=w.b // w.z), ["k"], "o", True)])


def test_heavy_ties(ex, data):
    host, dev, df = data
    got = ex.sql("select j, argMax(af, one) as x, argMin(a, one) as y from t where c > 900 group by j", dev)
    w = df[df.c > 900]
    first = picked(w, ["j"], None, False)
    same(got["x"], host["af"][first])
    same(got["y"], host["a"][first])
    got = ex.sql("select argMin(a, one * 3) as y from t", dev)
    same(got["y"], host["a"][:1])
