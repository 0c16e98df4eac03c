"""GPU: narrow physical column types (Int8/16/32, UInt8/16/32, Float32; nut_type NUT_T_I32 ..
NUT_T_F32) read at their stored width by the three generated kernels (agg_kernel load_rows,
select_kernel, eval_kernel) and by nut_gather_typed.

The reference of every comparison is the same query over the same values widened on the
host (astype(int64) / astype(float64)) and run through the 8-byte path; numpy as well where
it is one line.  Widening is exact, so everything compares bit for bit: integer sums wrap,
f64 sums are over dyadic values (exact in any order), NaNs are the canonical quiet ones."""

import numpy as np
import pytest
import torch

from nutdb_amd import ProgQuery
from nutdb_amd import _lib as L

pytestmark = pytest.mark.gpu

INT_TYPES = [np.int32, np.int16, np.int8, np.uint32, np.uint16, np.uint8]
ALL_TYPES = INT_TYPES + [np.float32]
ROWS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 511, 513, 100_003]
QNAN, NQNAN = 0x7FC00000, 0xFFC00000  # the canonical quiet NaNs


def dev(x, ex):
    return torch.from_numpy(np.ascontiguousarray(x)).to(ex.device)


def widen(x):
    return x.astype(np.float64 if x.dtype.kind == "f" else np.int64)


def is_f(t):
    return np.dtype(t).kind == "f"


def make_cols(rng, t, n, slack=0):
    """predicate, key and value columns of n (+ slack) rows: p and v of type t, k of type t
    (int32 for Float32: float keys are not grouped).  Integer columns hold their type's
    minimum and maximum (rows 0..3 and the last two) where n leaves room; Float32 values
    are dyadic (k / 8), so every f64 sum is exact in any order."""
    m = n + slack
    kt = np.int32 if is_f(t) else t
    if is_f(t):
        p = (rng.integers(-400, 400, m) / 8.0).astype(t)
        v = (rng.integers(-1024, 1025, m) / 8.0).astype(t)
    else:
        lo, hi = max(np.iinfo(t).min, -50), min(np.iinfo(t).max, 50)
        p = rng.integers(lo, hi + 1, m).astype(t)
        v = rng.integers(lo, hi + 1, m).astype(t)
    k = rng.integers(0, 5, m).astype(kt)
    s = slack
    if n >= 2:
        k[s + 0], k[s + 1] = np.iinfo(kt).min, np.iinfo(kt).max
        p[s + 0] = p[s + 1] = 10  # both pass WHERE
    if n >= 6 and not is_f(t):
        p[s + 2], p[s + 3] = np.iinfo(t).min, np.iinfo(t).max
        v[m - 2], v[m - 1] = np.iinfo(t).min, np.iinfo(t).max
        p[m - 2] = p[m - 1] = 10
    return p, k, v


WHERE = [("col", 0), ("i64", 0, 3), ("gt",)]
EXPR = [("col", 2), ("i64", 0, 2), ("mul",), ("col", 0), ("add",)]
AGGS = [("sum", EXPR, None), ("min", EXPR, None), ("max", EXPR, None), ("count", None, None)]


def run(ex, keys, cols, where, aggs, hint):
    q = ProgQuery(keys=[k if isinstance(k, list) else dev(k, ex) for k in keys], cols=[dev(c, ex) for c in cols],
                  where=where, aggs=aggs, rows=len(cols[0]))
    g = ex.groupby(q, group_hint=hint)
    out = g.to_host_words()
    g.free()
    return out


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, got[0][:4], want[0][:4])
    assert np.array_equal(got[1], want[1]), (what, got[1][:4], want[1][:4])


# ------------------------------------------------------------------ 1. group-by through the ABI
@pytest.mark.parametrize("t", ALL_TYPES, ids=lambda t: np.dtype(t).name)
def test_groupby_each_type(ex, t):
    """WHERE on one column, a key, SUM / MIN / MAX / COUNT of an arithmetic expression, the
    three columns of type t; 0, 1 and 2 keys (the second a plain int64 key column); private
    accumulators (hint 8) and the shared table (hint 0); row counts around the pair, the
    four-row step, a wave, a workgroup and an odd tail."""
    rng = np.random.default_rng(7)
    for n in ROWS:
        p, k, v = make_cols(rng, t, n)
        k2 = rng.integers(0, 2, n).astype(np.int64)
        for nkeys in (0, 1, 2):
            keys = [[("col", 1)], k2][:nkeys]
            for hint in (8, 0):
                got = run(ex, keys, [p, k, v], WHERE, AGGS, hint)
                want = run(ex, keys, [widen(p), widen(k), widen(v)], WHERE, AGGS, hint)
                same(got, want, (n, nkeys, hint))
                sel = widen(p) > 3
                if nkeys == 0:
                    assert got[1][:, 3].sum() == sel.sum()
                elif sel.any():
                    # an unsigned maximum comes out as itself (4294967295, 255), not as -1
                    assert got[0][:, 0].min() == widen(k)[sel].min() and got[0][:, 0].max() == widen(k)[sel].max()
    kt = np.int32 if is_f(t) else t
    assert got[0][:, 0].max() == np.iinfo(kt).max and got[0][:, 0].min() == np.iinfo(kt).min


# ------------------------------------------------------------------ 2. alignment
@pytest.mark.parametrize("t", ALL_TYPES, ids=lambda t: np.dtype(t).name)
def test_groupby_misaligned_slices(ex, t):
    """t[1:] slices put an int8 column at an odd address, int16 at 2 mod 4, int32 / float32
    at 4 mod 8: their pairs are loaded per row, while the value column of the same type and
    an int64 column in the same launch keep their vector loads (the decision is per
    column)."""
    rng = np.random.default_rng(11)
    n = 100_003
    p, k, v = make_cols(rng, t, n, slack=1)
    w = rng.integers(-2**40, 2**40, n).astype(np.int64)
    dp, dk = dev(p, ex)[1:], dev(k, ex)[1:]
    dv, dw = dev(v[1:], ex), dev(w, ex)
    width = np.dtype(t).itemsize
    assert dp.data_ptr() % (2 * width) == width and dv.data_ptr() % 16 == 0 and dw.data_ptr() % 16 == 0
    expr = EXPR + [("col", 3), ("add",)]
    aggs = [("sum", expr, None), ("min", expr, None), ("max", expr, None), ("count", None, None)]
    for hint in (8, 0):
        q = ProgQuery(keys=[[("col", 1)]], cols=[dp, dk, dv, dw], where=WHERE, aggs=aggs)
        g = ex.groupby(q, group_hint=hint)
        got = g.to_host_words()
        g.free()
        want = run(ex, [[("col", 1)]], [widen(p[1:]), widen(k[1:]), widen(v[1:]), w], WHERE, aggs, hint)
        same(got, want, hint)
        assert got[1][:, 3].sum() == (widen(p[1:]) > 3).sum()


# ------------------------------------------------------------------ 3. Float32 values
def test_float32_special_values(ex):
    """+-0.0, a denormal (1e-40), +-3.0e38, +-inf and the canonical +-NaN: SUM, MIN, MAX and
    a comparison in WHERE.  A group holds one class of value, so its sum is the same in
    every order."""
    bits = lambda b: np.array([b], dtype=np.uint32).view(np.float32)[0]
    classes = [[np.float32(0.0), np.float32(-0.0)], [np.float32(1e-40)], [np.float32(3.0e38)], [np.float32(-3.0e38)],
               [np.float32(np.inf)], [np.float32(-np.inf)], [bits(QNAN), np.float32(1.5)], [bits(NQNAN), np.float32(-2.5)],
               [np.float32(1e-40), np.float32(-1e-40)]]
    assert np.float32(1e-40) != 0 and abs(np.float32(1e-40)) < np.finfo(np.float32).tiny  # a denormal
    rng = np.random.default_rng(3)
    n = 20_011
    key = rng.integers(0, len(classes), n).astype(np.int32)
    v = np.empty(n, dtype=np.float32)
    for c, vals in enumerate(classes):
        m = key == c
        v[m] = np.array(vals, dtype=np.float32)[rng.integers(0, len(vals), int(m.sum()))]
    w = np.roll(v, 1)
    # host widening keeps the canonical NaNs' sign and payload, as the device's does
    assert widen(np.array([bits(QNAN), bits(NQNAN)])).view(np.uint64).tolist() == [0x7FF8000000000000, 0xFFF8000000000000]
    where = [("col", 1), ("f64", 0, 0.0), ("ge",)]
    val = [("col", 0)]
    aggs = [("sum", val, None), ("min", val, None), ("max", val, None), ("count", None, None)]
    for hint in (8, 0):
        got = run(ex, [[("col", 2)]], [v, w, key], where, aggs, hint)
        want = run(ex, [[("col", 2)]], [widen(v), widen(w), widen(key)], where, aggs, hint)
        same(got, want, hint)
        sel = widen(w) >= 0.0  # NaN compares false, -0.0 and +inf true
        assert np.array_equal(got[1][:, 3], np.bincount(key[sel], minlength=len(classes))[got[0][:, 0]])
        s = got[1][:, 0].view(np.float64)
        g = {int(k): i for i, k in enumerate(got[0][:, 0])}
        assert s[g[1]] > 0 and s[g[1]] == widen(v)[sel & (key == 1)].sum()  # the denormals were not flushed
        assert s[g[4]] == np.inf and s[g[5]] == -np.inf and np.isnan(s[g[6]]) and np.isnan(s[g[7]])
        assert got[1][g[6], 2] == 0x7FF8000000000000 and got[1][g[7], 1] == 0xFFF8000000000000  # MAX / MIN: the NaNs


# ------------------------------------------------------------------ 4. sixteen int8 columns
def test_sixteen_int8_columns(ex):
    rng = np.random.default_rng(5)
    n = 10_007
    cols = [rng.integers(-128, 128, n).astype(np.int8) for _ in range(L.NUT_MAX_PROG_COLS)]
    total = [("col", 0)]
    for c in range(1, 16):
        total += [("col", c), ("add",)]
    where = [("col", 0), ("i64", 0, -100), ("gt",)]
    key = [("col", 15), ("i64", 0, 3), ("bitand",)]
    aggs = [("sum", total, None), ("min", total, None), ("max", total, None), ("count", None, None)]
    got = run(ex, [key], cols, where, aggs, 4)
    want = run(ex, [key], [widen(c) for c in cols], where, aggs, 4)
    same(got, want, "16 x int8")
    sel = cols[0] > -100
    tot = sum(widen(c) for c in cols)
    assert got[1][:, 0].view(np.int64).sum() == tot[sel].sum() and got[1][:, 3].sum() == sel.sum()


# ------------------------------------------------------------------ 5. large G: the partitioned path
def test_large_g_partitioned(ex, opts):
    """3e6 rows of an int32 key with 2e6 distinct values and a Float32 SUM through the
    spill -> partition -> aggregate path: its second phase reads staged 8-byte arrays under
    a spec of its own and must not inherit the narrow types."""
    opts(gb_partition=1)
    n, G = 3_000_000, 2_000_000
    rng = np.random.default_rng(17)
    key = ((np.arange(n, dtype=np.int64) * 7919) % G - G // 2).astype(np.int32)
    rng.shuffle(key)
    v = (rng.integers(-1024, 1025, n) / 8.0).astype(np.float32)
    aggs = [("sum", [("col", 1)], None), ("count", None, None), ("max", [("col", 1)], None)]
    got = run(ex, [[("col", 0)]], [key, v], None, aggs, G)
    assert ex.groupby_stats()["path"] != "onchip"
    want = run(ex, [[("col", 0)]], [widen(key), widen(v)], None, aggs, G)
    assert ex.groupby_stats()["path"] != "onchip"
    same(got, want, "large G")
    assert len(got[0]) == G and got[0][0, 0] == -(G // 2)
    assert np.array_equal(got[1][:, 1], np.bincount(widen(key) + G // 2, minlength=G))
    assert np.array_equal(got[1][:, 0].view(np.float64), np.bincount(widen(key) + G // 2, weights=widen(v), minlength=G))


# ------------------------------------------------------------------ 6. select_rows and eval_rows
@pytest.fixture(scope="module")
def scan_cols():
    rng = np.random.default_rng(23)
    n = 100_003
    a = rng.integers(-2**31, 2**31, n).astype(np.int32)
    b = (rng.integers(-1024, 1025, n) / 8.0).astype(np.float32)
    c = rng.integers(-128, 128, n).astype(np.int8)
    a[0], a[1], c[0], c[1] = np.iinfo(np.int32).min, np.iinfo(np.int32).max, -128, 127
    return a, b, c


@pytest.mark.parametrize("n", [1, 16383, 16384, 16385, 100_003])
def test_select_and_eval_rows(ex, scan_cols, n):
    """the scan's row ids (select tile: 16384 rows) and projections evaluated at them, with
    a CASE that is NULL where its mask fails"""
    a, b, c = (x[:n] for x in scan_cols)
    where = [("col", 0), ("i64", 0, 3), ("mod",), ("i64", 0, 0), ("eq",), ("col", 1), ("f64", 0, -64.0), ("gt",), ("and",)]
    narrow = [dev(x, ex) for x in (a, b, c)]
    wide = [dev(widen(x), ex) for x in (a, b, c)]
    ids = ex.select_rows(narrow, where)
    ref = ex.select_rows(wide, where)
    assert torch.equal(ids, ref)
    # numpy % is floored, the program's truncates: equal at remainder 0
    assert np.array_equal(ids.cpu().numpy(), np.flatnonzero((widen(a) % 3 == 0) & (widen(b) > -64.0)))
    progs = [([("col", 2), ("i64", 0, 2), ("mul",), ("col", 0), ("add",)], [("col", 1), ("f64", 0, 0.0), ("gt",)]),
             ([("col", 1), ("col", 2), ("mul",)], None)]
    for rows in (ids, None):
        got, gv = ex.eval_rows(narrow, progs, rows)
        want, wv = ex.eval_rows(wide, progs, rows)
        r = ids.cpu().numpy() if rows is not None else np.arange(n)
        for j in range(2):
            assert torch.equal(got[j], want[j]) and torch.equal(gv[j], wv[j])
        ok = widen(b)[r] > 0.0
        assert np.array_equal(gv[0].cpu().numpy(), ok.astype(np.uint8)) and bool(gv[1].all())
        assert np.array_equal(got[0].cpu().numpy(), np.where(ok, widen(c)[r] * 2 + widen(a)[r], 0))
        assert np.array_equal(got[1].cpu().numpy().view(np.float64), widen(b)[r] * widen(c)[r])


# ------------------------------------------------------------------ 7. gather
@pytest.mark.parametrize("t", ALL_TYPES, ids=lambda t: np.dtype(t).name)
def test_gather_typed(ex, t):
    rng = np.random.default_rng(29)
    m = 5_003
    if is_f(t):
        src = (rng.integers(-1024, 1025, m) / 8.0).astype(t)
        src[:6] = np.array([0x00000001, 0x80000001, QNAN, NQNAN, 0x7F800000, 0x80000000], dtype=np.uint32).view(t)
        null = -7.5
    else:
        src = rng.integers(np.iinfo(t).min, int(np.iinfo(t).max) + 1, m).astype(t)
        src[0], src[1] = np.iinfo(t).min, np.iinfo(t).max
        null = -99
    idx = rng.integers(-m // 4, m, 20_001).astype(np.int64)
    idx[:8] = [0, 1, 2, 3, 4, 5, -1, m - 1]
    got = ex.gather(dev(src, ex), dev(idx, ex), null=null).cpu().numpy()
    want = np.where(idx < 0, null, widen(src)[np.maximum(idx, 0)])
    assert got.dtype == want.dtype and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    for n in (0, 1, 1025):  # no index: the widening pass
        got = ex.gather(dev(src[:n], ex), None).cpu().numpy()
        assert np.array_equal(got.view(np.uint64), widen(src[:n]).view(np.uint64))


def test_gather_typed_abi_forwards_8_byte_types(ex):
    """for NUT_T_I64 / NUT_T_F64 nut_gather_typed is nut_gather_u64 (and a copy without an
    index); an unknown type is NUT_ERR_INVALID_ARG"""
    src = dev(np.arange(100, dtype=np.int64) * 3, ex)
    idx = dev(np.array([5, -1, 99, 0], dtype=np.int64), ex)
    out = torch.empty(4, dtype=torch.int64, device=ex.device)
    L.check(L.lib.nut_gather_typed(ex.ctx, src.data_ptr(), L.T_I64, idx.data_ptr(), 4, 77, out.data_ptr()), "gather")
    ex.sync()
    assert out.tolist() == [15, 77, 297, 0]
    out = torch.empty(100, dtype=torch.int64, device=ex.device)
    L.check(L.lib.nut_gather_typed(ex.ctx, src.data_ptr(), L.T_F64, None, 100, 0, out.data_ptr()), "gather")
    ex.sync()
    assert torch.equal(out, src)
    assert L.lib.nut_gather_typed(ex.ctx, src.data_ptr(), L.T_STR, idx.data_ptr(), 4, 0, out.data_ptr()) == 1


# ------------------------------------------------------------------ 10. virtual ranks
def test_virtual_ranks_int32_program_column(ex):
    """nut_dist_groupby passes the spec through: two virtual ranks over row shards of an
    int32 key / Float32 value pair give the single-context result"""
    from nutdb_amd.dist import NutDist
    rng = np.random.default_rng(31)
    n = 200_003
    key = rng.integers(-500, 500, n).astype(np.int32)
    v = (rng.integers(-1024, 1025, n) / 8.0).astype(np.float32)
    aggs = [("sum", [("col", 1)], None), ("count", None, None), ("min", [("col", 0)], None)]
    want = run(ex, [[("col", 0)]], [key, v], None, aggs, 1000)
    d = NutDist.virtual(2)
    try:
        qs = [ProgQuery(keys=[[("col", 0)]], cols=[dev(key[a:b], ex), dev(v[a:b], ex)], aggs=aggs)
              for a, b in ((0, n // 2), (n // 2, n))]
        out = d.groupby(qs, group_hint=1000)
        got = out[0].to_host_words()
        out[0].free()
    finally:
        d.close()
    same(got, want, "virtual ranks")
    assert np.array_equal(got[1][:, 1], np.bincount(widen(key) + 500, minlength=1000)[got[0][:, 0] + 500])


# ------------------------------------------------------------------ 8. SQL over narrow tensors
def sql_both(ex, q, cols, right=None, hint=0):
    """the query over narrow tensors and over the same values widened on the host"""
    d = lambda t: {k: dev(v, ex) for k, v in t.items()}
    w = lambda t: {k: dev(widen(v), ex) for k, v in t.items()}
    got = ex.sql(q, d(cols), group_hint=hint, right=d(right) if right else None)
    want = ex.sql(q, w(cols), group_hint=hint, right=w(right) if right else None)
    assert list(got) == list(want), q
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (q, k, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint64) if a.dtype.itemsize == 8 else a,
                              b.view(np.uint64) if b.dtype.itemsize == 8 else b), (q, k)
    return got


@pytest.mark.parametrize("tx,ty", [(np.int32, np.int8), (np.float32, np.int16), (np.uint8, np.float32)],
                         ids=["i32-i8", "f32-i16", "u8-f32"])
def test_sql_over_narrow_tensors(ex, tx, ty):
    rng = np.random.default_rng(41)
    n = 50_021

    def col(t):
        if is_f(t):
            return (rng.integers(-64, 65, n) / 8.0).astype(t)
        return rng.integers(max(np.iinfo(t).min, -20), min(np.iinfo(t).max, 20) + 1, n).astype(t)
    t = {"x": col(tx), "y": col(ty)}
    got = sql_both(ex, "select x from t where x < 3", t)
    assert np.array_equal(got["x"], widen(t["x"])[widen(t["x"]) < 3])
    got = sql_both(ex, "select x from t where x < 3 order by x desc limit 100 offset 5", t)
    assert np.array_equal(got["x"], np.sort(widen(t["x"])[widen(t["x"]) < 3])[::-1][5:105])
    sql_both(ex, "select x, y from t order by y desc, x", t)
    sql_both(ex, "select y, sum(x), min(x), count(*) from t group by y having count(*) > 5 order by y", t, hint=64)
    got = sql_both(ex, "select distinct y from t", t, hint=64)
    assert sorted(got["y"].tolist()) == sorted(set(widen(t["y"]).tolist()))
    sql_both(ex, "select y, sum(x * 2), max(x) from t where x > -2 group by y order by y", t, hint=64)


def test_sql_float32_group_key_zeros_and_nans(ex):
    """a Float32 GROUP BY key: -0.0 and +0.0 are one group, the NaNs one group"""
    rng = np.random.default_rng(43)
    n = 20_003
    pool = np.array([0x00000000, 0x80000000, QNAN, NQNAN, 0x3FC00000, 0xC0200000], dtype=np.uint32).view(np.float32)
    t = {"y": pool[rng.integers(0, len(pool), n)], "x": rng.integers(-100, 100, n).astype(np.int32)}
    got = sql_both(ex, "select y, sum(x), count(*) from t group by y order by y", t, hint=16)
    assert len(got["y"]) == 4 and int(np.sum(got["count()"] if "count()" in got else list(got.values())[2])) == n


def test_sql_join_int32_keys(ex):
    rng = np.random.default_rng(47)
    n, m = 30_011, 2_003
    left = {"a": rng.integers(0, m, n).astype(np.int32), "v": (rng.integers(-64, 65, n) / 8.0).astype(np.float32)}
    right = {"b": rng.permutation(m).astype(np.int32), "g": rng.integers(0, 7, m).astype(np.int8)}
    sql_both(ex, "select g, sum(v), count(*) from l join r on a = b group by g order by g", left, right=right, hint=16)


# ------------------------------------------------------------------ 9. typed tables
Q1_DDL = """CREATE TABLE lineitem (l_returnflag Enum('A' = 0, 'N' = 1, 'R' = 2), l_linestatus String,
    l_quantity Int8, l_extendedprice Float32, l_discount Float32, l_shipdate Date, l_ok Boolean, l_part UInt16,
    l_supp Int32, l_big Int64)"""


def test_narrow_table_matches_wide_table(ex):
    """Table(narrow=True) against Table() with the same appends: Q1 over Enum / String / Int8 /
    Float32 / Date columns, scans and the widening extremes give identical results"""
    from nutdb_amd import NutError
    from nutdb_amd.table import Table
    rng = np.random.default_rng(53)
    n = 40_009
    data = dict(
        l_returnflag=np.array(["A", "N", "R"])[rng.integers(0, 3, n)].tolist(),
        l_linestatus=np.array(["F", "O"])[rng.integers(0, 2, n)].tolist(),
        l_quantity=rng.integers(-128, 128, n).astype(np.int8),
        l_extendedprice=(rng.integers(0, 8192, n) / 8.0).astype(np.float32),
        l_discount=(rng.integers(0, 9, n) / 64.0).astype(np.float32),
        l_shipdate=rng.integers(8036, 10562, n).astype(np.int64),
        l_ok=rng.integers(0, 2, n).astype(np.uint8),
        l_part=rng.integers(0, 65536, n).astype(np.uint16),
        l_supp=rng.integers(-2**31, 2**31, n).astype(np.int32),
        l_big=rng.integers(-2**62, 2**62, n).astype(np.int64))
    for k, lo, hi in (("l_quantity", -128, 127), ("l_part", 0, 65535), ("l_supp", -2**31, 2**31 - 1)):
        data[k][0], data[k][1] = lo, hi
    data["l_extendedprice"][:2] = np.array([0x00000001, 0x7F7FFFFF], dtype=np.uint32).view(np.float32)
    tables = []
    for narrow in (False, True):
        t = Table(ex, Q1_DDL, narrow=narrow)
        half = n // 2
        t.append(**{k: v[:half] for k, v in data.items()})
        t.append(**{k: v[half:] for k, v in data.items()})
        tables.append(t)
    wide, nar = tables
    assert nar.exec_types()["l_quantity"] == L.T_I8 and wide.exec_types()["l_quantity"] == L.T_I64
    with pytest.raises(NutError, match="already has rows"):
        nar.set_narrow(False)
    queries = [
        "select l_returnflag, l_linestatus, sum(l_quantity), sum(l_extendedprice), "
        "sum(l_extendedprice * (1 - l_discount)), count(*) from lineitem where l_shipdate <= 10471 "
        "group by l_returnflag, l_linestatus order by l_returnflag, l_linestatus",
        "select l_quantity, count(*), min(l_supp), max(l_part) from lineitem where l_ok = 1 group by l_quantity "
        "order by l_quantity",
        "select l_supp, l_part, l_extendedprice from lineitem where l_quantity > 120 order by l_supp desc, l_part",
        "select min(l_quantity), max(l_quantity), min(l_part), max(l_part), min(l_supp), max(l_supp), "
        "min(l_extendedprice), max(l_extendedprice) from lineitem",
        "select l_part from lineitem where l_part >= 65000 order by l_part desc limit 20",
        "select l_linestatus, sum(l_extendedprice) from lineitem where l_returnflag = 'N' group by l_linestatus "
        "order by l_linestatus",
    ]
    for q in queries:
        a, b = nar.sql(q, group_hint=64), wide.sql(q, group_hint=64)
        assert list(a) == list(b), q
        for k in b:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.dtype == y.dtype and x.shape == y.shape, (q, k)
            if x.dtype.kind in "fiu" and x.dtype.itemsize == 8:
                assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (q, k)
            else:
                assert np.array_equal(x, y), (q, k)
    ext = nar.sql(queries[3])
    vals = [np.asarray(v)[0] for v in ext.values()]
    assert vals[:6] == [-128, 127, 0, 65535, -2**31, 2**31 - 1]
    for t in tables:
        t.free()
