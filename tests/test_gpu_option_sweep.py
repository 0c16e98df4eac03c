"""GPU parity under every nut_ctx option value (include/nutexec.h: "Results never depend on
them").  Most options select another kernel instantiation, tile shape, table geometry or
grid; tests/option_sweep.py lists the values of each, and test_option_value runs, for every
(option, value), a workload that reads the option and compares the result with the oracle
or numpy.  Where the library reports what it did (nut_ctx_groupby_stats, nut_ctx_sort_stats,
nut_ctx_priv_shape, nut_ctx_groupby_overflow) the workload also checks that the option was
in force.

Comparisons are the project's own: integers, counts, MIN / MAX, row ids and join pairs bit
for bit; f64 sums bit for bit wherever the values are dyadic (generator kind 3, small
integers, k / 64 fractions: exact in any order, so every launch shape must give identical
words), else within helpers.F64_SUM_RTOL.  Inputs and their oracle results are made once
per module and shared by the cases (never modified)."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_gorder as gorder
import test_gpu_join as tjoin
import test_gpu_narrow as narrow
import test_gpu_probe as tprobe
from helpers import OPCODE
from option_sweep import NOT_MEMBERS, SWEEP, source_tables
from test_gpu_exec import AGGS4, I64_MAX, I64_MIN, check_vs_oracle, dev, gb_query, host

pytestmark = pytest.mark.gpu

TABLE = source_tables()
DEFAULT = {name: t[2] for name, t in TABLE.items()}
CASES = [(name, v) for name, vals in SWEEP.items() for v in vals]

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _CACHE.clear()


EXACT4 = ["i", "i", "i", "i"]  # check_vs_oracle: every word bit for bit (dyadic sums)


# ----------------------------------------------------------------------------- Q1 (priv_*)
Q1_AGGS = [(0, 0, (0,)), (0, 0, (1,)), (0, 4, (1, 2)), (1, 0, ())]
Q1_N = 2_100_003  # > 2 workgroups per CU at every shape, a ragged last tile
Q1_SMALL = 1_003  # fewer pairs than one workgroup


def q1_dyadic(ex, orc, n, nflag=3, nstatus=2):
    """Q1 columns whose three f64 sums are exact in any order: integer quantities and
    prices, discounts k / 64 (price * (1 - disc) is an integer / 64, far below 2^53)."""
    from nutdb_amd.workloads import Q1_DATE_K

    def make():
        rng = np.random.default_rng(1000 * nflag + n % 997)
        hcols = [rng.integers(8036, 10562, n).astype(np.int64), rng.integers(0, nflag, n).astype(np.int64),
                 rng.integers(0, nstatus, n).astype(np.int64), rng.integers(1, 51, n).astype(np.float64),
                 rng.integers(900, 104950, n).astype(np.float64), rng.integers(0, 7, n) / 64.0]
        sd, rf, ls, qty, price, disc = hcols
        ok, ow = orc.groupby([rf, ls], Q1_AGGS, values=[qty, price, disc], preds=[(sd, OPCODE["<="], Q1_DATE_K)])
        return hcols, [dev(x, ex) for x in hcols], ok, ow
    return cached(("q1", n, nflag, nstatus), make)


def q1_exact(ex, dcols, ok, ow, what):
    from nutdb_amd.workloads import Q1_DATE_K
    g = ex.q1(*dcols, date_k=Q1_DATE_K)
    keys, words = g.to_host_words()
    g.free()
    assert np.array_equal(keys, ok), what
    assert np.array_equal(words, ow), what


def shape_in_force(ex, bd, blocks):
    s = ex.priv_shape()
    assert s["threads"] == bd if bd else s["threads"] in (128, 192), s
    assert s["blocks_per_cu"] == blocks if blocks else s["blocks_per_cu"] in (2, 3, 4), s


@pytest.mark.parametrize("blocks", SWEEP["priv_blocks"])
@pytest.mark.parametrize("bd", SWEEP["priv_bd"])
def test_q1_priv_shapes(ex, orc, opts, bd, blocks):
    """The fused Q1 kernel at every threads x workgroups-per-CU combination — the three
    shapes the launch-shape probe (NUT_OPT_PRIV_PROBE) chooses among at >= 2^27 rows are
    192 x 2, 128 x 3 and 128 x 4 — bit-equal to the oracle on dyadic columns."""
    opts(priv_bd=bd, priv_blocks=blocks)
    shape_in_force(ex, bd, blocks)
    for n in (Q1_N, Q1_SMALL):
        _, dcols, ok, ow = q1_dyadic(ex, orc, n)
        assert len(ok) == 6
        q1_exact(ex, dcols, ok, ow, (bd, blocks, n))


Q1_SQL = """select l_returnflag, l_linestatus, sum(l_quantity) as q, sum(l_extendedprice) as p,
    sum(l_extendedprice * (1 - l_discount)) as d, count(*) as c
  from lineitem where {} group by l_returnflag, l_linestatus"""


def w_priv_bd(ex, orc, opts, v):
    from nutdb_amd.workloads import Q1_COLS, Q1_DATE_K, gen
    # the reference of the narrow-column query: the widened columns at the default shape
    rng = np.random.default_rng(7)
    ncols = {t: narrow.make_cols(rng, t, 100_003) for t in (np.int32, np.float32)}
    want = {t: cached(("narrow", t), lambda: narrow.run(ex, [[("col", 1)]], [narrow.widen(c) for c in ncols[t]],
                                                         narrow.WHERE, narrow.AGGS, 8))
            for t in ncols}
    opts(priv_bd=v)
    shape_in_force(ex, v, 0)
    hcols, dcols, ok, ow = q1_dyadic(ex, orc, Q1_N)
    q1_exact(ex, dcols, ok, ow, "six groups")
    # 12 (flag, status) pairs: more groups than the 8 private accumulators, so the rest
    # go through the LDS table inside the private kernel
    _, dcols12, ok12, ow12 = q1_dyadic(ex, orc, Q1_N, nflag=4, nstatus=3)
    assert len(ok12) == 12
    q1_exact(ex, dcols12, ok12, ow12, "twelve groups")
    # 8-byte but not 16-byte aligned columns leave the fused kernel (two 8-B loads per pair)
    shifted = [dev(np.concatenate([x[:1], x]), ex)[1:] for x in hcols]
    assert all(t.data_ptr() % 16 == 8 for t in shifted)
    q1_exact(ex, shifted, ok, ow, "misaligned")
    # the generator's non-dyadic columns (test_q1_vs_oracle_large's), within F64_SUM_RTOL
    gcols, gok, gow = cached("q1gen", lambda: _q1_generated(ex, orc, Q1_COLS, Q1_DATE_K, gen))
    g = ex.q1(*gcols, date_k=Q1_DATE_K)
    check_vs_oracle(g, gok, gow, ["sum_f64", "sum_f64", "sum_f64", "i"])
    g.free()
    # expression mode: every run-time-compiled private kernel is built with this bd.  The
    # compiled SQL Q1 (an OR in WHERE leaves the fused shape) equals the fused one word for
    # word on the dyadic columns, and both equal the oracle
    named = {s[0]: t for s, t in zip(Q1_COLS, dcols)}
    fused = ex.sql(Q1_SQL.format("l_shipdate <= 10471"), named, group_hint=6)
    comp = ex.sql(Q1_SQL.format("l_shipdate <= 10471 or l_quantity < 0"), named, group_hint=6)
    for got in (fused, comp):
        assert np.array_equal(got["l_returnflag"], ok[:, 0]) and np.array_equal(got["l_linestatus"], ok[:, 1])
        assert np.array_equal(got["c"].astype(np.uint64), ow[:, 3])
        for j, name in enumerate(("q", "p", "d")):
            assert np.array_equal(np.ascontiguousarray(got[name]).view(np.uint64), ow[:, j]), name
    # ... and a query over narrow columns (Int32, Float32: test_gpu_narrow's), bit for bit
    for t, cols in ncols.items():
        narrow.same(narrow.run(ex, [[("col", 1)]], list(cols), narrow.WHERE, narrow.AGGS, 8), want[t], (v, t))
        sel = narrow.widen(cols[0]) > 3
        assert int(want[t][1][:, 3].sum()) == int(sel.sum())


def _q1_generated(ex, orc, Q1_COLS, Q1_DATE_K, gen):
    gcols = [gen(ex, spec, Q1_N) for spec in Q1_COLS]
    sd, rf, ls, qty, price, disc = [orc.gen(spec, Q1_N) for spec in Q1_COLS]
    ok, ow = orc.groupby([rf, ls], Q1_AGGS, values=[qty, price, disc], preds=[(sd, OPCODE["<="], Q1_DATE_K)])
    return gcols, ok, ow


def w_priv_blocks(ex, orc, opts, v):
    opts(priv_blocks=v)
    shape_in_force(ex, 0, v)
    for n in (Q1_N, Q1_SMALL):
        _, dcols, ok, ow = q1_dyadic(ex, orc, n)
        q1_exact(ex, dcols, ok, ow, (v, n))


def w_priv_probe(ex, orc, opts, v):
    """The probe runs only at >= 2^27 rows (test_gpu_fullsize.py checks its three candidate
    shapes there); here: the option changes nothing about a small Q1."""
    opts(priv_probe=v)
    _, dcols, ok, ow = q1_dyadic(ex, orc, Q1_N)
    q1_exact(ex, dcols, ok, ow, v)


# ----------------------------------------------------------------------------- group-by
GB_N = 3_000_017


def gb_data(ex, orc, G, n=GB_N):
    """Pool keys, dyadic values (every sum exact) and the oracle's groups."""
    def make():
        key = orc.gen_column(2, 0x51, n, a=G)
        val = orc.gen_column(3, 0x52, n)
        ok, ow = orc.groupby([key], AGGS4, values=[val])
        return dev(key, ex), dev(val, ex), ok, ow
    return cached(("gb", G, n), make)


def gb_exact(ex, data, hint, preds=()):
    kd, vd, ok, ow = data
    g = ex.groupby(gb_query(kd, vd, preds), group_hint=hint)
    st = ex.groupby_stats()
    assert len(g) == len(ok)
    check_vs_oracle(g, ok, ow, EXACT4)
    g.free()
    return st


def _onchip(ex, orc, opts):
    """The shared-table streaming kernel: exact hints, a hint four times too low (the on-chip
    table overflows into the global one: a wrong hint costs speed, never correctness), a
    table that cannot hold the groups at all and no hint."""
    opts(gb_partition=0)
    for G, hint in [(1000, 1000), (1000, 250), (20_000, 20_000), (20_000, 0)]:
        st = gb_exact(ex, gb_data(ex, orc, G), hint)
        assert st["path"] == "onchip", (G, hint, st)


def w_agg_slots(ex, orc, opts, v):
    opts(agg_slots=v)
    _onchip(ex, orc, opts)


def w_agg_blocks(ex, orc, opts, v):
    opts(agg_blocks=v)
    _onchip(ex, orc, opts)


GP_SHAPES = [(100_000, 1), (2_000_000, 2)]  # (groups, partition levels)


def _partitioned(ex, orc, opts, path="partitioned_direct", shapes=GP_SHAPES):
    for G, levels in shapes:
        opts(gb_partition=1, gb_levels=levels)
        st = gb_exact(ex, gb_data(ex, orc, G), G)
        assert (st["path"], st["levels"]) == (path, levels), (G, st)


def w_gb_seg_slots(ex, orc, opts, v):
    opts(gb_seg_slots=v)
    _partitioned(ex, orc, opts)


def w_gb_chunks(ex, orc, opts, v):
    opts(gb_chunks=v)
    _partitioned(ex, orc, opts)
    if v == 1:
        # 256 level-0 partitions on <= 256 CUs: one chunk per partition at ONE level, so the
        # partitions' groups are appended unhashed (the dense append, else reached only
        # behind two levels)
        assert ex.info()["num_cus"] <= 256
        opts(gb_l0_bits=8)
        _partitioned(ex, orc, opts, shapes=GP_SHAPES[:1])


def w_gb_direct(ex, orc, opts, v):
    opts(gb_direct=v)
    _partitioned(ex, orc, opts, path="partitioned_direct" if v else "partitioned_spill")


def ordered_data(ex, orc):
    def make():
        G = 2_000_000
        key = orc.gen_column(2, 0x61, gorder.N, a=G)
        val = orc.gen_column(3, 0x62, gorder.N)
        ok, ow = orc.groupby([key], AGGS4, values=[val])
        return gb_query(dev(key, ex), dev(val, ex)), G, ok, ow
    return cached("ordered", make)


def ordered_exact(ex, orc, path="partitioned_ordered"):
    """nut_groupby_to_host at N = 2^24 + 4099 rows, G = 2e6, dyadic values, pinned outputs."""
    q, G, ok, ow = ordered_data(ex, orc)
    k, w, got = gorder.run_to_host(ex, q, G)
    assert got == path
    assert len(k) == len(ok) > 0.99 * G
    gorder.check(k, w, ok, ow, sums_exact=True)


def w_gb_l0_bits(ex, orc, opts, v):
    opts(gb_l0_bits=v)
    # the hashed partitioned path; 6- and 8-bit level-0 digits with both ends of gb_l1_bits
    for b1 in ((6, 8) if v in (6, 8) else (DEFAULT["gb_l1_bits"],)):
        opts(gb_l1_bits=b1)
        _partitioned(ex, orc, opts, shapes=GP_SHAPES if b1 == 6 else GP_SHAPES[1:])
    # the ordered path splits its 14 cell bits v + (14 - v)
    opts(gb_partition=DEFAULT["gb_partition"], gb_levels=DEFAULT["gb_levels"], gb_l1_bits=DEFAULT["gb_l1_bits"])
    ordered_exact(ex, orc)


def w_gb_l1_spare(ex, orc, opts, v):
    opts(gb_l1_spare=v)
    for threads in (1024, 512):
        opts(gb_l1_threads=threads)
        ordered_exact(ex, orc)


def w_gb_l1_threads(ex, orc, opts, v):
    opts(gb_l1_threads=v)
    ordered_exact(ex, orc)


def w_gb_ordered(ex, orc, opts, v):
    opts(gb_ordered=v)
    ordered_exact(ex, orc, "partitioned_ordered" if v else "partitioned_direct:shape")


def w_gb_heavy(ex, orc, opts, v):
    """Zipf-like keys (test_ordered_skew_generator's): with the heavy-key pass and exact
    regions (1), with the pass and capped regions (2), without it (0)."""
    from nutdb_amd import _lib as L
    opts(gb_heavy=v)
    G, N = 4_000_000, gorder.N
    q, ok, ow = cached("skew", lambda: (gb_query(ex.gen_column(L.GEN_SKEW_KEY, 0x51, N, a=G),
                                                  ex.gen_column(L.GEN_DYADIC, 0x52, N)),
                                         *orc.groupby_pool_dyadic(G, N, key_seed=0x51, val_seed=0x52, kind=7)))
    k, w, path = gorder.run_to_host(ex, q, int(ok.shape[0]))
    assert path == "partitioned_ordered"
    hk, hr = ex.groupby_heavy()
    if v:
        assert hk > 100 and hr > N // 4
        assert (ex.groupby_overflow_rows() == 0) == (v == 1)
    else:
        assert (hk, hr) == (0, 0) and ex.groupby_overflow_rows() > 0
    assert np.array_equal(k, ok) and np.array_equal(w.view(np.uint64), ow)


def w_gb_partition(ex, orc, opts, v):
    opts(gb_partition=v)
    for G in (1000, 100_000):  # auto partitions from 2^16 hinted groups
        st = gb_exact(ex, gb_data(ex, orc, G), G)
        assert (st["path"] != "onchip") == (v == 1 or (v == -1 and G >= 1 << 16)), (G, st)


def w_gb_levels(ex, orc, opts, v):
    opts(gb_partition=1, gb_levels=v)
    for G in (100_000, 2_000_000):  # auto: two levels above 256 Ki hinted groups
        st = gb_exact(ex, gb_data(ex, orc, G), G)
        assert (st["path"], st["levels"]) == ("partitioned_direct", v or (2 if G > 256 * 1024 else 1)), st


def w_gb_optimistic(ex, orc, opts, v):
    opts(gb_partition=1, gb_levels=1, gb_optimistic=v)
    st = gb_exact(ex, gb_data(ex, orc, 100_000), 100_000)
    assert (st["path"], st["optimistic"]) == ("partitioned_direct", bool(v)), st


def distinct_data(ex, orc):
    def make():
        key = orc.gen_column(1, 0x63, GB_N)  # distinct keys
        val = orc.gen_column(3, 0x64, GB_N)
        ok, ow = orc.groupby([key], AGGS4, values=[val])
        return dev(key, ex), dev(val, ex), ok, ow
    return cached("distinct", make)


def w_gb_l1_bits(ex, orc, opts, v):
    """Two capped levels (offered from 6.5 M hinted groups), test_gp_capped_level1_fallback's
    uniform case."""
    opts(gb_partition=1, gb_levels=2, gb_optimistic=1, gb_l1_bits=v)
    st = gb_exact(ex, distinct_data(ex, orc), 10_000_000)
    assert (st["path"], st["levels"], st["capped_levels"]) == ("partitioned_direct", 2, 2), st


def w_gb_dense(ex, orc, opts, v):
    """One workgroup per partition behind two levels: appended unhashed (1) or merged through
    the hash table (0); a hint far too small reruns hashed."""
    opts(gb_partition=1, gb_levels=2, gb_dense=v)
    for hint in (GB_N, 10):
        st = gb_exact(ex, distinct_data(ex, orc), hint)
        assert hint == 10 or (st["path"], st["levels"]) == ("partitioned_direct", 2), st


# ----------------------------------------------------------------------------- join
def join_inputs():
    def make():
        rng = np.random.default_rng(15)
        unique = (rng.permutation(np.arange(70_000, dtype=np.int64) * 5),
                  rng.integers(-100, 400_000, 100_003).astype(np.int64))
        rng = np.random.default_rng(5)
        dups = (rng.integers(0, 300, 20_000).astype(np.int64), rng.integers(-50, 350, 30_001).astype(np.int64))
        return unique, dups
    return cached("join", make)


def _joins(ex, orc, opts, any_order):
    """Unique build keys: with join_match on, the ordered probe runs in two passes (the walk
    kernel of join_any_cfg, then the write-out).  Repeated build keys: INNER / LEFT stay one
    ordered pass (join_probe_cfg).  Both forms of the API (passes 1: one probe into arrays,
    again at the exact size if they were too small; 2: count, then write)."""
    for match in ((1, 0) if not any_order else (DEFAULT["join_match"],)):
        opts(join_match=match)
        for b, p in join_inputs():
            for how in tjoin.HOW:
                for passes in (1, 2):
                    tjoin.check(ex, orc, b, p, how, passes=passes, any_order=any_order)


def _join_count_then_write(ex, orc, opts, built, written):
    """nut_join_i64 under one join_probe_cfg, nut_join_write under another: a join keeps
    the tile shape it was built with (its status array is sized by it)."""
    from nutdb_amd._lib import check, lib
    b, p = join_inputs()[1]
    bd, pd = dev(b, ex), dev(p, ex)
    for how in ("inner", "anti"):
        opts(join_probe_cfg=built)
        ex._bind_stream()
        h, n = C.c_void_p(), C.c_uint64()
        check(lib.nut_join_i64(ex.ctx, C.c_void_p(bd.data_ptr()), len(b), C.c_void_p(pd.data_ptr()), len(p),
                               ex.JOIN_TYPES[how], C.byref(h), C.byref(n)), "nut_join_i64")
        try:
            opts(join_probe_cfg=written)
            pi = torch.empty(n.value, dtype=torch.int64, device=ex.device)
            bi = torch.empty(n.value, dtype=torch.int64, device=ex.device)
            check(lib.nut_join_write(h, C.c_void_p(pi.data_ptr()), C.c_void_p(bi.data_ptr())), "nut_join_write")
            ex.sync()
        finally:
            lib.nut_join_free(h)
        pi, bi = host(pi), host(bi)
        wp, wb = orc.join_i64(b, p, how)
        assert len(wp) > 0 and np.all(pi[1:] >= pi[:-1])
        gp, gb = tjoin.canon(pi, bi)
        assert np.array_equal(gp, wp) and np.array_equal(gb, wb), (how, built, written)
    opts(join_probe_cfg=built)


def w_join_probe_cfg(ex, orc, opts, v):
    opts(join_probe_cfg=v)
    _joins(ex, orc, opts, any_order=False)
    # the smallest tiles (cfg 4: 256 x 4) against the largest (cfg 3: 512 x 16)
    _join_count_then_write(ex, orc, opts, v, 3 if v != 3 else 4)


def w_join_any_cfg(ex, orc, opts, v):
    opts(join_any_cfg=v)
    _joins(ex, orc, opts, any_order=False)
    _joins(ex, orc, opts, any_order=True)


def w_join_match(ex, orc, opts, v):
    opts(join_match=v)
    for b, p in join_inputs():
        for how in tjoin.HOW:
            tjoin.check(ex, orc, b, p, how)


def _pair_words(pi, bi):
    """The pairs as one sorted int64 word each (probe row * 2^22 + build row + 1): equal
    arrays = equal pair multisets (a lexsort of these 4 M pairs takes seconds per join)."""
    assert len(bi) == 0 or (bi.min() >= -1 and bi.max() + 1 < 1 << 22 and pi.max() < 1 << 40)
    return np.sort(pi * (1 << 22) + (bi + 1))


def w_join_region(ex, orc, opts, v):
    """test_join_region_build's size (> 2^20 build rows, repeated keys): built region by
    region in LDS (1) or by global CAS (0), the same pairs — those of the C oracle, which
    tests/test_join_cpu.py holds to the numpy one."""
    def make():
        rng = np.random.default_rng(31)
        b = rng.integers(0, 1_500_000, 2_100_000).astype(np.int64)
        p = rng.integers(-100_000, 1_600_000, 3_000_001).astype(np.int64)
        return dev(b, ex), dev(p, ex), {how: _pair_words(*orc.join_i64_c(b, p, how)) for how in tjoin.HOW}
    bd, pd, want = cached("join_region", make)
    opts(join_region=v)
    for how in tjoin.HOW:
        pi, bi = ex.join_i64(bd, pd, how)
        pi, bi = host(pi), host(bi)
        assert np.all(pi[1:] >= pi[:-1]), "pairs not in probe-row order"
        assert np.array_equal(_pair_words(pi, bi), want[how]), how


# ----------------------------------------------------------------------------- scans, sort
def w_sel_blocks(ex, orc, opts, v):
    """300 select tiles of 16384 rows and a ragged one: with sel_blocks = 1 (a workgroup per
    CU) there are fewer workgroups than tiles, so the option changes how many tiles a
    workgroup takes in turn; at the default and at 16 every tile has its own."""
    def make():
        rng = np.random.default_rng(19)
        n = 300 * 16384 + 1_003
        a = rng.integers(-50, 50, n).astype(np.int64)
        b = rng.integers(0, 10, n).astype(np.int64)
        return dev(a, ex), dev(b, ex), np.flatnonzero((a > 3) & (b < 7)).astype(np.int64)
    a, b, want = cached("select", make)
    if v == 1:
        assert ex.info()["num_cus"] * v < 301, "sel_blocks = 1 would still give every tile its own workgroup"
    opts(sel_blocks=v)
    where = [("col", 0), ("i64", 0, 3), ("gt",), ("col", 1), ("i64", 0, 7), ("lt",), ("and",)]
    assert np.array_equal(host(ex.select_rows([a, b], where)), want)


def w_stream_blocks(ex, orc, opts, v):
    opts(stream_blocks=v)
    tprobe.test_probe_writes_ratio(ex, 64 * 37 + 13, 32)  # its contents check


def w_topk(ex, orc, opts, v):
    """ORDER BY ... LIMIT over >= 2^16 rows: the top-k candidates (1) or the full sort (0)."""
    def make():
        rng = np.random.default_rng(13)
        n = 200_003
        a = rng.integers(-10**6, 10**6, n).astype(np.int64)
        b = rng.integers(0, 50, n).astype(np.int64)  # heavy ties
        return a, b, {"a": dev(a, ex), "b": dev(b, ex)}
    a, b, cols = cached("topk", make)
    opts(topk=v)
    got = ex.sql("select a from t where a > 5 order by a desc limit 37 offset 11", cols)["a"]
    assert np.array_equal(got, np.sort(a[a > 5])[::-1][11:48])
    got = ex.sql("select b, a from t order by b limit 7000", cols)
    o = np.argsort(b, kind="stable")[:7000]
    assert np.array_equal(got["b"], b[o]) and np.array_equal(got["a"], a[o])


SORT_N = 1 << 25  # the capped two-level layout starts here


def sort_data(ex, orc, kind):
    def make():
        rng = np.random.default_rng(5)
        if kind == "uniform":      # full range: the identity digit map
            v = orc.gen_column(1, 0x57, SORT_N)
        elif kind == "range40":    # keys in [0, 2^40): the mapped-range digit
            v = rng.integers(0, 1 << 40, SORT_N, dtype=np.int64)
        else:                      # test_sort_capped_fallback's unsampled_skew
            v = rng.integers(I64_MIN, I64_MAX, SORT_N, dtype=np.int64)
            keep = np.zeros(SORT_N, dtype=bool)
            keep[(np.arange(16384, dtype=np.int64) * SORT_N) // 16384] = True
            v[~keep] = 77
        return dev(v, ex), np.sort(v)
    return cached(("sort", kind), make)


def w_sort_bd(ex, orc, opts, v):
    """The capped scatter levels at 1024 threads (0, 1024) or 512 (another kernel
    instantiation and tile table): 48 B/key, two levels, bit-exact both ways; a skew the
    admission sample does not see overflows a level-0 region at run time and the exact
    layout sorts again."""
    opts(sort_bd=v)
    for kind in ("uniform", "range40"):
        col, want = sort_data(ex, orc, kind)
        for desc in (False, True):
            got = host(ex.sort_i64(col, descending=desc))
            assert ex.sort_stats() == (48 * SORT_N, 2), (kind, desc)
            assert np.array_equal(got, want[::-1] if desc else want), (kind, desc)
    col, want = sort_data(ex, orc, "unsampled_skew")
    got = host(ex.sort_i64(col))
    assert ex.sort_stats()[0] != 48 * SORT_N
    assert np.array_equal(got, want)


# ----------------------------------------------------------------------------- the sweep
WORKLOADS = {
    "gb_partition": w_gb_partition, "gb_levels": w_gb_levels, "gb_optimistic": w_gb_optimistic,
    "gb_direct": w_gb_direct, "gb_chunks": w_gb_chunks, "join_region": w_join_region,
    "join_probe_cfg": w_join_probe_cfg, "join_any_cfg": w_join_any_cfg, "gb_seg_slots": w_gb_seg_slots,
    "gb_dense": w_gb_dense, "gb_l1_bits": w_gb_l1_bits, "topk": w_topk, "gb_l0_bits": w_gb_l0_bits,
    "stream_blocks": w_stream_blocks, "priv_bd": w_priv_bd, "priv_blocks": w_priv_blocks,
    "agg_blocks": w_agg_blocks, "sel_blocks": w_sel_blocks, "sort_bd": w_sort_bd, "gb_ordered": w_gb_ordered,
    "priv_probe": w_priv_probe, "gb_heavy": w_gb_heavy, "join_match": w_join_match,
    "gb_l1_threads": w_gb_l1_threads, "agg_slots": w_agg_slots, "gb_l1_spare": w_gb_l1_spare,
}


@pytest.mark.parametrize("name,value", CASES, ids=[f"{n}={v}" for n, v in CASES])
def test_option_value(ex, orc, opts, name, value):
    WORKLOADS[name](ex, orc, opts, value)
    assert _get(ex, name) == value  # the workload ran under it to the end


def _get(ex, name):
    from nutdb_amd._lib import check, lib
    v = C.c_int64()
    check(lib.nut_ctx_get_option(ex.ctx, ex.OPTIONS[name], C.byref(v)), "nut_ctx_get_option")
    return v.value


@pytest.mark.parametrize("name", list(SWEEP))
def test_option_rejects_values_outside_its_set(ex, name):
    """lo - 1, hi + 1 and the non-members of an enumerated set are refused, and the stored
    value stays what it was."""
    from nutdb_amd._lib import STATUS_NAMES, NutError
    lo, hi, default, _ = TABLE[name]
    before = _get(ex, name)
    assert before == default  # every earlier test restored it
    for bad in [lo - 1, hi + 1] + NOT_MEMBERS.get(name, []):
        with pytest.raises(NutError) as ei:
            ex.set_option(name, bad)
        assert STATUS_NAMES[ei.value.status] == "NUT_ERR_INVALID_ARG", (name, bad)
        assert _get(ex, name) == before, (name, bad)
