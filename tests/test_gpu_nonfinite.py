"""GPU: NaN, +-inf, subnormal, overflowing and zero f64 VALUES through every accumulator of
the group-by and through expression programs, against the C oracle (pinned on the CPU by
tests/test_oracle_nonfinite_cpu.py) and the numpy expression oracle.

The values come from helpers.nonfinite_values: each group has one class, and every finite
sum is exact in any summation order, so NOTHING here uses a tolerance (helpers.nf_check):
  * keys, COUNT, MIN and MAX words are bit-equal to the oracle's — NaN sign and payload
    included, since MIN / MAX select an input value in the total order
    -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN (payload bits significant);
  * SUM words are bit-equal, except where the oracle's sum is NaN: there only isnan(got)
    is asked (the sign and payload of an inf - inf NaN are the hardware's);
  * each test checks that its reference holds a NaN sum, both infinities, a non-zero
    subnormal sum and a zero sum (helpers.nf_covers_all), and that it ran the path it names
    as far as the library reports one (nut_ctx_groupby_stats / _heavy / _overflow: the
    partitioned and ordered paths, their levels, the heavy pass, the arenas).  The stats say
    only "onchip" for every on-chip kernel, so the private / shared / g_row kernels, the
    fused shapes, Q1 and the small to-host path are reached BY CONSTRUCTION — hint <= 8 and
    keys inside the direct map, 16-byte aligned columns (pick_kernel's vector gate), the
    aggregate lists of agg_ops.hpp's shapes, a table that fits the small path's staging
    (which otherwise falls back silently to the general path) — not by an assertion; finer
    stats would let these tests pin the kernel.
A subnormal that an atomic add flushed would show as 0, an identity-equality shortcut that
dropped a value equal to agg_init (MAX: -NaN 0xFFFF..., MIN: +NaN 0x7FFF...) as a wrong
MIN / MAX word."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from helpers import (NF_ALL, NF_BOTH_INF, NF_HUGE, NF_NAN, NF_NINF, NF_PINF, NF_PLAIN, NF_SUBNORMAL, NF_ZERO, OPCODE,
                     f64_from_ord, f64_ord, nf_check, nf_covers_all, nonfinite_divisors, nonfinite_values)
from oracle import oracle as _orc
from test_gpu_exec import AGGS4, gb_query

pytestmark = pytest.mark.gpu

CLASSES7 = (NF_PINF, NF_NINF, NF_BOTH_INF, NF_NAN, NF_SUBNORMAL, NF_HUGE, NF_ZERO)  # for G = 7
MAX_IDENTITY = 0xFFFFFFFFFFFFFFFF  # -NaN, ord 0: agg_init of an f64 MAX
MIN_IDENTITY = 0x7FFFFFFFFFFFFFFF  # +NaN, ord ~0: agg_init of an f64 MIN


@lru_cache(maxsize=None)
def table(G, n, classes=NF_ALL):
    """(key, val, finite int column, oracle keys, oracle words of AGGS4), made once and shared;
    keys are multiples of 7 around 0 (odd step: key mod 8 still takes every class) or, for
    G <= 8, the class indices themselves (inside the private kernels' direct map)."""
    rng = np.random.default_rng(G + n)
    key = rng.integers(0, G, n).astype(np.int64)
    if G > 8:
        key = key * 7 - 3 * G
    val = nonfinite_values(rng, key, classes)
    f = rng.integers(0, 100, n).astype(np.int64)
    ok, ow = _orc.groupby([key], AGGS4, values=[val])
    nf_covers_all(ow[:, 0])
    for a in (key, val, f, ok, ow):
        a.setflags(write=False)
    return key, val, f, ok, ow


def dev(x, ex):
    return torch.from_numpy(np.array(x)).to(ex.device)  # (a copy: the shared tables are read-only)


def run(ex, key, val, hint, preds=()):
    g = ex.groupby(gb_query(dev(key, ex), dev(val, ex), preds), group_hint=hint)
    out = g.to_host_words()
    g.free()
    return out


# ----------------------------------------------------------------------------- on-chip paths
@pytest.mark.parametrize("G,hint,n", [(8, 8, 200_003), (1000, 1000, 200_003), (100_000, 1000, 300_007)],
                         ids=["private_direct_map", "shared_lds", "global_fallback"])
def test_onchip_accumulators(ex, G, hint, n):
    """private per-thread accumulators (8 groups inside the direct map, hint 8), the shared
    LDS table (hint = G = 1000), and keys the block tables do not admit (G = 1e5 under a
    hint of 1000: g_row into the global table, which grows).  The library reports "onchip"
    for all three: which kernel ran follows from the hint and the keys, it is not asserted."""
    key, val, _, ok, ow = table(G, n)
    gk, gw = run(ex, key, val, hint)
    assert ex.groupby_stats()["path"] == "onchip"
    nf_check(gk, gw, ok, ow, what=G)


def test_small_to_host(ex):
    """nut_groupby_to_host at G = 7: the small-result path (one staged copy of the table).
    Reached by construction (one key, hint 7: the table fits the staging buffer); the stats
    cannot tell it from its fall-back, nut_groupby + nut_groups_to_host, which is "onchip" too."""
    key, val, _, ok, ow = table(7, 200_003, CLASSES7)
    gk, gw = ex.groupby_to_host(gb_query(dev(key, ex), dev(val, ex)), group_hint=7)
    assert ex.groupby_stats()["path"] == "onchip"
    nf_check(gk, gw, ok, ow)


@pytest.mark.parametrize("cls", [NF_PINF, NF_NAN, NF_SUBNORMAL])
def test_no_key_global_aggregate(ex, orc, cls):
    from nutdb_amd import Agg, AggQuery
    rng = np.random.default_rng(cls)
    n = 70_001
    zero = np.zeros(n, dtype=np.int64)
    val = nonfinite_values(rng, zero, (cls,))
    q = AggQuery(keys=[], values=[dev(val, ex)],
                 aggs=[Agg("sum", "col", (0,)), Agg("count"), Agg("min", "col", (0,)), Agg("max", "col", (0,))])
    g = ex.groupby(q)
    gk, gw = g.to_host_words()
    g.free()
    ok, ow = orc.groupby([zero], AGGS4, values=[val])
    s = ow[0, 0:1].view(np.float64)[0]
    assert {NF_PINF: s == np.inf, NF_NAN: np.isnan(s), NF_SUBNORMAL: s != 0 and abs(s) < 1e-300}[cls]
    nf_check(gk, gw, ok, ow, what=cls)


def test_fused_shapes_agree(ex, orc):
    """ShapeSum, ShapeSumCount, ShapeAll4 and a five-aggregate list (Generic), private
    (G = 8) and shared (G = 1000) kernels: each equals the oracle, so all four agree bit for
    bit outside NaN sums.  The shapes are selected by the aggregate lists (aggregate.hip
    shape_matches); no statistic names the one that ran."""
    from nutdb_amd import Agg, AggQuery
    a5 = [Agg("sum", "col", (0,)), Agg("count"), Agg("min", "col", (0,)), Agg("max", "col", (0,)),
          Agg("min", "col", (0,))]
    o5 = AGGS4 + [(2, 0, (0,))]
    for G in (8, 1000):
        key, val, _, _, _ = table(G, 200_003)
        k, v = dev(key, ex), dev(val, ex)
        sums = []
        for na in (1, 2, 4, 5):
            g = ex.groupby(AggQuery(keys=[k], values=[v], aggs=a5[:na]), group_hint=G)
            gk, gw = g.to_host_words()
            g.free()
            ok, ow = orc.groupby([key], o5[:na], values=[val])
            nf_check(gk, gw, ok, ow, what=(G, na))
            sums.append(gw[:, 0].copy())
        nan = np.isnan(sums[0].view(np.float64))
        for s in sums[1:]:
            assert np.array_equal(np.isnan(s.view(np.float64)), nan) and np.array_equal(s[~nan], sums[0][~nan])


def test_q1_fused_shape(ex, orc):
    """nut_q1 (ShapeQ1, two keys): SUM(qty), SUM(price), SUM(price * (1 - disc)), COUNT.
    disc is one of 0, 1/4, 1/2 and — where linestatus is 0 — 1, so price * (1 - disc) meets
    inf * 0 (NaN) there and inf * finite elsewhere; the factors are non-negative dyadics, so
    products keep their class.  A subnormal times 3/4 or 1/2 rounds: the test relies on the
    device's f64 multiply being correctly rounded on subnormals, as the host's is — each
    product is then the same on both sides, and sums of multiples of 2^-1074 stay exact."""
    rng = np.random.default_rng(41)
    n = 200_003
    rf = rng.integers(0, 4, n).astype(np.int64)
    ls = rng.integers(0, 2, n).astype(np.int64)
    gk = rf * 2 + ls
    price = nonfinite_values(rng, gk, (NF_PINF, NF_PINF, NF_NINF, NF_NINF, NF_SUBNORMAL, NF_HUGE, NF_PLAIN, NF_NAN))
    qty = nonfinite_values(rng, gk, (NF_ZERO, NF_BOTH_INF, NF_HUGE, NF_SUBNORMAL, NF_NAN, NF_PLAIN, NF_NINF, NF_PINF))
    disc = np.where(ls == 0, np.array([0.0, 0.25, 0.5, 1.0])[rng.integers(0, 4, n)],
                    np.array([0.0, 0.25, 0.5])[rng.integers(0, 3, n)])
    sd = rng.integers(0, 100, n).astype(np.int64)
    g = ex.q1(*[dev(c, ex) for c in (sd, rf, ls, qty, price, disc)], date_k=69)
    got = g.to_host_words()
    g.free()
    ok, ow = orc.groupby([rf, ls], [(0, 0, (0,)), (0, 0, (1,)), (0, 4, (1, 2)), (1, 0, ())],
                         values=[qty, price, disc], preds=[(sd, OPCODE["<="], 69)])
    dp = ow[:, 2].view(np.float64)
    assert len(ok) == 8 and np.isnan(dp[0]) and dp[1] == np.inf and np.isnan(dp[2]) and dp[3] == -np.inf
    assert dp[4] != 0 and abs(dp[4]) < 1e-300 and dp[5] == np.inf
    nf_covers_all(ow[:, 0])
    nf_check(got[0], got[1], ok, ow, sum_cols=(0, 1, 2))


# ----------------------------------------------------------------------------- partitioned paths
@pytest.mark.parametrize("levels", [1, 2])
def test_partitioned_direct_and_spill(ex, orc, opts, levels):
    """gb_partition = 1 at G = 1e5: without a predicate the rows are partitioned directly,
    with one (on a second, finite column: the classes stay pure) they are staged first."""
    opts(gb_partition=1, gb_levels=levels)
    key, val, f, ok, ow = table(100_000, 300_007)
    gk, gw = run(ex, key, val, 100_000)
    st = ex.groupby_stats()
    assert (st["path"], st["levels"]) == ("partitioned_direct", levels)
    nf_check(gk, gw, ok, ow, what="direct")
    gk, gw = run(ex, key, val, 100_000, [(dev(f, ex), ">=", 30)])
    st = ex.groupby_stats()
    assert (st["path"], st["levels"]) == ("partitioned_spill", levels)
    pk, pw = orc.groupby([key], AGGS4, values=[val], preds=[(f, OPCODE[">="], 30)])
    nf_covers_all(pw[:, 0])
    nf_check(gk, gw, pk, pw, what="spill")


def test_masked_aggregates_through_the_spill(ex, opts):
    """Expression mode through the spill: a masked-out row stages its aggregate's identity
    (agg_kernel.hpp), so a group whose ONLY unmasked value is the bit pattern of that
    identity (MAX: -NaN 0xFFFF..., MIN: +NaN 0x7FFF...) must still report it, not a masked
    row's value and not "no row"."""
    from test_gpu_expr import run_both
    opts(gb_partition=1)
    key, val, f, _, _ = (a.copy() for a in table(100_000, 300_007))
    ka, kb = 7 * 100_000 + 1, 7 * 100_000 + 2  # two keys of their own
    for k, bits in ((ka, MAX_IDENTITY), (kb, MIN_IDENTITY)):
        rows = np.arange(5) * 1009 + (k - ka) + 17
        key[rows] = k
        val[rows] = [3.5, -2.25, 0.0, 100.0, -7.0]
        f[rows] = 90                       # masked out ...
        val[rows[2]] = np.array([bits], dtype=np.uint64).view(np.float64)[0]
        f[rows[2]] = 10                    # ... but for the identity pattern
    mask = [("col", 1), ("i64", 0, 50), ("lt",)]
    x = [("col", 0)]
    aggs = [("max", x, mask), ("sum", x, mask), ("count", None, mask), ("min", x, mask), ("count", None, None)]
    gk, gw, ok, ow, _ = run_both(ex, [key], [val, f], None, aggs, 100_000)
    assert ex.groupby_stats()["path"] == "partitioned_spill"
    ia, ib = int(np.searchsorted(ok[:, 0], ka)), int(np.searchsorted(ok[:, 0], kb))
    assert (ow[ia, 0], ow[ia, 2], ow[ia, 4]) == (MAX_IDENTITY, 1, 5) and ow[ia, 3] == MAX_IDENTITY
    assert (ow[ib, 3], ow[ib, 2], ow[ib, 4]) == (MIN_IDENTITY, 1, 5) and ow[ib, 0] == MIN_IDENTITY
    nf_covers_all(ow[:, 1])
    nf_check(gk, gw, ok, ow, sum_cols=(1,))


N_ORDERED = (1 << 24) + 4099  # the ordered path starts at 2^24 rows


@pytest.mark.parametrize("heavy_cls", [NF_PINF, NF_NAN], ids=["heavy_pinf", "heavy_nan"])
def test_ordered_heavy_and_overflow(ex, orc, opts, heavy_cls):
    """nut_groupby_to_host on the ordered path (its smallest size): one key on 10 % of the
    rows goes through the heavy-key pass (heavy.hpp) — its class +inf, then NaN with the two
    identity patterns among its values.  gb_heavy = 2 keeps the levels capped behind that
    pass, and 128 adjacent keys (one range cell, every class) of 60 rows each — too few rows
    per key for the sample to call one heavy, 3x a level-1 region together — overflow into
    the arenas.  (A single key on 0.3 % of the rows joins the heavy set once there is one,
    so it cannot show the arenas in the same run.)"""
    opts(gb_heavy=2)
    G = 2_000_000
    key = orc.gen_column(2, 0x6A, N_ORDERED, a=G)
    rng = np.random.default_rng(11)
    head = key[:4096]
    hk = int(head[head % 8 == heavy_cls][0])
    c0 = int(head[head != hk][0])
    key[rng.random(N_ORDERED) < 0.1] = hk
    rows = np.flatnonzero(key != hk)
    rows = rows[rng.choice(len(rows), 128 * 60, replace=False)]
    key[rows] = c0 + 1 + np.arange(len(rows)) % 128
    val = nonfinite_values(rng, key)
    out = tuple(torch.empty((2 * G, c), dtype=torch.int64, pin_memory=True).numpy() for c in (1, 4))
    gk, gw = ex.groupby_to_host(gb_query(dev(key, ex), dev(val, ex)), group_hint=G, out=out)
    assert ex.groupby_stats()["path"] == "partitioned_ordered", ex.groupby_declined()
    nheavy, hrows = ex.groupby_heavy()
    assert nheavy >= 1 and hrows >= int((key == hk).sum())
    assert ex.groupby_overflow_rows() > 0
    ok, ow = orc.groupby([key], AGGS4, values=[val])
    nf_covers_all(ow[:, 0])
    s = ow[np.searchsorted(ok[:, 0], hk), 0:1].view(np.float64)[0]
    assert s == np.inf if heavy_cls == NF_PINF else np.isnan(s)
    nf_covers_all(ow[np.searchsorted(ok[:, 0], c0 + 1):, 0][:128])
    nf_check(gk, gw.view(np.uint64), ok, ow)


# ----------------------------------------------------------------------------- partials and merges
def test_accumulate_and_partition(ex, orc):
    """nut_groupby_accumulate + nut_groups_partition: two halves of the rows into one table,
    split so that a both-infinities group gets every +inf from the first half and every
    -inf from the second (the NaN appears only in the merge); then the owner partition's
    parts, each merged as partials (sum / sum / min / max) like a receiving rank does."""
    from nutdb_amd import Agg, AggQuery
    key, val, _, ok, ow = table(1000, 200_003)
    rng = np.random.default_rng(5)
    both = key % 8 == NF_BOTH_INF
    second = np.where(both & np.isinf(val), val < 0, rng.random(len(key)) < 0.5)
    assert not np.any(val[both & ~second] == -np.inf) and not np.any(val[both & second] == np.inf)
    a, b = ~second, second
    g = ex.groupby(gb_query(dev(key[a], ex), dev(val[a], ex)), group_hint=1000)
    ha = g.to_host_words()[1][:, 0].view(np.float64)
    assert not np.isnan(ha[ok[:, 0] % 8 == NF_BOTH_INF]).any()  # (every group has rows in both halves)
    ones = np.ones(int(b.sum()), dtype=np.int64)  # COUNT partials merge as sums
    ex.accumulate(AggQuery(keys=[dev(key[b], ex)], values=[dev(val[b], ex), dev(ones, ex)],
                           aggs=[Agg("sum", "col", (0,)), Agg("sum", "col", (1,)), Agg("min", "col", (0,)),
                                 Agg("max", "col", (0,))]), g)
    gk, gw = g.to_host_words()
    nf_check(gk, gw, ok, ow, what="accumulate")
    P, w = 3, 5
    buf, counts = g.partition(P)
    g.free()
    assert sum(counts) == len(ok) and min(counts) > 0
    parts, off = [], 0
    for p in range(P):
        seg = buf[w * off: w * (off + counts[p])].view(w, counts[p])
        off += counts[p]
        q = AggQuery(keys=[seg[0].contiguous()],
                     values=[seg[1].contiguous().view(torch.float64), seg[2].contiguous(),
                             seg[3].contiguous().view(torch.float64), seg[4].contiguous().view(torch.float64)],
                     aggs=[Agg("sum", "col", (0,)), Agg("sum", "col", (1,)), Agg("min", "col", (2,)),
                           Agg("max", "col", (3,))])
        o = ex.groupby(q, group_hint=1000)
        parts.append(o.to_host_words())
        o.free()
    keys = np.concatenate([p[0] for p in parts])
    words = np.concatenate([p[1] for p in parts])
    order = np.argsort(keys[:, 0], kind="stable")
    nf_check(keys[order], words[order], ok, ow, what="partition")


PADDED_GATHER_WORDS = 1 << 20  # dist.cpp kPaddedGather: at most this many gathered words take the padded gather


@pytest.mark.parametrize("G,rows", [(7, 100_003), (200_000, 200_003)], ids=["padded_gather", "header_gather"])
def test_virtual_ranks_owner_merge(orc, G, rows):
    """nut_dist over 3 virtual ranks: classes go by key, so every rank holds partial groups
    that meet in the owner merge.  Rank 0 gathers the owners' groups padded while the words
    owners 1.. receive — 1 + W x (partial groups received) each, W = keys + aggregates = 5 —
    stay within 2^20, else by their headers.  The library reports neither, so the test works
    the count out itself (nutdb_amd.dist.owner_of is the device's owner hash): G = 7 is far
    below the threshold, and G = 2e5 needs 200 003 rows per rank (~126 k distinct keys each,
    ~1.26 M words; 100 003 rows per rank cannot pass 2^20 with five words per group)."""
    from nutdb_amd import Agg, AggQuery
    from nutdb_amd.dist import NutDist, owner_of
    P, W = 3, 5
    n = P * rows
    key, val, _, ok, ow = table(G, n, CLASSES7 if G == 7 else NF_ALL)
    cuts = [(n * r // P, n * (r + 1) // P) for r in range(P)]
    received = np.zeros(P, dtype=np.int64)  # partial groups each owner receives
    for a, b in cuts:
        received += np.bincount(owner_of(np.unique(key[a:b]), None, P), minlength=P)
    gather_words = int(np.sum(1 + W * received[1:]))
    assert gather_words < PADDED_GATHER_WORDS // 100 if G == 7 else gather_words > 1.15 * PADDED_GATHER_WORDS
    aggs = [Agg("sum", "col", (0,)), Agg("count"), Agg("min", "col", (0,)), Agg("max", "col", (0,))]
    to = lambda x: torch.from_numpy(np.array(x)).to("cuda:0")  # noqa: E731
    qs = [AggQuery(keys=[to(key[a:b])], values=[to(val[a:b])], aggs=aggs, rows=b - a) for a, b in cuts]
    d = NutDist.virtual(P)
    try:
        out = d.groupby(qs, group_hint=G)
        assert out[0] is not None and all(o is None for o in out[1:])
        gk, gw = out[0].to_host_words()
        out[0].free()
    finally:
        d.close()
    nf_check(gk, gw, ok, ow, what=G)


# ----------------------------------------------------------------------------- expression mode
def prog_table(nk, n=200_003):
    """16 (x 3) groups: keys 0..7 keep their class under the divisors, keys 8..15 also divide
    by 0.0 and -0.0 (helpers.nonfinite_divisors); plus a NaN-bearing comparison column.
    Without a key every row is in ONE group, so the classes that must stay pure (only
    subnormals, only same-signed huge values) are left out there: what remains — dyadic
    values, infinities, NaNs, zeros — sums to the same word in any order."""
    rng = np.random.default_rng(300 + nk)
    k1 = rng.integers(0, 16, n).astype(np.int64)
    f0 = nonfinite_values(rng, k1, NF_ALL if nk else (NF_PLAIN, NF_PINF, NF_NINF, NF_BOTH_INF, NF_NAN, NF_ZERO))
    f1 = nonfinite_divisors(rng, k1)
    y = rng.integers(-64, 64, n).astype(np.float64) / 4.0
    sp = rng.random(n)
    y[sp < 0.05] = np.nan
    y[(sp >= 0.05) & (sp < 0.07)] = np.inf
    y[(sp >= 0.07) & (sp < 0.09)] = -np.inf
    y[(sp >= 0.09) & (sp < 0.11)] = -np.nan
    i0 = rng.integers(-50, 51, n).astype(np.int64)
    keys = [k1, rng.integers(0, 3, n).astype(np.int64)][:nk]
    return keys, [f0, f1, y, i0]


def check_prog(ex, keys, cols, where, aggs, hint, sum_cols):
    from test_gpu_expr import run_both
    gk, gw, ok, ow, types = run_both(ex, keys, cols, where, aggs, hint)
    assert gk.shape == ok.shape
    nf_check(gk if keys else ok, gw, ok, ow, sum_cols=sum_cols, what=(len(keys), hint))
    return ok, ow


@pytest.mark.parametrize("nk,hint", [(0, 0), (1, 4), (2, 64)])
def test_prog_f64_division_by_zero(ex, nk, hint):
    """sum(f0 / f1), min(f0 / f1), max(fmod(f0, f1)) where f1 holds 0.0 and -0.0 and f0 holds
    0.0: x / 0 is +-inf, 0 / 0 and fmod(x, 0) are NaN, as oracle/expr.py defines with numpy —
    no error (only an INTEGER division by zero raises)."""
    keys, cols = prog_table(nk)
    div = [("col", 0), ("col", 1), ("div",)]
    mod = [("col", 0), ("col", 1), ("mod",)]
    aggs = [("sum", div, None), ("min", div, None), ("max", mod, None), ("count", None, None), ("max", div, None)]
    ok, ow = check_prog(ex, keys, cols, None, aggs, hint, (0,))
    if nk:
        s = ow[:, 0].view(np.float64)[ok[:, 0] < 8]
        assert np.isnan(s).any() and (s == np.inf).any() and (s == -np.inf).any() and (s == 0).any()
        assert ((s != 0) & (np.abs(s) < 1e-300)).any()
        assert np.isnan(ow[:, 0].view(np.float64)[ok[:, 0] >= 8]).all()


@pytest.mark.parametrize("op,nk,hint", [("lt", 1, 4), ("le", 2, 64), ("gt", 0, 0), ("ge", 1, 64), ("eq", 2, 4),
                                        ("ne", 0, 0), ("ne", 1, 4)])
def test_prog_comparisons_with_nan(ex, op, nk, hint):
    """WHERE and an aggregate's mask compare a NaN-bearing column (both NaN signs, both
    infinities) with a column and with a constant: a NaN operand fails every comparison but
    !=.  The aggregated column keeps its classes (any subset of a class is of that class),
    and non-finite sums survive every WHERE here; 0, 1 and 2 keys, private and shared tables."""
    keys, cols = prog_table(nk)
    where = [("col", 2), ("col", 0), (op,)]
    mask = [("col", 2), ("f64", 0, 0.25), (op,)]
    x = [("col", 0)]
    aggs = [("count", None, None), ("sum", x, None), ("min", x, None), ("count", None, mask), ("sum", x, mask),
            ("max", x, mask)]
    ok, ow = check_prog(ex, keys, cols, where, aggs, hint, (1, 4))
    assert not np.isfinite(ow[:, 1].view(np.float64)).all() and ow[:, 0].sum() > 0
    f0, y = cols[0], cols[2]
    with np.errstate(all="ignore"):
        fn = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal,
              "ne": np.not_equal}[op]
        w = fn(y, f0)
        m = w & fn(y, 0.25)
    nan = np.isnan(y) | np.isnan(f0)
    assert nan.any() and np.array_equal(w[nan], np.full(int(nan.sum()), op == "ne"))
    assert ow[:, 0].sum() == w.sum() and ow[:, 3].sum() == m.sum()


def test_prog_if_with_nan_branch(ex):
    """IF selects, it does not blend: the branch not taken may be NaN (a constant or a
    column) without reaching the aggregate."""
    keys, cols = prog_table(1)
    nan = float("nan")
    pos = [("col", 3), ("i64", 0, 0), ("ge",)]
    x = [("col", 0)]
    aggs = [("sum", pos + x + [("f64", 0, nan), ("if",)], pos),            # the NaN branch is never taken
            ("min", pos + x + [("f64", 0, nan), ("if",)], None),           # taken: +NaN is the largest
            ("max", pos + [("col", 2)] + x + [("if",)], None),             # NaNs of a column
            ("sum", pos + [("f64", 0, nan)] + x + [("if",)], [("col", 3), ("i64", 0, 0), ("lt",)]),
            ("count", None, pos)]
    ok, ow = check_prog(ex, keys, cols, None, aggs, 0, (0, 3))
    nf_covers_all(ow[ok[:, 0] < 8, 0])
    nf_covers_all(ow[ok[:, 0] < 8, 3])


# ----------------------------------------------------------------------------- SQL
def test_sql_nonfinite_aggregates(ex):
    """SQL over 8 groups, one per class.  Rules pinned here (semantics):
      * sum / min / max are the kernels' (above); avg = sum / count in f64, so an infinite
        sum gives an infinite avg and a NaN sum a NaN avg;
      * ORDER BY an f64 aggregate sorts by the IEEE total order: a NaN sorts first or last by
        ITS SIGN (-NaN before -inf, +NaN after +inf) — for a NaN that an inf - inf sum made,
        the sign is the hardware's, so such a row is at one end or the other;
      * HAVING compares as IEEE doubles: a NaN sum fails `> 0`, +inf passes."""
    key, val, _, _, _ = table(8, 100_003)
    cols = {"k": dev(key, ex), "v": dev(val, ex)}
    body = "select k, sum(v) as s, avg(v) as a, min(v) as mn, max(v) as mx, count(*) as c from t group by k"
    cnt = np.bincount(key, minlength=8)
    ov = f64_ord(val)
    mn = f64_from_ord(np.array([ov[key == g].min() for g in range(8)], dtype=np.uint64))
    mx = f64_from_ord(np.array([ov[key == g].max() for g in range(8)], dtype=np.uint64))
    with np.errstate(all="ignore"):  # exact where finite (any order), else +-inf / NaN by class
        sums = np.array([np.sum(val[key == g]) for g in range(8)])
    assert np.isnan(sums[[NF_BOTH_INF, NF_NAN]]).all() and sums[NF_PINF] == sums[NF_HUGE] == np.inf
    assert sums[NF_NINF] == -np.inf and 0 < abs(sums[NF_SUBNORMAL]) < 1e-300 and sums[NF_ZERO] == 0

    def check_rows(got, keep):
        ks = got["k"]
        assert sorted(ks.tolist()) == [g for g in range(8) if keep[g]]
        s, a = got["s"], got["a"]
        for i, g in enumerate(ks):
            if np.isnan(sums[g]):
                assert np.isnan(s[i]) and np.isnan(a[i]), g
            else:
                assert s[i:i + 1].view(np.uint64)[0] == sums[g:g + 1].view(np.uint64)[0], (g, s[i], sums[g])
                with np.errstate(all="ignore"):
                    assert a[i:i + 1].view(np.uint64)[0] == (sums[g:g + 1] / cnt[g]).view(np.uint64)[0], g
            assert got["mn"][i:i + 1].view(np.uint64)[0] == mn[g:g + 1].view(np.uint64)[0], g
            assert got["mx"][i:i + 1].view(np.uint64)[0] == mx[g:g + 1].view(np.uint64)[0], g
            assert got["c"][i] == cnt[g]

    every = np.ones(8, dtype=bool)
    got = ex.sql(body + " order by s, k", cols, group_hint=8)
    check_rows(got, every)
    so = f64_ord(got["s"])
    assert np.all(so[1:] >= so[:-1])                        # the total order of what came out
    numbers = [g for g in range(8) if not np.isnan(sums[g])]   # (NaN rows: at the ends, by sign)
    assert got["k"][~np.isnan(got["s"])].tolist() == sorted(numbers, key=lambda g: (int(f64_ord(sums[g:g + 1])[0]), g))
    assert got["a"][got["k"] == NF_PINF][0] == np.inf and np.isnan(got["a"][got["k"] == NF_BOTH_INF][0])
    got = ex.sql(body + " order by mx desc, k", cols, group_hint=8)
    check_rows(got, every)
    order = sorted(range(8), key=lambda g: (-int(f64_ord(mx[g:g + 1])[0]), g))
    assert got["k"].tolist() == order
    got = ex.sql(body + " having s > 0 order by k", cols, group_hint=8)
    with np.errstate(all="ignore"):
        keep = sums > 0
    assert keep[NF_PINF] and keep[NF_HUGE] and not keep[NF_NAN] and not keep[NF_BOTH_INF]
    check_rows(got, keep)
    assert got["k"].tolist() == [g for g in range(8) if keep[g]]
