"""GPU: the distributed operators of csrc/dist.cpp (nut_dist_groupby, nut_dist_sort_i64,
nut_dist_filter_i64, nut_dist_join_i64) at 9 to 64 ranks — the rank counts the C ABI accepts
(P <= 64) and tests/test_gpu_dist_native.py (P <= 8) never reaches.

Everything runs in virtual mode (nut_dist_create_virtual: P ranks on device 0, exchanges as
device copies, the same partition / exchange / merge code as the RCCL ranks), in one process.
Every comparison is exact: expected values come from the C oracle and numpy on the
concatenated shards; sums are over the oracle's dyadic column or int64 values, so they are
bit-exact in any order.  The sample sort's per-rank output sizes are also pinned to the
Python restatement of the skew-safe ranges (nutdb_amd/dist.py sort_ranges / split_counts,
itself pinned by tests/test_sort_ranges_cpu.py): at P >= 33 the C++ takes a branch (only the
repeated splitter values get a bucket of their own) that no smaller rank count reaches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

I64_MAX = np.iinfo(np.int64).max
I64_MIN = np.iinfo(np.int64).min
SAMPLES = 4096  # csrc/dist.cpp kSamples: strided samples per rank


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def shards(n, P):
    return [(n * r // P, n * (r + 1) // P) for r in range(P)]


def cuts_of(sizes):
    at = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return [(int(a), int(b)) for a, b in zip(at, at[1:])]


@pytest.fixture(scope="module")
def ND():
    from nutdb_amd.dist import NutDist
    return NutDist


# ---------------------------------------------------------------------------------- sort
def predict_sort(parts, P):
    """What nut_dist_sort_i64 must do with these shards, from the Python restatement: each
    non-empty shard's strided sample (positions i * n_r // 4096), pooled and sorted; splitters
    at pool[i * m // P]; sort_ranges; per-shard bucket counts (bucket = #{e <= key}) split
    over the buckets' ranks by split_counts and summed over the shards.  Returns the per-rank
    output sizes and the partition splitters e."""
    from nutdb_amd.dist import sort_ranges, split_counts
    idx = np.arange(SAMPLES, dtype=np.int64)
    samples = [s[(idx * len(s)) // SAMPLES] for s in parts if len(s)]
    pool = np.sort(np.concatenate(samples)) if samples else np.zeros(0, np.int64)
    m = len(pool)
    spl = [int(pool[(i * m) // P]) if m else 0 for i in range(1, P)]
    e, lo, hi, w = sort_ranges(spl, pool, P)
    sizes = [0] * P
    for s in parts:
        bc = np.bincount(np.searchsorted(e, s, "right"), minlength=len(e) + 1).tolist()
        for r, c in enumerate(split_counts(bc, lo, w, P)):
            sizes[r] += c
    return sizes, e


def run_sort(ND, P, parts):
    d = ND.virtual(P)
    try:
        outs = d.sort_i64([dev(s) for s in parts])
        return [o.cpu().numpy() for o in outs]
    finally:
        d.close()


def check_sort(got, parts, P):
    k = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    assert len(got) == P
    assert np.array_equal(np.concatenate(got), np.sort(k))                 # (a)
    live = [g for g in got if len(g)]
    for a, b in zip(live, live[1:]):                                       # (b)
        assert a[-1] <= b[0]
    want_sizes, e = predict_sort(parts, P)
    sizes = [len(g) for g in got]
    assert sizes == want_sizes, (sizes, want_sizes)                        # (c)
    return sizes, e


def sort_keys(orc, kind, n, P):
    k = orc.gen_column(1, 0x5000 + P, n)  # uniform over the full int64 range
    u = np.random.default_rng(P).random(n)
    if kind == "uniform":
        pass
    elif kind == "range200":
        k = orc.gen_column(5, 0x5100 + P, n, a=0, b=200)
    elif kind == "adjacent":
        k[u < 0.3] = 100
        k[(u >= 0.3) & (u < 0.6)] = 101
    elif kind == "one_key":
        k[:] = 12345
    else:
        k[u < 0.5] = {"heavy": -77, "heavy_max": I64_MAX, "heavy_min": I64_MIN}[kind]
    return k


SORT_KINDS = ["uniform", "range200", "heavy", "heavy_max", "heavy_min", "adjacent", "one_key"]
HEAVY_KINDS = ("heavy", "heavy_max", "heavy_min", "adjacent", "one_key")


@pytest.mark.parametrize("kind", SORT_KINDS)
@pytest.mark.parametrize("P", [9, 32, 33, 63, 64])
def test_sort(ND, orc, P, kind):
    """(a) the ranks' outputs concatenate to the sorted input, (b) neighbouring ranks are
    ordered, (c) the per-rank sizes are exactly the restatement's, (d) heavy keys are spread:
    no rank above 1.15 n / P (the restatement itself stays below 1.03 for these kinds; not
    asserted for range200, where with P >= 33 only repeated values get their own bucket and a
    single-quantile value's whole run moves to the next rank, by design).

    Which branch of sort_ranges runs: the P - 1 splitters of full-range uniform keys are
    distinct and not adjacent, so giving each a bucket {v} of its own needs 2 (P - 1) partition
    splitters: 62 at P = 32, within the 63 the range partition accepts, and 64 at P = 33.
    From P = 33 on the uniform case therefore takes the other branch (only repeated splitter
    values get a bucket) and is left with the P - 1 splitters themselves: 32 at P = 33, 63 at
    P = 64, the partition's upper bound."""
    n = 6000 * P + 7
    k = sort_keys(orc, kind, n, P)
    parts = [k[a:b] for a, b in shards(n, P)]
    sizes, e = check_sort(run_sort(ND, P, parts), parts, P)
    assert len(e) <= 63
    if kind == "uniform":  # the inputs still reach the branch they are here for
        assert len(e) == (2 * (P - 1) if P <= 32 else P - 1), len(e)
    if kind in HEAVY_KINDS:
        assert max(sizes) <= 1.15 * n / P, sizes                           # (d)
    if kind == "heavy_max":
        assert int(e[-1]) == I64_MAX  # {INT64_MAX} is the open last bucket: no splitter v + 1
    if kind == "heavy_min":
        assert int(e[0]) == I64_MIN and int(e[1]) == I64_MIN + 1
    if kind == "adjacent":
        assert 100 in e and 101 in e and 102 in e


@pytest.mark.parametrize("P", [9, 64])
def test_sort_tiny_and_empty_shards(ND, orc, P):
    """Every third rank empty, the others holding 1 to 3 keys (samples with repetition, far
    fewer keys than the 4096 sample positions), and the last rank holding the rest."""
    n = 6000 * P + 7
    k = orc.gen_column(1, 0x5200 + P, n)
    sizes = [0 if r % 3 == 1 else 1 + (r // 3) % 3 for r in range(P - 1)]
    sizes.append(n - sum(sizes))
    assert sizes.count(0) >= P // 3 and set(sizes[:-1]) == {0, 1, 2, 3} and sizes[-1] > SAMPLES
    parts = [k[a:b] for a, b in cuts_of(sizes)]
    check_sort(run_sort(ND, P, parts), parts, P)


@pytest.mark.parametrize("P", [9, 64])
def test_sort_small_shards_only(ND, orc, P):
    """No shard reaches the sample size: every sample repeats its shard's keys."""
    sizes = [(37 * r + 5) % 900 for r in range(P)]
    k = orc.gen_column(5, 0x5300 + P, sum(sizes), a=-50, b=100_000)
    parts = [k[a:b] for a, b in cuts_of(sizes)]
    assert max(sizes) < SAMPLES
    check_sort(run_sort(ND, P, parts), parts, P)


@pytest.mark.parametrize("P", [9, 64])
def test_sort_all_shards_empty(ND, P):
    got = run_sort(ND, P, [np.zeros(0, np.int64)] * P)
    assert [len(g) for g in got] == [0] * P


@pytest.mark.parametrize("P", [9, 64])
def test_sort_one_rank_holds_all(ND, orc, P):
    n = 6000 * P + 7
    k = orc.gen_column(1, 0x5400 + P, n)
    parts = [k if r == P // 2 else np.zeros(0, np.int64) for r in range(P)]
    check_sort(run_sort(ND, P, parts), parts, P)


# ------------------------------------------------------------------------------ group-by
AGGS6 = [("sum", (0,)), ("count", ()), ("min", (0,)), ("max", (0,)), ("sum", (1,)), ("min", (1,))]
AGGS8 = [("sum", (0,)), ("count", ()), ("min", (0,)), ("max", (0,)), ("sum", (1,)), ("count", ()),
         ("max", (1,)), ("min", (0,))]
ORC_OP = {"sum": 0, "count": 1, "min": 2, "max": 3}


def run_groupby(ND, P, cuts, keys, vals, aggs, hint, pred=None):
    """nut_dist_groupby over the shards `cuts` of the columns -> rank 0's (keys, words)."""
    from nutdb_amd import Agg, AggQuery
    qs = []
    for a, b in cuts:
        qs.append(AggQuery(keys=[dev(c[a:b]) for c in keys], values=[dev(c[a:b]) for c in vals],
                           aggs=[Agg(op, "col", args) for op, args in aggs], rows=b - a,
                           preds=[(dev(pred[0][a:b]), pred[1], pred[2])] if pred else []))
    d = ND.virtual(P)
    try:
        out = d.groupby(qs, group_hint=hint)
        assert out[0] is not None and all(o is None for o in out[1:])
        got = out[0].to_host_words()
        out[0].free()
        return got
    finally:
        d.close()


def want_groupby(orc, keys, vals, aggs, cap, pred=None):
    return orc.groupby(keys, [(ORC_OP[op], 0, args) for op, args in aggs], values=vals,
                       preds=[(pred[0], {"<": 0, "<=": 1}[pred[1]], pred[2])] if pred else [], cap=cap)


def cmp_groups(got, want):
    gk, gw = got
    wk, ww = want
    assert gk.shape == wk.shape and np.array_equal(gk, wk), (gk.shape, wk.shape)
    assert gw.shape == ww.shape
    for j in range(ww.shape[1]):
        assert np.array_equal(gw[:, j], ww[:, j]), j


def groupby_cols(orc, n, G, seed=0):
    key = orc.gen_column(2, 0x51 + seed, n, a=G)
    vd = orc.gen_column(3, 0x52 + seed, n)               # dyadic: exact sums in any order
    vi = orc.gen_column(5, 0x53 + seed, n, a=-1000, b=2001)
    return key, vd, vi


@pytest.mark.parametrize("P,G", [(9, 1000), (33, 1000), (64, 1), (64, 7), (64, 1000), (63, 5000)])
def test_groupby(ND, orc, P, G):
    """(64, 7) and (64, 1): fewer groups than ranks — most owners receive nothing (their merge
    is an empty result of the right shape, their padded segment has bound 0)."""
    n = 3000 * P + 3
    key, vd, vi = groupby_cols(orc, n, G)
    got = run_groupby(ND, P, shards(n, P), [key], [vd, vi], AGGS6, G)
    cmp_groups(got, want_groupby(orc, [key], [vd, vi], AGGS6, G))


def test_groupby_header_gather(ND, orc):
    """The gather to rank 0 with exact counts in a second header (dist.cpp kPaddedGather): the
    owners 1 .. P-1 would send 1 + W * bound_q words each, bound_q = the partial groups owner
    q receives.  Here W = 1 key + 6 aggregates = 7, and each of the 16 shards of 25,000 rows
    draws from 200,000 keys, so it holds about 200,000 (1 - e^-0.125) = 23,500 distinct keys:
    376,000 partial groups in all, 15/16 of them on owners 1 .. 15 -> 7 * 352,000 = 2.5e6
    words, above the 2^20 = 1,048,576 of the padded path.  The test computes the figure from
    its inputs with the host restatement of the owner hash and asserts it."""
    from nutdb_amd.dist import owner_of
    P, G, n = 16, 200_000, 400_003
    key, vd, vi = groupby_cols(orc, n, G, seed=0x10)
    W = 1 + len(AGGS6)
    gather_words = 0
    for a, b in shards(n, P):
        own = owner_of(np.unique(key[a:b]), None, P)
        gather_words += W * int(np.count_nonzero(own != 0))
    gather_words += P - 1
    assert gather_words > 1 << 20, gather_words
    got = run_groupby(ND, P, shards(n, P), [key], [vd, vi], AGGS6, G)
    cmp_groups(got, want_groupby(orc, [key], [vd, vi], AGGS6, G))


def test_groupby_empty_shards_at_64(ND, orc):
    """Every third shard empty and one shard of a single row."""
    P, G = 64, 1000
    sizes = [0 if r % 3 == 0 else 1 if r == 1 else 3000 + r for r in range(P)]
    n = sum(sizes)
    key, vd, vi = groupby_cols(orc, n, G, seed=0x20)
    got = run_groupby(ND, P, cuts_of(sizes), [key], [vd, vi], AGGS6, G)
    cmp_groups(got, want_groupby(orc, [key], [vd, vi], AGGS6, G))


def test_groupby_no_row_passes(ND, orc):
    """A predicate that rejects every row on every rank: 0 groups, no error."""
    P, G = 9, 1000
    n = 3000 * P + 3
    key, vd, vi = groupby_cols(orc, n, G, seed=0x30)
    pc = orc.gen_column(5, 0x54, n, a=0, b=100)
    pred = (pc, "<", 0)
    got = run_groupby(ND, P, shards(n, P), [key], [vd, vi], AGGS6, G, pred=pred)
    want = want_groupby(orc, [key], [vd, vi], AGGS6, G, pred=pred)
    assert len(want[0]) == 0 and len(got[0]) == 0
    cmp_groups(got, want)


def test_groupby_two_keys_at_33(ND, orc):
    P = 33
    n = 3000 * P + 3
    k1 = orc.gen_column(5, 0x61, n, a=-20, b=50)
    k2 = orc.gen_column(5, 0x62, n, a=-7, b=40)
    _, vd, vi = groupby_cols(orc, n, 1, seed=0x40)
    pc = orc.gen_column(5, 0x63, n, a=0, b=100)
    pred = (pc, "<=", 69)
    got = run_groupby(ND, P, shards(n, P), [k1, k2], [vd, vi], AGGS6, 2000, pred=pred)
    want = want_groupby(orc, [k1, k2], [vd, vi], AGGS6, 2000, pred=pred)
    assert len(want[0]) == 2000
    cmp_groups(got, want)


def test_groupby_eight_aggregates_at_9(ND, orc):
    """8 aggregates, more than the 4 fused value slots: the owner merge runs in expression mode."""
    P, G = 9, 1000
    n = 3000 * P + 3
    key, vd, vi = groupby_cols(orc, n, G, seed=0x50)
    got = run_groupby(ND, P, shards(n, P), [key], [vd, vi], AGGS8, G)
    cmp_groups(got, want_groupby(orc, [key], [vd, vi], AGGS8, G))


# -------------------------------------------------------------------------------- filter
@pytest.mark.parametrize("k,some", [(int(0.3 * 2**62), True), (0, False)])
@pytest.mark.parametrize("P", [9, 64])
def test_filter_offsets(ND, orc, P, k, some):
    """Uneven shards, empty ones included; a constant selecting ~30 % of the rows and one
    selecting nothing.  Offsets are the prefix sums of the ranks' counts."""
    sizes = [0 if r % 4 == 2 else 1 if r % 4 == 3 else 500 + 731 * (r % 7) for r in range(P)]
    n = sum(sizes)
    col = orc.gen_column(0, 0x2A + P, n)  # uniform over [0, 2^62)
    d = ND.virtual(P)
    try:
        res = d.filter_i64([dev(col[a:b]) for a, b in cuts_of(sizes)], "<", k)
        res = [(v.cpu().numpy(), off) for v, off in res]
    finally:
        d.close()
    want = orc.filter_i64(col, 0, k)
    assert (len(want) > 0.25 * n) if some else len(want) == 0
    pos = 0
    for (v, off), (a, b) in zip(res, cuts_of(sizes)):
        assert off == pos
        assert np.array_equal(v, col[a:b][col[a:b] < k])
        pos += len(v)
    assert pos == len(want)
    assert np.array_equal(np.concatenate([v for v, _ in res]), want)


# ---------------------------------------------------------------------------------- join
HOWS = ["inner", "left", "semi", "anti"]


def run_join(d, b, p, bcuts, pcuts, how, bshift=0, pshift=0):
    res = d.join_i64([dev(b[x:y]) for x, y in bcuts], [dev(p[x:y]) for x, y in pcuts], how,
                     [x + bshift for x, _ in bcuts], [x + pshift for x, _ in pcuts])
    gp = np.concatenate([r[0].cpu().numpy() for r in res])
    gb = np.concatenate([r[1].cpu().numpy() for r in res])
    return gp, gb


def check_join(orc, got, b, p, how, bshift=0, pshift=0):
    gp, gb = got
    wp, wb = orc.join_i64(b, p, how)
    wp = wp + pshift
    wb = np.where(wb >= 0, wb + bshift, -1)  # "no build row" stays -1
    assert len(gp) == len(wp) and len(gb) == len(wb), (len(gp), len(wp))
    og, ow = np.lexsort((gb, gp)), np.lexsort((wb, wp))
    assert np.array_equal(gp[og], wp[ow]) and np.array_equal(gb[og], wb[ow])


def join_one(ND, orc, P, b, p, how, bcuts=None, pcuts=None, bshift=0, pshift=0):
    bcuts = bcuts or shards(len(b), P)
    pcuts = pcuts or shards(len(p), P)
    d = ND.virtual(P)
    try:
        got = run_join(d, b, p, bcuts, pcuts, how, bshift, pshift)
    finally:
        d.close()
    check_join(orc, got, b, p, how, bshift, pshift)
    return got


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("P", [2, 9, 63, 64])
def test_join(ND, orc, P, how):
    """Both sides hold repeats and misses.  P = 63 and 64: the join's header is 5 + 2 P words,
    131 and 133 — wider than the group-by's, the sort's and the filter's."""
    nb, np_ = 20_000, 60_000
    b = orc.gen_column(5, 0x71, nb, a=0, b=60_000)
    p = orc.gen_column(5, 0x72, np_, a=0, b=80_000)
    join_one(ND, orc, P, b, p, how)


@pytest.mark.parametrize("how", HOWS)
def test_join_one_key_owns_every_build_row(ND, orc, how):
    """Every build key identical: one owner holds the whole build side and half the probe
    rows (300 x 1000 = 300,000 inner pairs on one rank), the other ranks only misses."""
    P, key = 9, 0x1234_5678_9ABC
    b = np.full(300, key, dtype=np.int64)
    p = orc.gen_column(5, 0x73, 2000, a=1, b=1_000_000)
    p[::2] = key
    gp, gb = join_one(ND, orc, P, b, p, how)
    assert len(gp) == {"inner": 300_000, "left": 301_000, "semi": 1000, "anti": 1000}[how]


@pytest.mark.parametrize("how", HOWS)
def test_join_extreme_keys(ND, orc, how):
    """INT64_MIN, INT64_MAX, -1 and 0 mixed into both sides, each repeated."""
    P = 9
    b = orc.gen_column(1, 0x74, 3000)
    p = orc.gen_column(1, 0x75, 9000)
    p[::3] = b[np.arange(3000)]  # a third of the probe rows match an ordinary build key
    ext = np.array([I64_MIN, I64_MAX, -1, 0], dtype=np.int64)
    b[5::40] = ext[np.arange(len(b[5::40])) % 4]
    p[7::30] = ext[np.arange(len(p[7::30])) % 4]
    p[1::600] = I64_MAX - 1  # a neighbour of an extreme that matches nothing
    assert all((b == x).sum() > 1 and (p == x).sum() > 1 for x in ext)
    join_one(ND, orc, P, b, p, how)


def test_join_empty_sides(ND, orc):
    """An empty build side on every rank, an empty probe side on every rank, and both sides
    with empty shards on some ranks — every join type, on one nut_dist."""
    P = 9
    b = orc.gen_column(5, 0x76, 4000, a=0, b=6000)
    p = orc.gen_column(5, 0x77, 9000, a=0, b=8000)
    none = np.zeros(0, np.int64)
    bsz = [0 if r % 3 == 0 else 4000 // 6 for r in range(P)]
    bsz[-1] += 4000 - sum(bsz)
    psz = [0 if r % 2 == 1 else 9000 // 5 for r in range(P)]
    psz[-1] += 9000 - sum(psz)
    assert sum(bsz) == 4000 and sum(psz) == 9000 and min(bsz) == 0 and min(psz) == 0
    d = ND.virtual(P)
    try:
        for how in HOWS:
            check_join(orc, run_join(d, none, p, [(0, 0)] * P, shards(len(p), P), how), none, p, how)
            check_join(orc, run_join(d, b, none, shards(len(b), P), [(0, 0)] * P, how), b, none, how)
            check_join(orc, run_join(d, none, none, [(0, 0)] * P, [(0, 0)] * P, how), none, none, how)
            check_join(orc, run_join(d, b, p, cuts_of(bsz), cuts_of(psz), how), b, p, how)
    finally:
        d.close()


@pytest.mark.parametrize("how", HOWS)
def test_join_row_offsets_above_2_32(ND, orc, how):
    """build_row0 / probe_row0 shifted past 2^32: the pairs are the oracle's plus the shifts,
    and "no build row" stays -1."""
    P = 9
    b = orc.gen_column(5, 0x78, 5000, a=0, b=8000)
    p = orc.gen_column(5, 0x79, 15_000, a=0, b=10_000)
    gp, gb = join_one(ND, orc, P, b, p, how, bshift=1 << 33, pshift=3 << 33)
    assert gp.min() >= 3 << 33
    if how == "inner":
        assert gb.min() >= 1 << 33
    elif how == "left":
        assert (gb == -1).any() and gb[gb != -1].min() >= 1 << 33
    else:
        assert np.all(gb == -1)


# ------------------------------------------------------- one nut_dist, call after call
@pytest.mark.parametrize("P", [8, 64])
def test_reuse_steady_state_and_regrowth(ND, orc, P):
    """Group-by, sort and join on ONE nut_dist, three rounds: first use (every buffer is
    allocated), then smaller inputs (no buffer grows: the calls skip the second all-gather
    that agrees on reservations), then inputs 3x the first (every buffer grows).  The three
    operators share the members' buffers 0 - 9; every result is checked exactly."""
    d = ND.virtual(P)
    try:
        for rnd, rows in enumerate((3000, 1000, 9000)):
            seed = 0x100 * (rnd + 1)
            # group-by
            from nutdb_amd import Agg, AggQuery
            n = rows * P + 3
            G = 1000
            key, vd, vi = groupby_cols(orc, n, G, seed=seed)
            qs = [AggQuery(keys=[dev(key[a:b])], values=[dev(vd[a:b]), dev(vi[a:b])],
                           aggs=[Agg(op, "col", args) for op, args in AGGS6], rows=b - a) for a, b in shards(n, P)]
            out = d.groupby(qs, group_hint=G)
            assert out[0] is not None and all(o is None for o in out[1:])
            got = out[0].to_host_words()
            out[0].free()
            cmp_groups(got, want_groupby(orc, [key], [vd, vi], AGGS6, G))
            # sort: a heavy key, so the equal-key buckets and their split run every round
            n = 2 * rows * P + 7
            k = orc.gen_column(1, 0x5500 + seed, n)
            k[np.random.default_rng(seed).random(n) < 0.4] = 99
            parts = [k[a:b] for a, b in shards(n, P)]
            outs = [o.cpu().numpy() for o in d.sort_i64([dev(s) for s in parts])]
            check_sort(outs, parts, P)
            # join
            nb, np_ = rows * P // 3, rows * P
            b = orc.gen_column(5, 0x7A + seed, nb, a=0, b=2 * nb)
            p = orc.gen_column(5, 0x7B + seed, np_, a=0, b=3 * nb)
            how = HOWS[rnd]
            check_join(orc, run_join(d, b, p, shards(nb, P), shards(np_, P), how), b, p, how)
    finally:
        d.close()
