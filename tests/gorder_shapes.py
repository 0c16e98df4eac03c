"""Directed inputs for the ordered group-by's kernels (csrc/heavy.hpp, csrc/gpart.hpp, the phases
of aggregate.hip's groupby_ordered) and a host model of its sample
(numpy; no GPU).

The plan of an ordered group-by is a function of 65536 keys: go_sample_kernel reads rows
i * (n / 65536), and the key range, the admission, the heavy keys, their cuckoo table and the
layout follow from them (csrc/go_plan.hpp).  Every case here has n = 2^24 rows, or up to 4099
more, so the sampled rows are the multiples of 256 below 2^24.  A builder that writes a key on
sampled rows makes it heavy; one that stays off them hides a key from the plan.

The ordinary keys of a column lie on a grid (LO + position x STRIDE) and row r holds grid index
((r >> 8) A + (r & 255) C) mod g: the sampled rows (r & 255 = 0) hold 65536 distinct grid keys
spread over the whole range (A is coprime to g), so without directed keys the sample has no
repeats, the admission passes and every range cell holds about n / 16384 rows.

The model below restates go_plan.hpp (range, cell, heavy-key choice, cuckoo table) to PLACE keys.
tests/test_gorder_shapes_cpu.py proves every note from the plan driver (tests/c/test_go_plan.cpp,
which includes go_plan.hpp itself) and from the oracle; the model never produces an expected
result — the reference is always oracle.groupby.

A builder returns Case(name, keys, hint, opts, note).  note:
  heavy       the heavy keys the plan must choose (ascending int64 array; empty: no heavy pass)
  heavy_rows  the rows the heavy pass must take
  decline     "none", or why the ordered path must decline
  exact       the layout behind the heavy pass under the default options (None: declined before)
  arenas      True: rows must go through the overflow arenas; False: none may (exact layout, or a
              capped one whose every cell fits its region: test_capped_cells_fit); None: not stated
  arenas_capped  the same under gb_heavy = 2 (the capped layout behind the heavy pass)
  hq_missing  the heavy keys whose level-0 digit holds no kept row (hq = -1: the host folds them)
  digits      the non-empty level-0 digits of the kept rows at gb_l0_bits = 7 (None: not stated)
  groups      the distinct keys
and whatever a case states beyond that.

Values (value_columns): f64 columns are dyadic — multiples of 2^-10 below 2^19 in magnitude, some
-0.0 — so a group of up to 2^24 rows sums exactly in any order (2^24 x 2^19 x 2^10 = 2^53);
int64 columns either stay below 2^40 or span all 64 bits (wrapping sums).  Every comparison with
the oracle is therefore bit for bit."""
from collections import namedtuple

import numpy as np

from helpers import mix64

I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1
M64 = (1 << 64) - 1
SAMPLE = 1 << 16
N0 = 1 << 24          # the fewest rows the ordered path takes
STEP = N0 // SAMPLE   # the sample's stride (also at N0 + 4099 rows)
CELLS = 1 << 14
HK_TILE, HK_MAX, HK_WORDS, HK_SLOTS = 2048, 2048, 2048, 8192
HINT = 100 * CELLS    # the smallest hint (100 groups per range cell)
G0 = 1 << 18          # grid positions
LO, STRIDE = -(1 << 62), 1 << 45   # the grid of the "full" geometry: [-2^62, 2^62)
A_MUL, C_MUL = 165667, 1031
SEED0 = 0x9E3779B97F4A7C15
ORDERED = "partitioned_ordered"
GEOMS = {  # name -> (first key, stride): span / 2^18 keys
    "full": (LO, STRIDE),                  # t > 0; straddles 0
    "dense": (0, 1),                       # ids 0 .. g - 1: t = 0, and sh = 0 in every partition's ordering
    "negative": (-(1 << 62), 1 << 40),     # all keys < 0
    "straddle": (-(1 << 30), 1 << 13),     # t = 0 around 0
}

Case = namedtuple("Case", "name keys hint opts note")


# ----------------------------------------------------------------------------- the model (go_plan.hpp)
def biased(k):
    """signed keys as the unsigned words whose order is the keys' order"""
    return np.asarray(k, dtype=np.int64).view(np.uint64) ^ np.uint64(1 << 63)


def signed(u):
    u = int(u) ^ (1 << 63)
    return u - (1 << 64) if u >> 63 else u


def go_range(smin, smax):
    """go_range: (lo, span, t, mul), or None where the span is below 2^16"""
    lo, hi = (int(smin) & M64) ^ (1 << 63), (int(smax) & M64) ^ (1 << 63)
    margin = (hi - lo) >> 10
    lo = lo - margin if lo > margin else 0
    hi = hi + margin if hi < M64 - margin else M64
    span = hi - lo
    if span < 1 << 16:
        return None
    t = span.bit_length() - 32 if span >> 32 else 0
    return lo, span, t, (1 << 46) // ((span >> t) + 1)


def cell(rg, keys):
    """GpRange::cell of every key"""
    lo, span, t, mul = rg
    u = biased(np.atleast_1d(keys))
    with np.errstate(over="ignore"):
        x = np.where(u < np.uint64(lo), np.uint64(0), np.minimum(u - np.uint64(lo), np.uint64(span)))
    return (((x >> np.uint64(t)) * np.uint64(mul)) >> np.uint64(32)).astype(np.int64)


def sample_of(keys):
    """what go_sample_kernel reads"""
    return keys[::len(keys) // SAMPLE][:SAMPLE]


def range_of(keys):
    s = sample_of(keys)
    return go_range(s.min(), s.max())


def heavy_max(na):
    return min(HK_MAX, HK_WORDS // na)


def heavy_model(sample, na):
    """go_heavy_keys: the <= heavy_max(na) most frequent of the keys sampled >= 3 times (ties: the
    smaller key), if together they hold >= 5 % of the sample; ascending"""
    k, c = np.unique(sample, return_counts=True)
    k, c = k[c >= 3], c[c >= 3]
    order = np.lexsort((k, -c))[:heavy_max(na)]
    if int(c[order].sum()) * 20 < SAMPLE:
        return np.empty(0, np.int64)
    return np.sort(k[order])


def seeds(attempt=0):
    return int(mix64(SEED0 + 2 * attempt)[0]), int(mix64(SEED0 + 2 * attempt + 1)[0])


def hk_slot(k, seed):
    return ((mix64(np.asarray(k, dtype=np.int64).view(np.uint64) ^ np.uint64(seed)) >> np.uint64(32))
            & np.uint64(HK_SLOTS - 1)).astype(np.int64)


def cuckoo(hkeys, attempt=0):
    """hk_cuckoo with attempt 0's seeds: slot[HK_SLOTS] (key index + 1; 0: empty), or None"""
    s1, s2 = seeds(attempt)
    a, b = hk_slot(hkeys, s1).tolist(), hk_slot(hkeys, s2).tolist()
    slot = [0] * HK_SLOTS
    for j in range(len(hkeys)):
        cur, pos, steps = j + 1, a[j], 0
        while True:
            old, slot[pos] = slot[pos], cur
            if not old:
                break
            steps += 1
            if steps > 1000:
                return None
            cur = old
            pos = b[old - 1] if pos == a[old - 1] else a[old - 1]
    return np.array(slot, dtype=np.int64)


# ----------------------------------------------------------------------------- columns
def grid_index(n, g):
    r = np.arange(n, dtype=np.int64)
    return ((r >> 8) * A_MUL + (r & 255) * C_MUL) % g


def grid_keys(n, geom="full", g=G0):
    lo, stride = GEOMS[geom]
    return lo + grid_index(n, g) * stride


def okey(pos, geom="full"):
    lo, stride = GEOMS[geom]
    return lo + np.asarray(pos, dtype=np.int64) * stride


def sampled_slots():
    """the sampled rows in an order that spreads consecutive picks over the column"""
    return ((np.arange(SAMPLE, dtype=np.int64) * 40503 + 12345) & (SAMPLE - 1)) * STEP


def put_sampled(keys, hkeys, counts):
    """heavy key j on counts[j] sampled rows (and on no other row); the rows of the sample's least
    and greatest key stay as they are, so keys inside the sampled range leave the range alone"""
    counts = np.broadcast_to(np.asarray(counts, dtype=np.int64), (len(hkeys),))
    total = int(counts.sum())
    s = sample_of(keys)
    slots = sampled_slots()
    slots = slots[~np.isin(slots, [int(s.argmin()) * STEP, int(s.argmax()) * STEP])]
    assert total <= len(slots)
    keys[slots[:total]] = np.repeat(np.asarray(hkeys, dtype=np.int64), counts)


def unsampled_rows(m, first=1000, step=37):
    """m distinct rows that are no sampled rows"""
    i = np.arange(m, dtype=np.int64)
    r = STEP * (first + step * i) + 1 + (i % 254)
    assert r.max() < N0 and np.all(r % STEP != 0)
    return r


def _case(name, keys, heavy=(), hint=HINT, opts=None, decline="none", exact=None, arenas=None, hq_missing=(),
          digits=None, arenas_capped=None, **more):
    heavy = np.sort(np.asarray(heavy, dtype=np.int64))
    note = dict(heavy=heavy, heavy_rows=int(np.isin(keys, heavy).sum()) if len(heavy) else 0, decline=decline,
                arenas_capped=arenas_capped,
                exact=(len(heavy) > 0 if exact is None and decline == "none" else exact), arenas=arenas,
                hq_missing=np.sort(np.asarray(hq_missing, dtype=np.int64)), digits=digits,
                groups=int(len(np.unique(keys))))
    if note["exact"] and arenas is None:
        note["arenas"] = False
    note.update(more)
    return Case(name, np.ascontiguousarray(keys), hint, dict(opts or {}), note)


def few_heavy(geom="full", m=8, g=G0):
    """m keys beside grid keys spread over the range; 512 sampled rows each make them the heavy set
    (m x 512 >= 5 % of the sample) for every aggregate count"""
    return okey((np.arange(m, dtype=np.int64) * 2 + 1) * (g // (2 * m)), geom) + 1


# ----------------------------------------------------------------------------- builders
def plain(geom="full", n=N0, hint=HINT):
    """grid keys alone: no repeats in the sample, no heavy pass, capped layout, every cell within
    its region"""
    return _case(f"plain_{geom}_{n}_{hint}", grid_keys(n, geom), hint=hint, arenas=False)


def sampled_heavy(na):
    """The full heavy set: heavy_max(na) keys (2048 at one aggregate, 512 at four) on `each` sampled
    rows and on no other row, and 64 spare candidates on 3 sampled rows that the cut must drop (they
    stay ordinary keys).  The heavy keys hold well under 1 % of the rows."""
    hmax = heavy_max(na)
    each = max(4, -(-(SAMPLE // 20 + 1) // hmax) + 1)
    keys = grid_keys(N0)
    chosen = okey(np.arange(hmax, dtype=np.int64) * (G0 // hmax)) + 1
    spare = okey(np.arange(64, dtype=np.int64) * 4096 + 2048) + 3
    put_sampled(keys, np.concatenate([chosen, spare]), np.concatenate([np.full(hmax, each), np.full(64, 3)]))
    return _case(f"sampled_heavy_na{na}", keys, chosen, spare=spare, each=each, na=na, arenas_capped=False)


def hidden_key(m=8, with_heavy=False):
    """One key on m / 256 of the rows (m = 8: 3 %), none of them sampled.  Alone the sample has no
    repeats: no heavy pass, the capped layout, and the key's rows past its regions go through both
    arenas.  Beside a sampled heavy set the layout is exact and the key is one huge cell."""
    keys = grid_keys(N0)
    x = int(okey(G0 // 3)) + 5
    r = np.arange(N0, dtype=np.int64) & 255
    keys[(r >= 1) & (r <= m)] = x
    heavy = few_heavy() if with_heavy else ()
    if with_heavy:
        put_sampled(keys, heavy, 512)
    return _case(f"hidden_key_{m}_{int(with_heavy)}", keys, heavy, arenas=not with_heavy, hidden=x,
                 arenas_capped=True if with_heavy else None,
                 hidden_rows=m * (N0 // 256))


# rows of heavy_blocks' placements (tiles of 2048 rows; blocks of >= 2^20 rows, so that they hold
# whole workgroups of any heavy-pass grid: a workgroup reads at most 32 tiles = 2^16 rows at >= 256
# workgroups)
MI = 1 << 20
HB_ALL = (1 * MI, 3 * MI)          # 2^21 rows, every one heavy: whole tiles and whole workgroups keep nothing
HB_ONE_PER_TILE = (4 * MI, 5 * MI)  # every tile keeps exactly one row, at a varying lane and item
HB_ALTERNATE = (6 * MI, 7 * MI)    # odd rows heavy, even rows kept
HB_EDGES = 8 * MI                  # blocks that begin and end in mid-tile
HB_ONE_PER_WG = (10 * MI, 11 * MI)  # one kept row in the middle of 2^20 heavy rows: its workgroup keeps one row
HB_EDGE_BLOCKS = [(1000, 1), (3000, 63), (5000, 64), (7000, 65), (9000, 2047), (13000, 2049), (20000 + 1024, 2048),
                  (30000 + 2047, 2), (40000, 4096 + 1)]


def heavy_blocks(tail=0, last_heavy=False):
    """One heavy key H placed by tile and by block (HB_*), in a column of 2^24 + tail rows whose last
    row is heavy or kept."""
    n = N0 + tail
    keys = grid_keys(n)
    h = int(okey(G0 // 2)) + 1
    keys[HB_ALL[0]:HB_ALL[1]] = h
    a, b = HB_ONE_PER_TILE
    keep = keys[a:b].copy()
    keys[a:b] = h
    t = np.arange((b - a) // HK_TILE, dtype=np.int64)
    at = t * HK_TILE + (t * 389 + 7) % HK_TILE
    keys[a + at] = keep[at]
    keys[HB_ALTERNATE[0] + 1:HB_ALTERNATE[1]:2] = h
    for off, ln in HB_EDGE_BLOCKS:
        keys[HB_EDGES + off:HB_EDGES + off + ln] = h
    a, b = HB_ONE_PER_WG
    lone = a + (b - a) // 2 + 123
    keep1 = keys[lone]
    keys[a:b] = h
    keys[lone] = keep1
    if last_heavy:
        keys[n - 1] = h
    return _case(f"heavy_blocks_{tail}_{int(last_heavy)}", keys, [h], lone_row=lone, arenas_capped=False)


def gap(logp=18, s=6, hidden=False):
    """Grid keys (2^logp positions) over the lower s/16 and the upper s/16 of the range, the middle
    empty, and twelve sampled heavy keys: four inside the empty middle (hq = -1; two of them
    adjacent), two adjacent keys k, k + 1 inside one populated cell, one below and one above all of
    its cell's own keys, one in a cell without another key (at the gap's edge, in a level-0 digit
    that has rows: a partition of one group), two adjacent keys in another such cell (a partition of
    exactly two groups), one plain.  logp = 22, s = 7: 3.67 M groups, more than twice the smallest hint.
    hidden: also a key on 3 % of the rows, none sampled, and 16 keys of its cell on 4 rows each in
    the column's last eighth (under gb_heavy = 2 the capped layout sends them through the arenas)."""
    P = 1 << logp
    stride = 1 << (63 - logp)
    lower = s * (P // 16)

    def ok(pos):
        return LO + np.asarray(pos, dtype=np.int64) * stride
    g = 2 * lower
    j = grid_index(N0, g)
    keys = ok(np.where(j < lower, j, j + P - g))
    # (capped behind the heavy pass, the digits at the gap's edges hold rows in a few cells only: their
    # level-1 regions, sized from the digit's even share, overflow into the arena)
    extra = dict(arenas_capped=True)
    if hidden:
        x = int(ok(P // 8)) + 5
        r = np.arange(N0, dtype=np.int64) & 255
        keys[(r >= 1) & (r <= 8)] = x
        late = x + 1 + np.arange(16, dtype=np.int64)
        keys[unsampled_rows(64, first=60000, step=17)] = np.repeat(late, 4)
        extra = dict(hidden=x, late=late, arenas_capped=True)
    rg = range_of(keys)
    allpos = np.concatenate([np.arange(lower), np.arange(P - lower, P)]).astype(np.int64)
    pcell = cell(rg, ok(allpos))
    q = P // 64
    mid = [int(ok(P // 2)) + 1, int(ok(P // 2 + q)) + 1, int(ok(P // 2 - q)) + 1, int(ok(P // 2 - q)) + 2]
    adj = [int(ok(5 * q)) + 1, int(ok(5 * q)) + 2]
    c1, c2 = int(pcell[10 * q]), int(pcell[allpos.searchsorted(P - 14 * q)])
    below = int(ok(allpos[pcell == c1].min())) - 1
    above = int(ok(allpos[pcell == c2].max())) + 1
    used_cells, used_digits = set(pcell.tolist()), set((pcell >> 7).tolist())
    empty = []  # one key in each of the first two empty cells of a non-empty digit above the lower part
    for p in range(lower + P // 8192, lower + P // 128, max(1, P // 16384)):
        k = int(ok(p)) + 1
        c = int(cell(rg, k)[0])
        if c not in used_cells and c >> 7 in used_digits and c not in [x[1] for x in empty]:
            empty.append((k, c))
            if len(empty) == 2:
                break
    assert len(empty) == 2
    alone, pair = empty[0][0], [empty[1][0], empty[1][0] + 1]
    plain_h = int(ok(P - 8 * q)) + 1
    heavy = mid + adj + [below, above, alone, plain_h] + pair
    assert len(set(heavy)) == 12
    put_sampled(keys, heavy, 400)
    assert range_of(keys) == rg
    hc = cell(rg, np.array(heavy))
    assert hc[2] == hc[3] and hc[4] == hc[5] and hc[6] == c1 and hc[7] == c2 and hc[10] == hc[11] != hc[8]
    assert all(int(c) >> 7 not in used_digits for c in hc[:4])
    return _case(f"gap_{logp}_{s}_{int(hidden)}", keys, heavy, hq_missing=mid, digits=len(used_digits), adjacent=adj,
                 below=below, above=above, alone=alone, pair=pair, middle=mid, **extra)


def outlier_keys(rg):
    """24 keys below the range and 24 above it, INT64_MIN and INT64_MAX among them"""
    lo_s, hi_s = signed(rg[0]), signed(rg[0] + rg[1])
    assert lo_s > I64_MIN + 64 and hi_s < I64_MAX - 64
    db, da = (lo_s - I64_MIN) // 32, (I64_MAX - hi_s) // 32
    below = [I64_MIN, I64_MIN + 1] + [lo_s - 1 - i * db for i in range(22)]
    above = [I64_MAX, I64_MAX - 1] + [hi_s + 1 + i * da for i in range(22)]
    return np.array(sorted(set(below))), np.array(sorted(set(above)))


def outliers(geom="full"):
    """48 distinct keys outside [lo, lo + span], on 8 unsampled rows each: they clamp to cells 0 and
    16383, which stay within their regions and tables."""
    keys = grid_keys(N0, geom)
    rg = range_of(keys)
    below, above = outlier_keys(rg)
    out = np.concatenate([below, above])
    keys[unsampled_rows(8 * len(out))] = np.repeat(out, 8)
    assert range_of(keys) == rg
    return _case(f"outliers_{geom}", keys, arenas=False, below=below, above=above, t=rg[2])


def smallest_span():
    """the largest grid key M of ids 0 .. M at which the range (with its margins) reaches 2^16"""
    m = 1 << 16
    while go_range(0, m - 1) is not None:
        m -= 1
    return m


def tiny_span(accepted=True):
    """ids 0 .. M with the smallest accepted sampled span (M = smallest_span()), and M - 1, which
    the plan declines ("shape"); outliers as above on the accepted one"""
    m = smallest_span() - (0 if accepted else 1)
    keys = grid_keys(N0, "dense", g=m + 1)
    s = sample_of(keys)
    assert s.min() == 0 and s.max() == m
    if not accepted:
        return _case("tiny_span_declined", keys, decline="shape", top=m)
    rg = range_of(keys)
    below, above = outlier_keys(rg)
    out = np.concatenate([below, above])
    keys[unsampled_rows(8 * len(out))] = np.repeat(out, 8)
    return _case("tiny_span", keys, arenas=False, below=below, above=above, t=rg[2], top=m)


def cuckoo_neighbours(na):
    """The full heavy set of sampled_heavy(na) and 64 kept keys (4 unsampled rows each) whose two
    cuckoo slots both name heavy keys; second_slot: the heavy keys that sit in their second slot."""
    base = sampled_heavy(na)
    keys = base.keys.copy()
    heavy = base.note["heavy"]
    slot = cuckoo(heavy)
    assert slot is not None
    s1, s2 = seeds()
    first = hk_slot(heavy, s1)
    second = heavy[slot[first] != np.arange(1, len(heavy) + 1)]
    cand = okey(np.arange(G0, dtype=np.int64)) + 7
    hit = cand[(slot[hk_slot(cand, s1)] != 0) & (slot[hk_slot(cand, s2)] != 0)][:64]
    assert len(hit) == 64 and len(second) > 0
    keys[unsampled_rows(4 * 64)] = np.repeat(hit, 4)
    return _case(f"cuckoo_na{na}", keys, heavy, neighbours=hit, second_slot=second, na=na, arenas_capped=False)


def identity_keys():
    """few_heavy's set on sampled rows; its first key Z is the one whose values identity_columns makes
    equal to every aggregate kind's initial word, its second key Y the one whose aggregates equal
    another kind's initial word"""
    keys = grid_keys(N0)
    heavy = few_heavy()
    put_sampled(keys, heavy, 512)
    return _case("identity", keys, heavy, z=int(heavy[0]), y=int(heavy[1]), arenas_capped=False)


def clustered():
    """half the grid's keys packed into one range cell (consecutive integers): half the sample's
    distinct keys fall into one level-0 digit and the admission declines before any work"""
    j = grid_index(N0, G0)
    keys = np.where(j < G0 // 2, okey(2 * j), int(okey(100000)) + 1 + (j - G0 // 2))
    return _case("clustered", keys, decline="clustered")


# ---- declines after work has started
def arena_level0():
    """a hidden key on 154 / 256 = 60 % of the rows: level 0's arena (about n / 2 rows) is exhausted"""
    c = hidden_key(154)
    return _case("arena_level0", c.keys, decline="arena", hidden=c.note["hidden"], hidden_rows=c.note["hidden_rows"])


def arena_level1():
    """128 hidden keys, one per level-0 digit, together on 60 % of the rows: every level-0 region
    holds its even share, and each key's level-1 cell overflows by ~77 K rows — 9.8 M rows for level
    1's arena of n / 2"""
    keys = grid_keys(N0)
    rg = range_of(keys)
    hid = okey(np.arange(128, dtype=np.int64) * 2048 + 1024) + 5
    assert np.array_equal(cell(rg, hid) >> 7, np.arange(128))
    r = np.arange(N0, dtype=np.int64)
    m = ((r & 255) >= 1) & ((r & 255) <= 154)
    keys[m] = hid[(r[m] >> 8) & 127]
    return _case("arena_level1", keys, decline="arena", hidden=hid)


def table_overflow():
    """One cell whose rows all hold distinct hidden keys (its ~1024 own rows and 3000 more, none
    sampled — the cell's sampled rows move to a neighbouring cell's key): whatever rows its capped
    region takes, they are more distinct keys than a partition's table admits."""
    keys = grid_keys(N0)
    rg = range_of(keys)
    p0 = 150000
    c = int(cell(rg, okey(p0))[0])
    own = np.flatnonzero(cell(rg, keys) == c)
    extra = np.setdiff1d(unsampled_rows(3000, first=2000, step=21), own)
    rows = np.concatenate([own, extra])
    first = int(okey(p0))
    hid = first + 2 + np.arange(len(rows), dtype=np.int64)
    assert np.all(cell(rg, hid) == c)
    keys[rows] = hid
    smp = rows[rows % STEP == 0]
    keys[smp] = okey(p0 + 64 + 16 * np.arange(len(smp)))  # (keys of other cells, sampled once more)
    assert range_of(keys) == rg and np.unique(sample_of(keys), return_counts=True)[1].max() < 3
    return _case("table_overflow", keys, decline="table", cell=c, cell_keys=int(len(rows) - len(smp)))


def level1_fits(d, na, hint=HINT, slots=0):
    """go_plan_level1 with d non-empty level-0 digits (gb_l0_bits = 7): does a partition's table fit
    the ordering pass?  From nut_groupby_layout."""
    from groupby_shapes import library_layout
    per = max(64, 2 * -(-hint // (d * 128)))
    lcap = library_layout(1, na, per, segment=1, slots=slots)["lds_cap"]
    return lcap != 0 and lcap + 1 <= 4097


def fewest_digits(na):
    d = 1
    while not level1_fits(d, na):
        d += 1
    return d


def few_digits(d, fits=True):
    """Kept rows in d level-0 digits only.  Two sampled heavy keys at the ends of the grid pin the
    range; the grid keys fill digits [40, 40 + d), 700 sampled rows per digit; 256 more heavy keys
    inside those digits take the other sampled rows (the admission allows 1040 distinct sampled keys
    per digit, heavy ones included).  With
    fewest_digits(na) - 1 digits go_plan_level1 declines ("capacity"), with fewest_digits(na) it
    fits."""
    g = d * 2048 - 600
    first = 40 * 2048 + 300
    keys = okey(first + grid_index(N0, g))
    ends = okey([0, G0 - 1])
    fill = okey(first + (np.arange(256, dtype=np.int64) * 2 + 1) * g // 512) + 1
    heavy = np.concatenate([ends, fill])
    rest = SAMPLE - 700 * d
    counts = np.concatenate([[64, 64], np.full(256, (rest - 128) // 256)])
    counts[2:2 + (rest - 128) % 256] += 1
    slots = sampled_slots()
    keys[slots[:rest]] = np.repeat(heavy, counts)
    # the other 700 d sampled rows: distinct grid keys, evenly spread over the d digits
    keys[slots[rest:]] = okey(first + np.arange(700 * d, dtype=np.int64) * g // (700 * d))
    rg = range_of(keys)
    digs = np.unique(cell(rg, okey(first + np.arange(g, dtype=np.int64))) >> 7)
    assert np.array_equal(digs, np.arange(40, 40 + d)) and set((cell(rg, fill) >> 7).tolist()) <= set(digs.tolist())
    return _case(f"few_digits_{d}", keys, heavy, hq_missing=ends, digits=d, d=d, exact=True,
                 decline="none" if fits else "capacity")


# ----------------------------------------------------------------------------- values and aggregates
# aggregate shapes: name -> (value column kinds, [(oracle op, column)]); ops: 0 SUM, 1 COUNT, 2 MIN, 3 MAX
# column kinds: "f" dyadic f64, "i" int64 below 2^40, "w" int64 over all 64 bits (wrapping sums), "k" the key column
SHAPES = {
    "count": ((), [(1, None)]),                                           # NV = 0
    "one": (("f",), [(0, 0), (1, None), (2, 0), (3, 0)]),                # NV = 1
    "keyval": (("k",), [(0, 0), (1, None), (2, 0), (3, 0)]),             # the value column IS the key column
    "three": (("f", "i", "f"), [(2, 0), (3, 1), (0, 2), (1, None)]),     # NV = 3: f64 MIN, i64 MAX, f64 SUM
    "four": (("w", "i", "f", "f"), [(0, 0), (2, 1), (0, 2), (3, 3), (3, 1)]),  # NV = 4, five aggregates
}


def shape_na(shape):
    return len(SHAPES[shape][1])


def value_column(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "f":
        v = rng.integers(-(1 << 29), 1 << 29, n).astype(np.float64) / 1024.0
        v[::97] = -0.0
        return v
    if kind == "i":
        return rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)
    assert kind == "w"
    return rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64)


def value_columns(shape, keys):
    return [keys if k == "k" else value_column(k, len(keys), 0x60 + i) for i, k in enumerate(SHAPES[shape][0])]


def oracle_aggs(shape):
    return [(op, 0, () if col is None else (col,)) for op, col in SHAPES[shape][1]]


# the initial words of the accumulators (gtable.hpp agg_init, as result words): the heavy pass's
# workgroup merge skips an accumulator that still equals them
NAN_MIN_ID = 0x7FFFFFFFFFFFFFFF  # f64 MIN starts at +NaN (all ones), the total order's greatest
NAN_MAX_ID = 0xFFFFFFFFFFFFFFFF  # f64 MAX at -NaN (all ones), its least
IDENTITY_SHAPES = {
    # i64: SUM wraps to 0 (every row 2^62; Z's rows are a multiple of 4), MIN of INT64_MAX, MAX of INT64_MIN
    "id_i64": (("i", "i", "i"), [(0, 0), (2, 1), (3, 2), (1, None)], (1 << 62, I64_MAX, I64_MIN)),
    # f64: SUM of only -0.0 (the accumulator starts at +0.0 and stays there), MIN of the +NaN, MAX of the -NaN
    "id_f64": (("f", "f", "f"), [(0, 0), (2, 1), (3, 2), (1, None)], (0x8000000000000000, NAN_MIN_ID, NAN_MAX_ID)),
}
IDENTITY_WORDS = {"id_i64": (0, I64_MAX, I64_MIN & M64), "id_f64": (0, NAN_MIN_ID, NAN_MAX_ID)}
# and a second heavy key Y whose aggregates equal the initial word of the NEXT aggregate's kind, not their own: the
# skip must compare with the accumulator's own kind (None: ordinary values).  i64: MIN of INT64_MIN (MAX's word), MAX
# of 0 (COUNT's); f64: MIN of the -NaN (MAX's word)
OTHER_KIND_WORDS = {"id_i64": (None, I64_MIN & M64, 0), "id_f64": (None, NAN_MAX_ID, None)}


def identity_columns(shape, case):
    """value columns of identity_keys(): ordinary values; on Z's rows the words that leave every
    accumulator at its initial word; on Y's rows OTHER_KIND_WORDS"""
    kinds, _, words = IDENTITY_SHAPES[shape]
    z, y = case.keys == case.note["z"], case.keys == case.note["y"]
    assert int(z.sum()) % 4 == 0 and int(y.sum()) > 0
    cols = []
    for i, (k, w, o) in enumerate(zip(kinds, words, OTHER_KIND_WORDS[shape])):
        v = value_column(k, len(case.keys), 0x70 + i)
        v.view(np.uint64)[z] = np.uint64(w & M64)
        if o is not None:
            v.view(np.uint64)[y] = np.uint64(o)
        cols.append(v)
    return cols


def identity_aggs(shape):
    return [(op, 0, () if col is None else (col,)) for op, col in IDENTITY_SHAPES[shape][1]]
