"""Directed inputs for the group-by tables (csrc/agg_kernel.hpp, csrc/gtable.hpp) and a host
model of their layout arithmetic (numpy; no GPU).

The model restates csrc/gb_layout.hpp.  On-chip (LDS) table of a workgroup: a power of two of
slots sized from the hint, admitting 3/4 of them; a key's slot word is the key itself (one
key) or a 64-bit hash of the tuple nudged off the empty marker (two keys); its home is a
4-slot bucket, the top bits of a 32-bit Fibonacci hash of the word's xor-fold; new keys go
to the first empty slot from the bucket's start, wrapping at the table's end.  Global (HBM)
table: slot = top bits of hash x golden ratio, hash = the key (one key) or mix64 of the
tuple, whose top half is the tag stored beside an arena index; tables of 2^18 slots and
more count claims in 256 shards (the slot's low bits) and arena entries in 256 shards (the
tag's low bits).  Every one of these maps is a bijection on some word, so the builders below
COMPUTE keys with a chosen bucket, slot word, slot, tag, shard, owner or digit.
tests/test_groupby_shapes_cpu.py pins `layout` to the library's own arithmetic
(nut_groupby_layout) and proves that every builder holds what its note says.  The model
never produces an expected result: the reference is always the oracle (oracle.groupby).

What the model can say about racing inserts: under linear probing the SET of occupied
slots does not depend on the insertion order, so chain lengths and wraps are exact; WHICH
key of a chain sits where is the race's.

A builder returns Case(name, nk, keys, hint, note): keys = nk int64 arrays of the K distinct
key tuples.  rows() turns a case into key and value columns."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from helpers import _u64, mix64, unmix64

I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
GOLDEN_INV = pow(GOLDEN, -1, 1 << 64)
LK_ADD, LK_MUL = 0x632BE59BD9B4E019, 0xC2B2AE3D27D4EB4F      # lkey<2>
LK_MUL_INV = pow(LK_MUL, -1, 1 << 64)
FIB32 = 0x9E3779B1                                            # lhome
FIB32_INV = pow(FIB32, -1, 1 << 32)
OWNER_C = 0x6A09E667F3BCC908                                  # owner_hash
EMPTY = 1 << 63                                               # kEmpty: the single-key tables' empty marker
BUCKET, DIRECT, PRIV_MAX = 4, 256, 8
BD_SHARED, BD_PRIV, BD_TUNED, TUNED_BLOCKS = 512, 256, 192, 2
LDS_MAX = 160 * 1024 - 2048
NUT_MAX_AGGS = 8

Case = namedtuple("Case", "name nk keys hint note")


def _i64(x):
    return np.ascontiguousarray(_u64(x)).view(np.int64)


def _mul(a, b):
    with np.errstate(over="ignore"):
        return _u64(a) * np.uint64(b)


def _add(a, b):
    with np.errstate(over="ignore"):
        return _u64(a) + np.uint64(b)


def _log2(cap):
    l2 = int(cap).bit_length() - 1
    assert cap > 0 and 1 << l2 == cap
    return l2


# ----------------------------------------------------------------------------- the model: on-chip table
def lkey2(k1, k2):
    """lkey<2>: two odd multiplies, an xorshift, and the nudge off the empty marker."""
    h = _mul(k1, GOLDEN) ^ _mul(_add(k2, LK_ADD), LK_MUL)
    h = h ^ (h >> np.uint64(29))
    return np.where(h == np.uint64(EMPTY), h ^ np.uint64(1), h)


def lkey(nk, k1, k2=0):
    return _u64(k1) if nk == 1 else lkey2(k1, k2)


def lhome(w, cap):
    w = _u64(w)
    f = (w ^ (w >> np.uint64(32))) & np.uint64(0xFFFFFFFF)
    p = (f * np.uint64(FIB32)) & np.uint64(0xFFFFFFFF)
    return ((p >> np.uint64(32 - _log2(cap))) & np.uint64(~(BUCKET - 1) & 0xFFFFFFFF)).astype(np.int64)


def direct_idx(nk, k1, k2=0):
    k1, k2 = _u64(k1), _u64(k2)
    if nk == 1:
        return np.where(k1 < np.uint64(DIRECT), k1, np.uint64(DIRECT)).astype(np.int64)
    return np.where((k1 | k2) < np.uint64(16), (k1 << np.uint64(4)) | k2, np.uint64(DIRECT)).astype(np.int64)


def lds_bytes(cap, nk, na, priv, P, bd):
    if cap == 0:
        return 0
    al = lambda o: (o + 15) & ~15  # noqa: E731
    stride = cap + 1
    o = al(stride * 8 * (1 + na))
    if nk == 2:
        o += stride * 16
    if priv:
        o += stride * 4 + (PRIV_MAX + DIRECT) * 4
    o = al(o + 16)
    if priv:
        o += P * na * bd * 8
    return al(o)


def lds_cap(nk, na, hint, slots=4):
    want = slots * hint if hint else 4096
    cap = 32
    while cap < want and lds_bytes(cap * 2, nk, na, False, 0, BD_SHARED) <= LDS_MAX:
        cap *= 2
    return 0 if hint > 8 * cap else cap


def lds_limit(cap):
    return cap - cap // 4


def priv_groups(cap, nk, na, hint, seg=False):
    if cap and hint and hint <= PRIV_MAX and na > 0 and not seg:
        if lds_bytes(cap, nk, na, True, hint, BD_PRIV) <= LDS_MAX // 2:
            return hint
    return 0


# ----------------------------------------------------------------------------- the model: global table
def key_hash(nk, k1, k2=0):
    return _u64(k1) if nk == 1 else mix64(_u64(k1) ^ mix64(_add(k2, GOLDEN)))


def slot_of(h, cap):
    return (_mul(h, GOLDEN) >> np.uint64(64 - _log2(cap))).astype(np.int64)


def owner_hash(nk, k1, k2=0):
    h = mix64(_u64(k1) ^ np.uint64(OWNER_C))
    return h if nk == 1 else mix64(h ^ _u64(k2))


def table_cap_for(groups):
    cap = 1024
    while cap < 2 * groups:
        cap *= 2
    return cap


def table_rule(cap, nk):
    arena = cap + 65536 if nk == 2 else 0
    nsh_log2 = 8 if cap >= 1 << 18 else 0
    nsh = 1 << nsh_log2
    limit = min(cap - cap // 4, 0xFFFFFFF0)
    arena_cap = min(arena, 0xFFFFFFF0)
    return {"limit": limit, "nshards": nsh, "limit_shard": limit if nsh == 1 else limit // nsh + limit // nsh // 16,
            "arena_cap": arena_cap, "arena_shard_limit": arena_cap // nsh}


def gb_levels(hint):
    return 2 if hint > 256 * 1024 else 1


def l0_bits(levels, hint):
    return 7 if levels == 1 and hint <= 150000 else 8


def digit(nk, k1, k2, bits):
    return ((owner_hash(nk, k1, k2) >> np.uint64(64 - bits)) & np.uint64(255)).astype(np.int64)


# ----------------------------------------------------------------------------- the model: the launch
def blocks_per_cu(lb, bd, priv, tuned, agg_blocks):
    b = max(1, min(4 if bd == 512 else 8, LDS_MAX // lb)) if lb else 4
    if tuned:
        b = min(b, TUNED_BLOCKS)
    if not priv and agg_blocks:
        b = min(b, agg_blocks)
    return b


def layout(nkeys, naggs, hint, key=(0, 0), segment=0, slots=0, table_cap=0, num_cus=256, agg_blocks=0, expr=0, n=0):
    """The model's nut_groupby_layout: the same fields, from the functions above."""
    k1, k2 = int(key[0]) & M64, (int(key[1]) & M64 if nkeys == 2 else 0)
    cap = lds_cap(nkeys, naggs, hint, slots or (2 if segment else 4))
    P = priv_groups(cap, nkeys, naggs, hint, bool(segment))
    w = int(lkey(nkeys, k1, k2)[0])
    tcap = table_cap or table_cap_for(hint or 8192)
    h = int(key_hash(nkeys, k1, k2)[0])
    home = int(slot_of(h, tcap)[0])
    r = table_rule(tcap, nkeys)
    priv, tuned = P > 0, P > 0 and bool(expr)
    bd = BD_SHARED if not priv else BD_TUNED if tuned else BD_PRIV
    bpc = blocks_per_cu(lds_bytes(cap, nkeys, naggs, priv, P, bd), bd, priv, tuned, agg_blocks)
    pairs = (n + 1) // 2
    lv = gb_levels(hint)
    return {"lds_cap": cap, "lds_limit": lds_limit(cap), "priv": P, "lds_home": int(lhome(w, cap)[0]) if cap else 0,
            "lds_bucket": BUCKET, "direct_idx": int(direct_idx(nkeys, k1, k2)[0]), "direct_size": DIRECT, "lds_word": w,
            "table_cap": tcap, "hash": h, "home": home, "tag": h >> 32, "claim_shard": home & (r["nshards"] - 1),
            "arena_shard": (h >> 32) & (r["nshards"] - 1), "limit": r["limit"], "nshards": r["nshards"],
            "limit_shard": r["limit_shard"], "arena_shard_limit": r["arena_shard_limit"], "arena_cap": r["arena_cap"],
            "threads": bd, "blocks_per_cu": bpc, "blocks": max(1, min(num_cus * bpc, (pairs + bd - 1) // bd)),
            "levels": lv, "l0_bits": l0_bits(lv, hint), "l0_digit": int(digit(nkeys, k1, k2, l0_bits(lv, hint))[0]),
            "owner_hash": int(owner_hash(nkeys, k1, k2)[0])}


def library_layout(nkeys, naggs, hint, key=(0, 0), segment=0, slots=0, table_cap=0, num_cus=256, agg_blocks=0, expr=0,
                   n=0):
    """nut_groupby_layout (host only) as a dict with layout()'s fields."""
    import ctypes as C

    from nutdb_amd._lib import NutGroupbyLayoutInfo, NutGroupbyLayoutQuery, lib
    q = NutGroupbyLayoutQuery(nkeys=nkeys, naggs=naggs, group_hint=hint, segment=segment, slots_per_group=slots,
                              table_cap=table_cap, num_cus=num_cus, agg_blocks=agg_blocks, expr_kernel=expr, n=n)
    q.key[0], q.key[1] = int(key[0]), int(key[1])
    o = NutGroupbyLayoutInfo()
    st = lib.nut_groupby_layout(C.byref(q), C.byref(o))
    assert st == 0, st
    return {f: getattr(o, f) for f, _ in NutGroupbyLayoutInfo._fields_}


def lane_steps(n, blocks, threads):
    """What every lane of a streaming launch of n rows does (agg_kernel's row loop): (full
    steps of two pairs, pairs of its guarded last step) per lane, as two int64 arrays."""
    g = blocks * threads
    q0 = np.arange(g, dtype=np.int64)
    full, npairs = n // 2, (n + 1) // 2
    # the loop runs steps while q + g < full, advancing q by 2 g
    steps = np.where(q0 + g < full, (full - q0 - g + 2 * g - 1) // (2 * g), 0)
    q = q0 + 2 * g * steps
    tail = np.where(q < npairs, np.where(q + g < npairs, 2, 1), 0)
    return steps, tail


def loop_rows(blocks, threads, r=1000):
    """A row count at which lanes < r run four full steps and no last step, lane r three and
    a last step of two pairs (the second one the odd row), every other lane three and a last
    step of one pair: 2 (7 g + r) + 1 rows, g = blocks x threads lanes."""
    g = blocks * threads
    assert 0 < r < g
    return 2 * (7 * g + r) + 1


# ----------------------------------------------------------------------------- inverses
def lds_word_at(home, cap, salt, hi=0):
    """64-bit words whose home bucket starts at slot `home` of a `cap`-slot table, with high
    half `hi`: the 32-bit product's top bits are home + (salt mod 4), its low bits salt div 4;
    the odd multiplier is inverted mod 2^32 and the xor-fold undone with `hi`."""
    l2 = _log2(cap)
    home, salt, hi = np.broadcast_arrays(_u64(home), _u64(salt), _u64(hi))
    assert np.all(home % np.uint64(BUCKET) == 0) and np.all(home < np.uint64(cap))
    assert np.all((salt >> np.uint64(2)) < np.uint64(1 << (32 - l2))) and np.all(hi < np.uint64(1 << 32))
    p = ((home + (salt & np.uint64(3))) << np.uint64(32 - l2)) | (salt >> np.uint64(2))
    f = (p * np.uint64(FIB32_INV)) & np.uint64(0xFFFFFFFF)
    return (hi << np.uint64(32)) | (f ^ hi)


def lds_key_at(home, cap, salt, hi=0):
    """int64 keys of a single-key table (the key is its slot word)."""
    return _i64(lds_word_at(home, cap, salt, hi))


def tuple_with_word(h, k2):
    """k1 with the un-nudged lkey<2> hash of (k1, k2) equal to h: the xorshift by 29 is undone
    by x ^ x >> 29 ^ x >> 58, the multiplies by their inverses."""
    h = _u64(h)
    h = h ^ (h >> np.uint64(29)) ^ (h >> np.uint64(58))
    return _i64(_mul(h ^ _mul(_add(k2, LK_ADD), LK_MUL), GOLDEN_INV))


def gkey_at(slot, cap, salt):
    """Global hashes (single key: the keys) with home slot `slot` of a `cap`-slot table."""
    shift = 64 - _log2(cap)
    slot, salt = np.broadcast_arrays(_u64(slot), _u64(salt))
    assert np.all(slot < np.uint64(cap)) and np.all(salt < np.uint64(1 << shift))
    return _mul((slot << np.uint64(shift)) | salt, GOLDEN_INV)


def tuple_with_hash(h, k2):
    """k1 with key_hash<2>(k1, k2) = h."""
    return _i64(unmix64(h) ^ mix64(_add(k2, GOLDEN)))


def key_with_owner_hash(h):
    return _i64(unmix64(h) ^ np.uint64(OWNER_C))


def tuple_with_owner_hash(h, k1):
    return _i64(unmix64(h) ^ mix64(_u64(k1) ^ np.uint64(OWNER_C)))


def _distinct(*cols):
    t = np.stack([np.asarray(c, dtype=np.int64) for c in cols], axis=1)
    return len(np.unique(t, axis=0)) == len(t)


def _case(name, keys, hint, note):
    keys = tuple(np.ascontiguousarray(k, dtype=np.int64) for k in keys)
    assert _distinct(*keys), name
    for k in keys:
        k.setflags(write=False)
    return Case(name, len(keys), keys, hint, note)


case_of = _case


# ----------------------------------------------------------------------------- rows of a case
ORDERS = ("round_robin", "blocked")
TAIL_ROWS = (1, 2, 3, 4, 5, 4099)       # tail-only sizes: every lane at most one guarded step (4099: odd)


def key_index(K, n, order):
    """Which of the K tuples row i carries.  round_robin: i mod K — every wave meets every new
    key at once (claim contention).  blocked: runs of 128 rows (one wave's lanes at a step:
    same-address fold atomics), shorter where n would not reach every key."""
    i = np.arange(n, dtype=np.int64)
    if order == "round_robin":
        return i % K
    run = max(1, min(128, n // K))
    return (i // run) % K


def dyadic(n, seed):
    """f64 multiples of 2^-10 below 2^20 with some -0.0: sums of up to 2^32 rows are exact in
    any order (52 bits), so every comparison is bit for bit."""
    rng = np.random.default_rng([seed, n])
    v = rng.integers(-(1 << 30) + 1, 1 << 30, n).astype(np.float64) / 1024.0
    v[rng.random(n) < 0.02] = -0.0
    return v


def wrapping(n, seed):
    """int64 values over the whole range: the sums wrap."""
    return np.random.default_rng([seed, n, 1]).integers(I64_MIN, I64_MAX, n, dtype=np.int64)


def rows(case, n, order, seed=0):
    """(key columns, f64 value column) of n rows over the case's tuples."""
    idx = key_index(len(case.keys[0]), n, order)
    return [np.ascontiguousarray(k[idx]) for k in case.keys], dyadic(n, seed + len(case.keys[0]))


# ----------------------------------------------------------------------------- cases: single-key on-chip table
HIS = (0, 0x9E3C1A57)                    # the high-word variants of A1-A4 (the second: a negative key)
MID = lambda cap: (cap // 2) & ~3        # noqa: E731  a bucket in the middle of the table


@lru_cache(maxsize=None)
def a1_bucket(cap, hi=0):
    h = MID(cap)
    return _case("A1", [lds_key_at(h, cap, [0, 1, 2, 3], hi)], None,
                 f"4 keys homed at bucket {h} of {cap}: the bucket holds them, a hit at each j")


@lru_cache(maxsize=None)
def a2_chain(cap, hi=0, at=None):
    h = MID(cap) if at is None else at
    return _case("A2" if at is None else "A3", [lds_key_at(h, cap, 4 + np.arange(12), hi)], None,
                 f"12 keys homed at bucket {h} of {cap}: one chain over slots {h}..{(h + 11) % cap}")


def a3_wrap(cap, hi=0):
    return a2_chain(cap, hi, cap - 4)


@lru_cache(maxsize=None)
def a4_behind(cap, hi=0):
    h = MID(cap)
    k = np.concatenate([lds_key_at(h, cap, 16 + np.arange(5), hi), lds_key_at(h + 4, cap, 32 + np.arange(4), hi)])
    return _case("A4", [k], None, f"5 keys homed at bucket {h}, 4 at bucket {h + 4}: slots {h}..{h + 8}, the key at "
                                  f"{h + 8} behind two full buckets")


@lru_cache(maxsize=None)
def a5_count(K):
    k = np.unique(np.random.default_rng(K).integers(I64_MIN + 1, I64_MAX, 2 * K, dtype=np.int64))
    return _case("A5", [np.random.default_rng(K + 1).permutation(k)[:K]], 9, f"{K} distinct keys, hint 9")


@lru_cache(maxsize=None)
def a6_extremes(cap):
    k = np.concatenate([a2_chain(cap).keys[0], np.array([I64_MIN, I64_MAX, -1, 0], dtype=np.int64)])
    return _case("A6", [k], None, "A2's chain and INT64_MIN (the special slot), INT64_MAX, -1, 0")


@lru_cache(maxsize=None)
def a7_swapped_halves():
    rng = np.random.default_rng(7)
    a, b = rng.integers(1, 1 << 32, 6, dtype=np.uint64), rng.integers(1, 1 << 32, 6, dtype=np.uint64)
    k = np.concatenate([(a << np.uint64(32)) | b, (b << np.uint64(32)) | a])
    return _case("A7", [_i64(k)], None, "6 pairs (a << 32 | b, b << 32 | a): equal fold, equal home, different keys")


def no_lds_hint(nk, na):
    """The smallest hint for which a launch has no on-chip table (above 8 x the largest)."""
    big = lds_cap(nk, na, 4096)
    assert big and lds_cap(nk, na, 8 * big) == big and lds_cap(nk, na, 8 * big + 1) == 0
    return 8 * big + 1


@lru_cache(maxsize=None)
def a8_no_table(na):
    k = np.unique(np.random.default_rng(8).integers(I64_MIN, I64_MAX, 300, dtype=np.int64))[:257]
    k[0] = I64_MIN
    return _case("A8", [k], no_lds_hint(1, na), "257 keys (INT64_MIN among them), no on-chip table: every row through g_row")


# ----------------------------------------------------------------------------- cases: two-key on-chip table
def _tuples(words, k2):
    words, k2 = np.broadcast_arrays(_u64(words), _u64(k2))
    assert not np.any(words == np.uint64(EMPTY))
    return tuple_with_word(words, k2), _i64(k2)


@lru_cache(maxsize=None)
def b1_same_word(cap, m, across):
    h = MID(cap)
    w = lds_word_at(h, cap, 41, 0x1234ABCD)
    k1, k2 = _tuples(np.repeat(w, m), 100 + np.arange(m))
    if across:  # four more tuples of the bucket, each with a word of its own
        f1, f2 = _tuples(lds_word_at(h, cap, 48 + np.arange(4), 0x0BADF00D), 7)
        k1, k2 = np.concatenate([k1, f1]), np.concatenate([k2, f2])
    return _case("B1", [k1, k2], None, f"{m} tuples with one slot word homed at bucket {h} of {cap}" +
                 (", and four more tuples of that bucket: a chain across it" if across else ""))


@lru_cache(maxsize=None)
def b2_nudged():
    k2 = np.array([5, -9, 11, 12], dtype=np.int64)
    pre = np.array([EMPTY, EMPTY ^ 1, EMPTY ^ 2, EMPTY ^ 3], dtype=np.uint64)
    return _case("B2", [tuple_with_word(pre, k2), k2], None,
                 "tuples hashing to the empty marker (nudged to marker ^ 1), to marker ^ 1 itself, to marker ^ 2 and ^ 3")


@lru_cache(maxsize=None)
def b3_count(K):
    rng = np.random.default_rng(300 + K)
    k1 = rng.integers(I64_MIN, I64_MAX, K, dtype=np.int64)
    return _case("B3", [k1, np.arange(K, dtype=np.int64) % 7 - 3], 9, f"{K} tuples, hint 9")


@lru_cache(maxsize=None)
def b4_chain(cap, wrap):
    h = cap - 4 if wrap else MID(cap)
    k1, k2 = _tuples(lds_word_at(h, cap, 64 + np.arange(12), 0x00C0FFEE), np.arange(12) % 3)
    return _case("B4", [k1, k2], None, f"12 tuples with distinct words homed at bucket {h} of {cap}")


# ----------------------------------------------------------------------------- cases: private accumulators
@lru_cache(maxsize=None)
def c1_direct_edge():
    return _case("C1", [np.array([255, 256, -1, 0, 7], dtype=np.int64)], 8,
                 "keys 255 (last direct-map entry), 256 and -1 (outside), 0, 7")


@lru_cache(maxsize=None)
def c2_direct_edge():
    t = np.array([(15, 15), (16, 0), (0, 16), (-1, 0), (0, 0), (3, 4)], dtype=np.int64)
    return _case("C2", [t[:, 0], t[:, 1]], 8, "tuples (15,15) (last entry), (16,0), (0,16), (-1,0) (outside), (0,0), (3,4)")


@lru_cache(maxsize=None)
def c3_ids_run_out():
    return _case("C3", [np.array([0, 1, 2, 3, 4, 300], dtype=np.int64)], 3,
                 "6 groups, hint 3: three private ids, the other groups fold in the table")


@lru_cache(maxsize=None)
def c4_cutoff():
    return _case("C4", [np.array([0, 1, 2, 3, 4, 5, 6, 255], dtype=np.int64)], 8, "8 groups, hint 8")


# ----------------------------------------------------------------------------- cases: global table
D1_HINT, D1_CAP, D1_SLOT = 100, 1024, 1020


@lru_cache(maxsize=None)
def d1_long_run():
    k = _i64(gkey_at(D1_SLOT, D1_CAP, 1 + np.arange(100)))
    return _case("D1", [k], D1_HINT, "100 keys homed at slot 1020 of 1024: one run over 1020..1023, 0..95")


@lru_cache(maxsize=None)
def d2_regrow(K):
    k = np.unique(np.random.default_rng(K).integers(I64_MIN + 1, I64_MAX, 2 * K, dtype=np.int64))
    return _case("D2", [np.random.default_rng(K + 1).permutation(k)[:K]], 1, f"{K} distinct keys, hint 1 (1024 slots, limit 768)")


SHARD_HINT, SHARD_CAP = 131072, 1 << 18   # the largest hint whose first table has 2^18 slots (sharded counters)
D3_SHARD = 77


@lru_cache(maxsize=None)
def d3_claim_shard(K):
    per = SHARD_CAP // 256
    assert K <= per
    slots = D3_SHARD + 256 * ((np.arange(K) * 5) % per)     # distinct slots, spread over the table
    return _case("D3", [_i64(gkey_at(slots, SHARD_CAP, 12345 + np.arange(K)))], SHARD_HINT,
                 f"{K} keys with distinct home slots in claim shard {D3_SHARD} of a 2^18-slot table")


@lru_cache(maxsize=None)
def d4_same_hash(m):
    h = np.uint64(0xC0DEC0DE12345678)
    k2 = 1000 + np.arange(m, dtype=np.int64)
    extra = np.array([7, 8, 9], dtype=np.int64)
    return _case("D4", [np.concatenate([tuple_with_hash(np.repeat(h, m), k2), extra]), np.concatenate([k2, extra])], 16,
                 f"{m} tuples with one 64-bit hash (one slot, one tag), and three others")


@lru_cache(maxsize=None)
def d5_tag_and_slot(cap):
    shift = 64 - _log2(cap)
    # same tag, different slot: hashes differing in the low half only
    h1 = np.array([0xABCD123400000001, 0xABCD123477777777], dtype=np.uint64)
    # same slot, different tag: hash x golden with equal top bits
    h2 = gkey_at(513 % cap, cap, [(1 << (shift - 1)) + 5, 99])
    h = np.concatenate([h1, h2])
    k2 = np.array([1, 2, 3, 4], dtype=np.int64)
    return _case("D5", [tuple_with_hash(h, k2), k2], 16, "two tuples with one tag and two slots; two with one slot and two tags")


D6_SHARD = 200


@lru_cache(maxsize=None)
def d6_arena_shard(K):
    rng = np.random.default_rng(6)
    h = rng.integers(0, 1 << 64, K, dtype=np.uint64)
    h = (h & np.uint64(~(0xFF << 32) & M64)) | np.uint64(D6_SHARD << 32)
    return _case("D6", [tuple_with_hash(h, np.arange(K)), np.arange(K, dtype=np.int64)], SHARD_HINT,
                 f"{K} tuples with tags in arena shard {D6_SHARD} of a 2^18-slot table")


# ----------------------------------------------------------------------------- cases: compaction, partition
@lru_cache(maxsize=None)
def e1_special_chunk(cap):
    k = np.unique(np.random.default_rng(cap).integers(I64_MIN + 1, I64_MAX, 400, dtype=np.int64))[:300]
    k[0] = I64_MIN
    return _case("E1", [k], cap // 2, f"INT64_MIN and 299 keys in a {cap}-slot table: slot {cap} opens a compaction chunk")


@lru_cache(maxsize=None)
def e2_owners(nk, P, spread):
    """spread: one group per part (P groups); else 40 groups all owned by part P - 1."""
    n = P if spread else 40
    part = np.arange(n) if spread else np.full(n, P - 1)
    h = _u64(np.random.default_rng([nk, P]).integers(0, (1 << 63) // P, n)) * np.uint64(P) + _u64(part)
    if nk == 1:
        keys = [key_with_owner_hash(h)]
    else:
        k1 = np.arange(n, dtype=np.int64) * 3 - 5
        keys = [k1, tuple_with_owner_hash(h, k1)]
    return _case("E2", keys, 64, f"{n} groups, " + ("one per part" if spread else f"all owned by part {P - 1}") + f" of {P}")


# ----------------------------------------------------------------------------- cases: segment mode
SEG_HINT, SEG_BITS = 256, 8          # with gb_l0_bits = 8: 256 level-0 partitions, each a workgroup of its own


def seg_limit():
    """Groups a partition's block table admits in segment mode at SEG_HINT over 256 partitions."""
    per = max(64, 2 * ((SEG_HINT + 255) // 256))
    return lds_limit(lds_cap(1, 4, per, 2))


@lru_cache(maxsize=None)
def g_partition(K, d=93):
    """K keys with level-0 digit d and one key with every other digit (so that all 256
    partitions exist and each takes one workgroup)."""
    shift = 64 - SEG_BITS
    big = key_with_owner_hash((np.uint64(d) << np.uint64(shift)) | _u64(1 + np.arange(K)))
    others = np.array([x for x in range(256) if x != d], dtype=np.uint64)
    one = key_with_owner_hash((others << np.uint64(shift)) | np.uint64(12345))
    return _case("G", [np.concatenate([big, one])], SEG_HINT, f"{K} groups in level-0 partition {d}, one in each other")
