"""Directed inputs for the hash join (csrc/join.hip) and a host model of its table layout
(numpy only; no GPU).

The model restates csrc/hj_layout.hpp: the capacity is the power of two >= 2 x build rows
(>= 64); a key's home slot is the top log2(capacity) bits of mix64(key ^ HJ_SALT); a run
is probed linearly and wraps inside aligned blocks of `block` slots — the whole table, or
one 8192-slot region of a region-built table.  mix64 is a bijection, so `key_at` computes
a key for any chosen home slot: the low bits of the hash (the salt) are free, and many
distinct keys share a home.  tests/test_join_shapes_cpu.py pins `home` to the library's
own arithmetic (nut_join_layout) and proves with `occupied` that every builder below
holds the runs, wraps and region counts it claims.  The model never produces an expected
join result: the reference is always the numpy oracle (oracle.join_i64).

What the model can and cannot say about a racing build: the SET of occupied slots under
linear probing does not depend on the insertion order, so `occupied` is exact for the
CAS builds, and so is every walk length of an ABSENT key.  WHICH key of a run sits in
which slot depends on who wins a slot, except where only one outcome exists; `lockstep`
models the one case the tests need it for (32 build rows: one wave, whose lanes take
their rounds together) and refuses inputs whose placement would depend on a tie.

The builders return (build, probe, note)."""
from functools import lru_cache

import numpy as np

from helpers import _u64, mix64, unmix64  # noqa: F401  (shared with groupby_shapes.py)

I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
HJ_SALT = 0x3C6EF372FE94F82A          # home hash = mix64(key ^ HJ_SALT)
RS = 8192                             # slots of a region (HJ_RS)
RLIMIT = RS * 7 // 8                  # records a region-built region may hold (HJ_RLIMIT)
TILES = (1024, 2048, 4096, 8192)      # probe tile sizes (hj_cfg, hj_any_cfg, hj_match_cfg, hj_emit_cfg)


def capacity_of(nbuild):
    log2c = 6
    while (1 << log2c) < 2 * nbuild:
        log2c += 1
    return 1 << log2c


def _log2(capacity):
    log2c = int(capacity).bit_length() - 1
    assert 1 << log2c == capacity and log2c >= 6
    return log2c


def home(keys, capacity):
    k = np.atleast_1d(np.asarray(keys, dtype=np.int64)).view(np.uint64)
    return (mix64(k ^ np.uint64(HJ_SALT)) >> np.uint64(64 - _log2(capacity))).astype(np.int64)


def key_at(slot, capacity, salt):
    """int64 keys whose home is `slot`; `salt` (< capacity's free hash bits) picks among the
    2^(64 - log2 capacity) keys of that home.  slot and salt broadcast."""
    shift = 64 - _log2(capacity)
    slot, salt = np.broadcast_arrays(_u64(slot), _u64(salt))
    assert np.all(slot < np.uint64(capacity)) and np.all(salt < np.uint64(1 << shift))
    h = (slot << np.uint64(shift)) | salt
    return (unmix64(h) ^ np.uint64(HJ_SALT)).view(np.int64)


def occupied(keys, capacity, block):
    """The occupied slots (a sorted int64 array) after inserting `keys` by linear probing
    from their homes with wrap inside aligned blocks of `block` slots, in ANY order.
    Going round a block, the number of keys carried past slot s follows
    c[s+1] = max(0, c[s] + n[s] - 1) (n: keys homed at s), and s is occupied iff
    c[s] + n[s] > 0.  Two laps: a block that is not full has an empty slot, after which
    the first lap's carry is the stationary one."""
    n = np.bincount(home(keys, capacity), minlength=capacity).astype(np.int64).reshape(-1, block)
    assert np.all(n.sum(axis=1) < block), "a block without an empty slot"
    x = np.concatenate([n, n], axis=1) - 1
    s = np.cumsum(x, axis=1) - x                     # S[s] = sum of x before s
    c = s - np.minimum.accumulate(np.minimum(s, 0), axis=1)
    occ = (c[:, block:] + n) > 0
    return np.flatnonzero(occ.reshape(-1))


def next_slot(s, block):
    return (s & ~(block - 1)) | ((s + 1) & (block - 1))


def walk_length(key, occ, capacity, block):
    """Slots an absent key's probe reads before its empty slot (the occupied ones)."""
    occ = occ if isinstance(occ, (set, frozenset)) else set(occ.tolist())
    s, n = int(home(key, capacity)[0]), 0
    while s in occ:
        s, n = next_slot(s, block), n + 1
    return n


def lockstep(keys, capacity):
    """Slot of each build row when the rows take their probing rounds together (the lanes of
    one wave of hj_build_kernel: every row tries its slot, an empty slot goes to one of the
    rows trying it, everyone else steps on).  Only equal keys may meet at an empty slot —
    their placement is symmetric; a tie between different keys raises."""
    keys = np.asarray(keys, dtype=np.int64)
    assert len(keys) <= 64
    at = home(keys, capacity).tolist()
    table, left = {}, list(range(len(keys)))
    while left:
        want = {}
        for i in left:
            if at[i] not in table:
                want.setdefault(at[i], []).append(i)
        for s, rows in want.items():
            if len({int(keys[i]) for i in rows}) != 1:
                raise ValueError(f"slot {s}: a tie between different keys")
            table[s] = rows[0]
        won = {r for r in table.values()}
        left = [i for i in left if i not in won]
        for i in left:
            at[i] = next_slot(at[i], capacity)
    return np.array(at, dtype=np.int64)


# ----------------------------------------------------------------------------- 64-slot tables
def _absent(slot, capacity, n=1, salt0=1 << 20):
    return key_at(slot, capacity, salt0 + np.arange(n))


@lru_cache(maxsize=None)
def table_end_run():
    """Six distinct keys homed at slots 62 and 63 of a 64-slot table: one run over 62, 63,
    0, 1, 2, 3.  Probes: every build key; absent keys homed at 62, 63 and 0 (walks of 6, 5
    and 4 slots) and at the first empty slot, 4 (no walk)."""
    build = np.concatenate([key_at(62, 64, [1, 2, 3]), key_at(63, 64, [1, 2, 3])])
    probe = np.concatenate([build, _absent(62, 64), _absent(63, 64), _absent(0, 64), _absent(4, 64)])
    return build, probe, "run 62,63,0..3"


DUP_VARIANTS = ("adjacent", "same_home", "staggered", "wrapped")
DUP_HOME = {"adjacent": 10, "same_home": 10, "staggered": 10, "wrapped": 63}


@lru_cache(maxsize=None)
def one_duplicate(variant):
    """32 build rows on 64 slots: 31 distinct keys and ONE repeat, K (the last two rows).
      adjacent   K, K homed at 10, alone: slots 10, 11.
      same_home  K, K and four foreign keys, all homed at 10: the run 10..15 holds the twins
                 and the four; who sits where is the build's race (13 of the 15 placements
                 put a foreign key before or between the twins).
      staggered  K, K homed at 10, four foreign keys homed at 11, 12, 13, 14: in one wave the
                 foreign keys take their homes in the first round, so the second K walks past
                 all four: twins at 10 and 15 (lockstep).
      wrapped    K, K homed at 63, alone: slots 63 and 0.
    The other keys sit alone, no slot next to them taken.  Probes: every build row's key
    (K twice) and absent keys homed at K's home, inside and one past its run."""
    h = DUP_HOME[variant]
    k = key_at(h, 64, 7)
    if variant == "adjacent":
        near, alone = [], list(range(13, 62, 2)) + [0, 2, 4, 6, 8]
    elif variant == "same_home":
        near, alone = key_at(10, 64, [1, 2, 3, 4]).tolist(), list(range(17, 62, 2)) + [0, 2, 4]
    elif variant == "staggered":
        near, alone = key_at([11, 12, 13, 14], 64, 1).tolist(), list(range(17, 62, 2)) + [0, 2, 4]
    else:
        near, alone = [], list(range(2, 62, 2))
    rest = np.concatenate([np.array(near, dtype=np.int64), key_at(alone, 64, 3)])
    build = np.concatenate([rest, k, k])
    assert len(build) == 32
    run = {"adjacent": 2, "same_home": 6, "staggered": 6, "wrapped": 2}[variant]
    probe = np.concatenate([build, _absent(h, 64), _absent((h + run - 1) % 64, 64), _absent((h + run) % 64, 64)])
    return build, probe, f"one duplicate, {variant}"


@lru_cache(maxsize=None)
def half_table_run(dup=False):
    """32 keys all homed at slot 40 of a 64-slot table: one run over 40..63, 0..7 (half the
    table, across its end).  dup: the last key repeats the one before (31 distinct + one
    repeat, one run: a twin has its home slot to itself in 2 of 32 outcomes only).  Probes:
    every key, and absent keys homed at the run's first, middle and last slot (walks of
    32, 16 and 1 slots)."""
    build = key_at(40, 64, 1 + np.arange(32))
    if dup:
        build[31] = build[30]
    probe = np.concatenate([build, _absent(40, 64), _absent(56, 64), _absent(7, 64)])
    return build, probe, "32 keys homed at 40" + (", one repeat" if dup else "")


TINY = [(nb, np_) for nb in (1, 2, 3, 5) for np_ in (1, 65)]


@lru_cache(maxsize=None)
def tiny(nb, np_):
    """nb in {1, 2, 3, 5} random build keys; probe rows alternate build keys and absent ones."""
    rng = np.random.default_rng([nb, np_])
    build = rng.integers(I64_MIN, I64_MAX, nb, dtype=np.int64)
    probe = np.where(np.arange(np_) % 3 == 1, rng.integers(I64_MIN, I64_MAX, np_, dtype=np.int64),
                     build[np.arange(np_) % nb])
    return build, probe, f"{nb} x {np_}"


# ----------------------------------------------------------------------------- region-built tables
REGION_NB = (1 << 20) + 1             # the smallest build side with regions: 2^22 slots, 512 regions
REGION_CAP = 1 << 22
NREG = REGION_CAP // RS
END_REGIONS = (0, 255, NREG - 1)      # regions whose end holds a directed run
DUP_REGION, FULL_REGION, RUN_REGION = 100, 300, 400
RUN_SLOT = 5000
# the filler keeps out of the directed regions and their successors, so a directed run is
# the only thing in its neighbourhood under either wrap rule
RESERVED = sorted({r % NREG for q in END_REGIONS + (DUP_REGION, FULL_REGION, RUN_REGION) for r in (q, q + 1)})


@lru_cache(maxsize=None)
def region_filler():
    """REGION_NB unique random keys homed outside the RESERVED regions."""
    rng = np.random.default_rng(2 ** 20)
    k = np.unique(rng.integers(I64_MIN, I64_MAX, REGION_NB + (REGION_NB >> 4), dtype=np.int64))
    k = k[~np.isin(home(k, REGION_CAP) // RS, RESERVED)]
    k = rng.permutation(k)[:REGION_NB]
    assert len(k) == REGION_NB
    k.setflags(write=False)
    return k


def _region_build(directed, seed):
    directed = np.asarray(directed, dtype=np.int64)
    b = np.concatenate([region_filler()[:REGION_NB - len(directed)], directed])
    return np.random.default_rng(seed).permutation(b)


def _rslot(region, slot):
    return region * RS + slot


@lru_cache(maxsize=None)
def region_end_runs():
    """Unique keys.  In each region R of END_REGIONS, eight distinct keys homed at R's slots
    8190 and 8191 (four each): region-built, the run covers R's slots 8190, 8191, 0..5;
    built table-wide it covers 8190, 8191 and slots 0..5 of region R + 1 (for the last
    region: of region 0, across the table's end).  Probes: the 24 keys; per R, absent keys
    homed at R's last slot, at R's first slot (the wrapped part of the run, region-built)
    and at region R + 1's first slot (the same part, table-wide); 2000 filler keys and
    2000 random (absent) keys."""
    rng = np.random.default_rng(81)
    d = np.concatenate([key_at(_rslot(r, s), REGION_CAP, 1 + np.arange(4)) for r in END_REGIONS for s in (8190, 8191)])
    a = np.unique(np.concatenate([_absent(_rslot(q, s), REGION_CAP) for r in END_REGIONS
                                  for q, s in ((r, 8191), (r, 0), ((r + 1) % NREG, 0))]))
    build = _region_build(d, 1)
    probe = rng.permutation(np.concatenate([d, a, rng.choice(region_filler(), 2000),
                                            rng.integers(I64_MIN, I64_MAX, 2000, dtype=np.int64)]))
    return build, probe, "runs across the ends of regions 0, 255, 511"


REGION_DUP_VARIANTS = ("adjacent", "wrapped")


@lru_cache(maxsize=None)
def region_duplicate(variant):
    """Unique filler and ONE repeated key K in region DUP_REGION (otherwise empty): adjacent
    = homed at slot 4000 (slots 4000, 4001); wrapped = homed at slot 8191 (slots 8191 and,
    region-built, the region's slot 0; table-wide, the next region's slot 0).  Probes: K,
    absent keys at its home and behind its run under both wrap rules, 2000 filler keys,
    2000 random keys."""
    rng = np.random.default_rng(82)
    s = 4000 if variant == "adjacent" else 8191
    k = key_at(_rslot(DUP_REGION, s), REGION_CAP, 7)
    a = np.concatenate([_absent(_rslot(DUP_REGION, s), REGION_CAP), _absent(_rslot(DUP_REGION, (s + 1) % RS), REGION_CAP),
                        _absent(_rslot(DUP_REGION + 1, 0), REGION_CAP)])
    build = _region_build(np.concatenate([k, k]), 2)
    probe = rng.permutation(np.concatenate([k, a, rng.choice(region_filler(), 2000),
                                            rng.integers(I64_MIN, I64_MAX, 2000, dtype=np.int64)]))
    return build, probe, f"one duplicate in region {DUP_REGION}, {variant}"


@lru_cache(maxsize=None)
def region_full(extra=0):
    """Region FULL_REGION holds exactly RLIMIT + extra distinct keys, homes spread over the
    region (slot (8 i) div 7: seven taken, one free); every other region holds fewer.
    extra = 0 is the fullest region the LDS build takes, with all HJ_RK = 7 records of
    every lane live; extra = 1 sends the whole table to the global CAS build.  Probes:
    all of the region's keys and 1000 absent keys homed in it."""
    rng = np.random.default_rng(83)
    i = np.arange(RLIMIT)
    d = key_at(_rslot(FULL_REGION, (8 * i) // 7), REGION_CAP, 1 + i)
    if extra:
        d = np.concatenate([d, key_at(_rslot(FULL_REGION, 8 * np.arange(extra) + 7), REGION_CAP, 5)])
    a = key_at(_rslot(FULL_REGION, rng.integers(0, RS, 1000)), REGION_CAP, (1 << 20) + np.arange(1000))
    build = _region_build(d, 3)
    return build, rng.permutation(np.concatenate([d, a])), f"{len(d)} keys in region {FULL_REGION}"


RUN_PRESENT, RUN_ABSENT = 64, 64


@lru_cache(maxsize=None)
def region_long_run():
    """RLIMIT distinct keys all homed at slot RUN_SLOT of region RUN_REGION: one run of 7168
    slots — region-built it wraps inside the region (5000..8191, 0..3975), table-wide it
    runs on into the next (empty) region.  Probes: 64 of the keys and 64 absent keys homed
    at the run's start, each of which walks all 7168 slots."""
    rng = np.random.default_rng(84)
    d = key_at(_rslot(RUN_REGION, RUN_SLOT), REGION_CAP, 1 + np.arange(RLIMIT))
    a = _absent(_rslot(RUN_REGION, RUN_SLOT), REGION_CAP, RUN_ABSENT)
    build = _region_build(d, 4)
    return build, rng.permutation(np.concatenate([rng.choice(d, RUN_PRESENT, replace=False), a])), "a 7168-slot run"


# ----------------------------------------------------------------------------- tile edges
TILE_NPROBE = sorted({1, 63, 64, 65} | {n for t in TILES for n in (t - 1, t, t + 1, 2 * t + 1)})
EDGE_STEP = 512                       # divides every probe tile (the smallest unordered one is 512)
BIG_NPROBE = 65 * 8192 + 1            # 66 write-out tiles: the look-back takes a second 64-tile step


@lru_cache(maxsize=None)
def tile_build(repeated):
    """25 build rows: repeated = five keys three times each and ten single keys; else 25
    distinct keys.  (keys3, keys1, build)."""
    rng = np.random.default_rng(85)
    k = rng.integers(I64_MIN, I64_MAX, 25, dtype=np.int64)
    assert len(np.unique(k)) == 25
    if not repeated:
        return k[:0], k, k
    return k[:5], k[5:15], rng.permutation(np.concatenate([np.repeat(k[:5], 3), k[5:15]]))


@lru_cache(maxsize=None)
def tile_edges(nprobe, repeated):
    """nprobe probe rows that match 0, 1 or (repeated) 3 build rows at random, except that
    rows i with i mod 512 in {511, 0}, i >= 511 — the last lane of every tile of 1024,
    2048, 4096 or 8192 rows and the first lane of the next — match 3 (unique build keys: 1),
    and the rows next to them (i mod 512 in {510, 1}) match none."""
    k3, k1, build = tile_build(repeated)
    rng = np.random.default_rng([nprobe, int(repeated)])
    pool = np.concatenate([k3, k1, rng.integers(I64_MIN, I64_MAX, 10, dtype=np.int64)])
    probe = pool[rng.integers(0, len(pool), nprobe)]
    i = np.arange(nprobe)
    edge = (i >= EDGE_STEP - 1) & np.isin(i % EDGE_STEP, (EDGE_STEP - 1, 0))
    beside = (i >= EDGE_STEP - 2) & np.isin(i % EDGE_STEP, (EDGE_STEP - 2, 1))
    top = k3 if repeated else k1
    probe[edge] = top[i[edge] % len(top)]
    probe[beside] = pool[-1 - (i[beside] % 10)]
    return build, probe, f"{nprobe} probe rows, {'repeated' if repeated else 'unique'} build keys"


@lru_cache(maxsize=None)
def big_probe():
    """BIG_NPROBE probe rows over 25 unique build keys, two rows in three matching."""
    _, k1, build = tile_build(False)
    rng = np.random.default_rng(86)
    pool = np.concatenate([k1, k1, rng.integers(I64_MIN, I64_MAX, 25, dtype=np.int64)])
    return build, pool[rng.integers(0, len(pool), BIG_NPROBE)], f"{BIG_NPROBE} probe rows"
