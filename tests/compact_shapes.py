"""Directed inputs for the order-preserving compaction kernels (csrc/filter.hip,
csrc/select_kernel.hpp) and the decoupled look-back they share with the join
(csrc/lookback.hpp), and a host model of their tile geometry (numpy only; no GPU).

The model restates the three geometries:
  staged filter    tile 32768 rows = 16 stripes x 2048; thread t of 1024 holds rows 2t and
                   2t + 1 of each stripe, so a wave covers 128 consecutive rows of a
                   stripe; the LDS buffer holds FS_CAP = 20224 rows and `half` is the
                   selected count of the tile's first 16384 rows (stripes 0..7);
  unstaged filter  tile 16384 rows = 16 stripes x 1024; 512 threads, 8 waves;
  select           tile 16384 rows; item i of 32 of thread t of 512 is row
                   base + 512 i + t; 8 waves.
tests/test_compact_shapes_cpu.py pins the constants to the sources and proves, from the
mask alone, that every builder holds the totals, halves, per-(stripe, wave) and
per-(item, wave) counts and parities its GPU test (tests/test_gpu_compact_paths.py) relies
on.

Column values make every misplaced, duplicated or dropped row visible: under the
predicate `>= 0` a selected row r holds r and any other row holds -r - 1 (`column`;
`column_op` derives the other five operators' columns and constants from the same mask).

The model never produces an expected output: the reference is always col[mask] /
np.flatnonzero(mask) (and oracle.filter_i64).  `staged_model`, `select_model` and
`lookback_walk` restate what the kernels do with a tile, a pair of count buffers and a
chain of granules; the CPU test holds them to that reference on the named cases, which is
what shows that a wrong threshold, clamp, buffer flip, lane mask or walk step would make a
named case differ.

Builders return (column, note)."""
from functools import lru_cache

import numpy as np

WAVE = 64
FS_THREADS, FS_WAVES, FS_STRIPES, FS_STRIPE_ROWS, FS_TILE = 1024, 16, 16, 2048, 32768
FS_HALF, FS_CAP = 16384, 20224
FT_THREADS, FT_WAVES, FT_STRIPES, FT_STRIPE_ROWS, FT_TILE = 512, 8, 16, 1024, 16384
SEL_THREADS, SEL_WAVES, SEL_ITEMS, SEL_TILE = 512, 8, 32, 16384
FLAG_AGG, FLAG_INC, VAL_MASK = 1 << 62, 2 << 62, (1 << 62) - 1
SENTINEL = -0x0123456789ABCDEF
OPS = ("<", "<=", ">", ">=", "==", "!=")

# kind -> (tile rows, stripes, waves); a wave holds 128 consecutive rows of a stripe
PAIR = {"staged": (FS_TILE, FS_STRIPES, FS_WAVES), "unstaged": (FT_TILE, FT_STRIPES, FT_WAVES)}


# ----------------------------------------------------------------------------- geometry
def pair_row(kind, stripe, wave, lane, which):
    """In-tile row of lane `lane` of wave `wave` in stripe `stripe` (which: 0 = .x, 1 = .y)."""
    tile, stripes, waves = PAIR[kind]
    return stripe * (tile // stripes) + 2 * WAVE * wave + 2 * lane + which


def sel_row(item, wave, lane):
    return SEL_THREADS * item + WAVE * wave + lane


def _tiles(mask, tile):
    mask = np.asarray(mask, dtype=bool)
    pad = -len(mask) % tile
    return np.concatenate([mask, np.zeros(pad, dtype=bool)]).reshape(-1, tile)


def pair_counts(mask, kind):
    """[tile, stripe, wave] selected rows: what the kernel's s_cnt holds for each tile."""
    tile, stripes, waves = PAIR[kind]
    return _tiles(mask, tile).reshape(-1, stripes, waves, 2 * WAVE).sum(axis=-1)


def sel_counts(mask):
    """[tile, item, wave] selected rows: select_kernel's s_cnt for each tile."""
    return _tiles(mask, SEL_TILE).reshape(-1, SEL_ITEMS, SEL_WAVES, WAVE).sum(axis=-1)


def totals(mask, tile):
    return _tiles(mask, tile).sum(axis=1)


def halves(mask):
    """The staged kernel's `half`: selected rows of each tile's stripes 0..7."""
    return _tiles(mask, FS_TILE)[:, :FS_HALF].sum(axis=1)


def max_rank(mask, kind):
    """The largest in-wave rank any selected row's lane holds (the packed rank's range)."""
    tile, stripes, waves = PAIR[kind]
    m = _tiles(mask, tile).reshape(-1, WAVE, 2)
    lanes = m.sum(axis=-1)
    before = np.cumsum(lanes, axis=1) - lanes
    return int(before[m.any(axis=-1)].max(initial=0))


# ----------------------------------------------------------------------------- columns
def column(mask, row0=0):
    """`>= 0` selects exactly `mask`: row r holds r where selected, -r - 1 elsewhere."""
    r = row0 + np.arange(len(mask), dtype=np.int64)
    return np.where(mask, r, -r - 1)


def mask_of(col):
    return np.asarray(col) >= 0


def column_op(mask, op):
    """(column, k) with `column <op> k` == mask, rows told apart wherever the operator
    allows it (== can only give the selected rows one value)."""
    r = np.arange(len(mask), dtype=np.int64)
    if op in (">=", ">"):
        return np.where(mask, r, -r - 1), 0 if op == ">=" else -1
    if op in ("<", "<="):
        return np.where(mask, -r - 1, r), 0 if op == "<" else -1
    if op == "==":
        return np.where(mask, 42, r + 43), 42
    assert op == "!="
    return np.where(mask, r, -1), -1


def apply_op(col, op, k):
    return {"<": col < k, "<=": col <= k, ">": col > k, ">=": col >= k, "==": col == k, "!=": col != k}[op]


# ----------------------------------------------------------------------------- one tile's selection
def _scramble(size):
    """A bijection of [0, size) (size a power of two) that spreads a prefix over the tile."""
    return (np.arange(size) * 5923 + 7) % size


def t_total(kind, total):
    """Exactly `total` rows of a tile, spread evenly over it."""
    return _scramble(PAIR[kind][0]) < total


def t_dense(half, rest):
    """Staged tile with `half` rows in stripes 0..7 and `rest` in stripes 8..15."""
    s = _scramble(FS_HALF)
    return np.concatenate([s < half, s < rest])


def t_wave(kind, stripe, wave):
    """All 128 rows of one wave of one stripe: lane 63's pair has in-wave rank 126."""
    m = np.zeros(PAIR[kind][0], dtype=bool)
    lo = pair_row(kind, stripe, wave, 0, 0)
    m[lo:lo + 2 * WAVE] = True
    return m


def t_stripe(kind, stripe):
    tile, stripes, _ = PAIR[kind]
    m = np.zeros(tile, dtype=bool)
    m[stripe * (tile // stripes):(stripe + 1) * (tile // stripes)] = True
    return m


def t_lane(kind, lane):
    """Both rows of lane `lane` of every wave of every stripe."""
    return (np.arange(PAIR[kind][0]) % (2 * WAVE)) // 2 == lane


def t_parity(kind, which):
    return np.arange(PAIR[kind][0]) % 2 == which


STAGED_TOTALS = (0, 1, 2, 3, 20223, 20224, 20225, 32767, 32768)
STAGED_DENSE = ((3841, 16384), (16384, 3841), (16383, 3842), (10113, 10113), (10114, 10114))
PLACEMENTS = ["wave:5:3", "wave:0:0", "wave:15:7", "stripe:0", "stripe:7", "stripe:8", "stripe:15",
              "lane:0", "lane:63", "parity:0", "parity:1"]
STAGED_SHAPES = [f"total:{t}" for t in STAGED_TOTALS] + [f"dense:{h}:{r}" for h, r in STAGED_DENSE] + \
    PLACEMENTS + ["wave:5:9", "wave:15:15"]
UNSTAGED_SHAPES = [f"total:{t}" for t in (0, 1, 2, 3, 16383, 16384)] + PLACEMENTS


def tile_shape(kind, name):
    what, *a = name.split(":")
    a = [int(x) for x in a]
    if what == "total":
        return t_total(kind, *a)
    if what == "dense":
        assert kind == "staged"
        return t_dense(*a)
    return {"wave": t_wave, "stripe": t_stripe, "lane": t_lane, "parity": t_parity}[what](kind, *a)


# ----------------------------------------------------------------------------- (a) one shaped tile
@lru_cache(maxsize=None)
def one_tile(kind, name):
    """n = one tile, shaped `name`."""
    col = column(tile_shape(kind, name))
    col.setflags(write=False)
    return col, f"{kind} tile {name}"


PREV_ODD, PREV_EVEN, NEXT_TOTAL = 12345, 12346, 7777


@lru_cache(maxsize=None)
def three_tiles(kind, name, prev_odd):
    """Three tiles, the shaped one in the middle; the tile before it holds an odd
    (PREV_ODD) or an even (PREV_EVEN) count, so the shaped tile's output offset has that
    parity; the tile behind it shows whether the shaped tile's count was passed on."""
    prev = t_total(kind, min(PREV_ODD if prev_odd else PREV_EVEN, PAIR[kind][0]))
    col = column(np.concatenate([prev, tile_shape(kind, name), t_total(kind, NEXT_TOTAL)]))
    col.setflags(write=False)
    return col, f"{kind} tile {name} behind {'an odd' if prev_odd else 'an even'} count"


# ----------------------------------------------------------------------------- (b) last-tile edges
STAGED_EDGE_N = (2, 3, 32769, 32770, 32771, 65535, 32768 + 2047, 32768 + 2048, 32768 + 2049)


def last_rows(n, bits):
    """n rows alternating (even rows selected), the last three rows n - 3, n - 2, n - 1
    selected by bits 2, 1, 0 of `bits` (n = 2: bits 1, 0)."""
    m = np.arange(n) % 2 == 0
    for b in range(min(3, n)):
        m[n - 1 - b] = bool((bits >> b) & 1)
    return column(m), f"n = {n}, last rows {bits:03b}"


# ----------------------------------------------------------------------------- (c) persistence
PERSIST_PATTERN = (0, 1, 20224, 20225, 32768)   # tile t holds PERSIST_PATTERN[t % 5] rows
PERSIST_RAGGED = 12345                          # rows of the ragged last tile


def staged_persistent(ntiles, ragged):
    """ntiles staged tiles, tile t shaped total:PERSIST_PATTERN[t % 5]; ragged: the last
    tile is cut to PERSIST_RAGGED rows.  5 and any power-of-two CU count are coprime, so
    whichever tiles a workgroup takes in turn, the pattern moves on: its tiles switch
    between the `fits` path and the two-halves path."""
    shapes = np.stack([t_total("staged", t) for t in PERSIST_PATTERN])
    m = shapes[np.arange(ntiles) % len(PERSIST_PATTERN)].reshape(-1)
    if ragged:
        m = m[:(ntiles - 1) * FS_TILE + PERSIST_RAGGED]
    return column(m), f"{ntiles} staged tiles{', the last ragged' if ragged else ''}"


# ----------------------------------------------------------------------------- (d) unstaged sizes, (e) select
UNSTAGED_N = (1, 2, 3, 16383, 16384, 16385, 65 * 16384 + 1, 130 * 16384 + 3)
SELECT_N = (16383, 16384, 16385)
SELECT_CORNERS = ((0, 0), (0, 7), (31, 0), (31, 7))
STEP = 7919   # prime; coprime to 16385 = 5 x 29 x 113


def varied(n, tile=FT_TILE):
    """n rows in tiles of 16384; full tile t holds exactly (t * STEP + 1) mod 16385 rows,
    spread over the tile — pairwise different counts for the first 16385 tiles, so any two
    tiles a persistent workgroup takes in turn differ in their total and their counts."""
    t = np.arange(-(-n // tile))
    want = (t * STEP + 1) % (tile + 1)
    m = (_scramble(tile)[None, :] < want[:, None]).reshape(-1)[:n]
    return column(m), f"n = {n}, every tile a different count"


def select_item_wave(n, item, wave):
    """Selected rows only in item `item` of wave `wave` of every tile (all 64 lanes)."""
    r = np.arange(n) % SEL_TILE
    m = (r // SEL_THREADS == item) & ((r % SEL_THREADS) // WAVE == wave)
    return column(m), f"n = {n}, item {item} of wave {wave}"


def select_const(n, value):
    return column(np.full(n, bool(value))), f"n = {n}, {'all' if value else 'no'} rows"


def select_alternating(ntiles, extra=5):
    n = ntiles * SEL_TILE + extra
    return column((np.arange(n) // SEL_TILE) % 2 == 0), f"{ntiles} tiles alternating all and none, + {extra} rows"


# ----------------------------------------------------------------------------- (f) look-back chains
LB_RUNS = (0, 1, 62, 63, 64, 65, 127, 128, 129, 200)
BIG = (1 << 61) + 12345   # a value no true sum below may include


def lookback_reference(status, tile, total):
    """(exclusive prefix, granule published): the sum of the values from tile - 1 down to
    and including the most recent inclusive granule, or down to index 0."""
    excl = 0
    for i in range(tile - 1, -1, -1):
        excl += int(status[i]) & VAL_MASK
        if int(status[i]) >> 62 == 2:
            break
    assert excl + total <= VAL_MASK
    return excl, FLAG_INC | (excl + total)


def chain(run, behind=5, seed=0, value=None):
    """(status, tile, total): `run` aggregate-flagged predecessors, before them one
    inclusive granule, before that `behind` older granules with values of 2^61 under both
    flags that must not be counted.  tile = behind + 1 + run."""
    rng = np.random.default_rng([run, behind, seed])
    tile = behind + 1 + run
    vals = rng.integers(0, 1 << 40, tile + 3, dtype=np.uint64) if value is None else \
        np.full(tile + 3, value, dtype=np.uint64)
    st = vals | np.uint64(FLAG_AGG)
    st[behind] = vals[behind] | np.uint64(FLAG_INC)
    st[:behind] = np.uint64(BIG) | np.where(np.arange(behind) % 2 == 0, np.uint64(FLAG_INC), np.uint64(FLAG_AGG))
    st[tile:] = 0    # this tile and its successors: not published yet
    return st, tile, int(rng.integers(0, 1 << 40))


def chain_no_inclusive(tile, value=None):
    """tile aggregate-flagged predecessors and no inclusive one: the walk runs off index 0."""
    rng = np.random.default_rng(tile)
    vals = rng.integers(0, 1 << 40, tile + 1, dtype=np.uint64) if value is None else \
        np.full(tile + 1, value, dtype=np.uint64)
    st = vals | np.uint64(FLAG_AGG)
    st[tile] = 0
    return st, tile, 17


def chain_one_huge(tile, at):
    """One predecessor of 2^62 - 1, the rest 0, no inclusive granule; total 0."""
    st = np.full(tile + 1, FLAG_AGG, dtype=np.uint64)
    st[at] = np.uint64(FLAG_AGG | VAL_MASK)
    st[tile] = 0
    return st, tile, 0


# ----------------------------------------------------------------------------- what the kernels do
def lookback_walk(status, tile, total, lane_mask=True, second_step=True):
    """lookback_publish + lookback_resolve as one wave runs them: 64 predecessors a step,
    lane l reads status[pred - l] (an index below 0 reads as inclusive 0); the step that
    sees an inclusive granule counts the lanes up to the first one and ends the walk."""
    if tile == 0:
        return 0, FLAG_INC | total
    excl, pred = 0, tile - 1
    while True:
        idx = pred - np.arange(WAVE)
        s = [int(status[i]) if i >= 0 else FLAG_INC for i in idx]
        inc = [x >> 62 == 2 for x in s]
        if any(inc):
            first = inc.index(True)
            excl += sum(x & VAL_MASK for l, x in enumerate(s) if l <= first or not lane_mask)
            break
        excl += sum(x & VAL_MASK for x in s)
        if not second_step:
            break
        pred -= WAVE
    excl &= (1 << 64) - 1
    return excl, (FLAG_INC | ((excl + total) & VAL_MASK))


def _flush(out, at, cnt, buf, word0):
    """flush_staged: out[at .. at + cnt) = buf[0 .. cnt) as aligned pairs with a scalar head
    and tail; word0 = the output's address in 8-byte words."""
    head = (word0 + at) & 1
    if head and cnt:
        out[at] = buf[0]
    i = np.arange(head, max(cnt - 1, head), 2)
    out[at + i] = buf[i]
    out[at + i + 1] = buf[i + 1]
    if cnt > head and (cnt - head) & 1:
        out[at + cnt - 1] = buf[cnt - 1]


def staged_model(col, word0=0, fits_cap=FS_CAP, upper_half=True):
    """filter_i64_staged_kernel under `>= 0`, tile by tile: 16-byte loads at pair indices
    clamped to n - 2, the pair holding row n - 1 of an odd n taking its row from the upper
    half, staging into a buffer of FS_CAP rows (whole if total <= fits_cap, else in two
    halves) and flush_staged.  Returns (guarded output, count): a buffer of n + 2 words of
    SENTINEL with the output at word 0."""
    col = np.asarray(col, dtype=np.int64)
    n = len(col)
    out = np.full(n + 2, SENTINEL, dtype=np.int64)
    excl = 0
    for base in range(0, n, FS_TILE):
        idx = base + 2 * np.arange(FS_TILE // 2)
        at = np.minimum(idx, n - 2)
        x, y = col[at].copy(), col[at + 1]
        if base + FS_TILE > n and (n - 1 - base) % 2 == 0 and upper_half:
            p = (n - 1 - base) // 2
            x[p] = y[p]
        p0, p1 = (x >= 0) & (idx < n), (y >= 0) & (idx + 1 < n)
        rows = np.stack([x, y], axis=1).reshape(-1)
        keep = np.stack([p0, p1], axis=1).reshape(-1)
        half, total = int(keep[:FS_HALF].sum()), int(keep.sum())
        buf = np.full(FS_TILE + 2, SENTINEL + 1, dtype=np.int64)   # behind FS_CAP: not the buffer

        def stage(lo, hi):
            v = rows[lo:hi][keep[lo:hi]]
            v = v[:FS_CAP]          # a store behind the buffer does not land in it
            buf[:len(v)] = v
        if total <= fits_cap:
            stage(0, FS_TILE)
            _flush(out, excl, total, buf, word0)
        else:
            stage(0, FS_HALF)
            _flush(out, excl, half, buf, word0)
            stage(FS_HALF, FS_TILE)
            _flush(out, excl + half, total - half, buf, word0)
        excl += total
    return out, excl


def select_model(mask, grid, flip=True):
    """select_kernel's persistent loop with `grid` workgroups, workgroup g taking tiles g,
    g + grid, ...: the counts of the tile being written out are read from s_cnt[b] while
    the next tile's are evaluated into s_cnt[b ^ 1].  The look-back is taken as exact on
    what each tile published.  Returns (row ids, count)."""
    mask = np.asarray(mask, dtype=bool)
    n = len(mask)
    cnt = sel_counts(mask)
    bits = _tiles(mask, SEL_TILE).reshape(-1, SEL_ITEMS, SEL_WAVES, WAVE)
    ntiles = len(cnt)
    used = [None] * ntiles
    for g in range(min(grid, ntiles)):
        mine = list(range(g, ntiles, grid))
        s_cnt, b = [cnt[mine[0]], None], 0
        for j, t in enumerate(mine):
            if j + 1 < len(mine):
                s_cnt[b ^ 1] = cnt[mine[j + 1]]
            used[t] = s_cnt[b]
            if flip:
                b ^= 1
    out = np.full(n + SEL_TILE, SENTINEL, dtype=np.int64)
    excl = 0
    for t in range(ntiles):
        u = used[t]
        all_ = u.sum(axis=1)
        off = excl + np.cumsum(all_) - all_
        before = np.cumsum(u, axis=1) - u
        rank = np.cumsum(bits[t], axis=2) - bits[t]
        pos = (off[:, None, None] + before[:, :, None] + rank)[bits[t]]
        ids = (t * SEL_TILE + sel_row(*np.meshgrid(np.arange(SEL_ITEMS), np.arange(SEL_WAVES), np.arange(WAVE),
                                                   indexing="ij")))[bits[t]]
        ok = pos < len(out)
        out[pos[ok]] = ids[ok]
        excl += int(all_.sum())
    return out[:min(excl, len(out))], excl
