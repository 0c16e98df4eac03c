"""Directed small inputs for the sort family (msd_sort.hip, sort.hip, topk.hip) and a host
model of the local sort's window rule (numpy only; no GPU, no library).

The model restates DESIGN.md §4.3 / `LocalCfg` for a single-segment sort (n <= 24576 keys:
hi = 64, base = 0): a key's bucket is the top SB bits of its order-mapped value u = key ^
flip; buckets are laid out in order; window q starts at the first bucket start >= q * WS
and the last window ends at n.  A window of 2-16 keys is sorted inside one lane, 17-32 by a
half-wave bitonic network, 33-64 / 65-128 by the wave-wide networks; one window over 128
keys sends the whole segment to ms_lsd_kernel.  The model is used ONLY to prove that an
input holds the window sizes it claims (tests/test_sort_shapes_cpu.py); it never produces
an expected result: the reference is always numpy's sort.

The builders return `Case(name, keys, desc)`: `desc` is the direction the case is built for
(the window layout of the network inputs depends on it: DESC complements u, which reverses
the bucket order), or None when both directions make the same claim."""
from collections import namedtuple

import numpy as np

I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
FLIP = {False: np.uint64(0x8000000000000000), True: np.uint64(0x7FFFFFFFFFFFFFFF)}  # RS_FLIP, RS_FLIP_DESC
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)

# The local-sort classes: name -> (smallest n, largest n, SB bucket bits, WS window stride).
# THIS TABLE MUST CHANGE WITH `LocalCfg` / `ls_class` (msd_sort.hip): SB = 12 above 5120
# keys of capacity, 11 above 2048, else 9; WS = 10 for capacities in (4096, 8192], else 12.
CLASSES = {"S": (1, 2048, 9, 12), "M": (2049, 5120, 11, 10), "M2": (5121, 6144, 12, 10), "L": (6145, 24576, 12, 12)}
LDS_KEYS = 16384    # keys per LDS round (LocalCfg::LDS_KEYS); the L class takes two rounds above it
MAX_WINDOW = 128    # LS_MAX_WINDOW: the largest network
LANE_N = 16         # LS_LANE_N: windows up to this size are sorted inside one lane
LS_CAP = 24576      # the largest single-segment sort

Case = namedtuple("Case", "name keys desc")


def class_of(n):
    for name, (lo, hi, _, _) in CLASSES.items():
        if lo <= n <= hi:
            return name
    raise ValueError(f"{n} keys are not a single-segment sort")


def umap(keys, desc):
    """The order-mapped keys of nut_sort_i64 / nut_sort_i64_desc."""
    return np.ascontiguousarray(keys, dtype=np.int64).view(np.uint64) ^ FLIP[bool(desc)]


# ----------------------------------------------------------------------------- the model
def window_starts(keys, desc):
    """s_win[0 .. nq] of ms_local_kernel for a single-segment sort of `keys`."""
    n = len(keys)
    _, _, sb, ws = CLASSES[class_of(n)]
    counts = np.bincount((umap(keys, desc) >> np.uint64(64 - sb)).astype(np.int64), minlength=1 << sb)
    ends = np.cumsum(counts[counts > 0])           # the bucket boundaries after position 0
    nq = (n + ws - 1) // ws
    win = np.empty(nq + 1, dtype=np.int64)
    win[0] = 0
    q = np.arange(1, nq)
    win[1:nq] = ends[np.searchsorted(ends, q * ws, side="left")]  # first bucket start >= q * WS
    win[nq] = n
    return win


def window_sizes(keys, desc):
    d = np.diff(window_starts(keys, desc))
    return d[d > 0]


def round_split(keys, desc):
    """(mid, n - mid): round 0 sorts [0, mid) in LDS, round 1 the rest (n > LDS_KEYS only)."""
    n = len(keys)
    win = window_starts(keys, desc)
    if n <= LDS_KEYS:
        return n, 0
    mid = int(win[:-1][win[:-1] <= LDS_KEYS].max())  # the last window that starts inside round 0
    return mid, n - mid


def takes_fallback(keys, desc):
    """True when ms_local_kernel lists the segment for ms_lsd_kernel."""
    return int(window_sizes(keys, desc).max()) > MAX_WINDOW or round_split(keys, desc)[1] > LDS_KEYS


# ----------------------------------------------------------------------------- single segment
def _keys_from_buckets(counts, sb, rng, variant, desc):
    """Keys whose bucket (top `sb` bits of u) sizes are `counts`, in bucket order: the used
    buckets spread over all 2^sb, the low 40 bits random, shuffled.  variant "dups": half of
    every bucket of >= 10 keys repeats one value; "extremes": u = 0 and u = all ones (the
    padding value) occur: INT64_MIN / INT64_MAX ascending, INT64_MAX / INT64_MIN descending."""
    nb = len(counts)
    if variant == "extremes":
        ids = np.concatenate([[0], np.sort(rng.choice(np.arange(1, (1 << sb) - 1), nb - 2, replace=False)),
                              [(1 << sb) - 1]])
    else:
        ids = np.sort(rng.choice(1 << sb, nb, replace=False))
    parts = []
    for b, c in zip(ids, counts):
        low = rng.integers(0, 1 << 40, c, dtype=np.int64).astype(np.uint64)
        if variant == "dups" and c >= 10:
            low[c // 2:] = low[0]
        parts.append((np.uint64(int(b)) << np.uint64(64 - sb)) | low)
    if variant == "extremes":
        parts[0][0] = np.uint64(0)
        parts[-1][-min(3, len(parts[-1])):] = ONES
    u = np.concatenate(parts)
    rng.shuffle(u)
    return (u ^ FLIP[bool(desc)]).view(np.int64)


def network_layouts(cls):
    """Bucket-size lists, one per input, that hold every window size 1..128 in class `cls`
    with no window over 128.  Per w in WS..128: one filler bucket of exactly WS keys (a
    window of WS keys), one bucket of w keys starting at a multiple of WS (a window of
    exactly w keys), then WS - (w mod WS) singleton buckets (a window of that many keys,
    which brings the position back to a multiple of WS).  The groups are packed into as few
    inputs as the class's key and bucket counts allow, and an input too small for its class
    is filled up with filler buckets."""
    lo, hi, sb, ws = CLASSES[cls]
    layouts, cur = [], []
    for w in range(ws, MAX_WINDOW + 1):
        group = [ws, w] + [1] * ((-w) % ws)
        if sum(cur) + sum(group) > hi or len(cur) + len(group) > (1 << sb):
            layouts.append(cur)
            cur = []
        cur += group
    layouts.append(cur)
    for lay in layouts:
        while sum(lay) < lo:
            lay.append(ws)
        assert sum(lay) <= hi and len(lay) <= (1 << sb)
    return layouts


NETWORK_VARIANTS = ("plain", "dups", "extremes")


def network_inputs(cls, variant="plain"):
    _, _, sb, _ = CLASSES[cls]
    out = []
    for i, lay in enumerate(network_layouts(cls)):
        for desc in (False, True):
            # the same u for both directions: the window layout is a property of u
            rng = np.random.default_rng([ord(cls[0]), len(cls), i, NETWORK_VARIANTS.index(variant)])
            out.append(Case(f"net-{cls}-{i}-{variant}-{'desc' if desc else 'asc'}",
                            _keys_from_buckets(lay, sb, rng, variant, desc), desc))
    return out


def two_round_inputs():
    """L class above LDS_KEYS keys: the segment is sorted in two LDS rounds split at a window
    start.  (name, keys, desc) with both directions built from the same u."""
    sb = CLASSES["L"][2]
    lays = {
        # 8-key buckets: windows of 16 and 8 keys; bucket 2048 starts at 16384 = the first
        # bucket start >= 1365 * 12, so round 0 holds exactly LDS_KEYS keys
        "boundary16384": [8] * 3048,
        # a 100-key bucket at 16320 = 1360 * 12: one 100-key window over [16320, 16420)
        "straddle100": [8] * 2040 + [100] + [8] * 900,
    }
    out = []
    for name, lay in lays.items():
        for desc in (False, True):
            rng = np.random.default_rng([7, len(lay)])
            out.append(Case(f"two-{name}-{'desc' if desc else 'asc'}", _keys_from_buckets(lay, sb, rng, "plain", desc), desc))
    rng = np.random.default_rng(16385)
    for n in (16385, 24576):
        out.append(Case(f"two-uniform-{n}", rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True), None))
    return out


FALLBACK_SIZES = {"S": (1000, 2047, 2048), "M": (2049, 5120), "M2": (5121, 6144), "L": (6145, 16385, 24576)}
FALLBACK_KINDS = ("const", "two", "win129", "maxrun", "minrun")


def fallback_inputs(cls):
    """Single-segment inputs with a window over 128 keys (in both directions): they go to
    ms_lsd_kernel<THREADS, MAXK> of their class.  Sizes at the class edges and, per class,
    one that is no multiple of the thread count, so that the LSD padding is in play."""
    sb = CLASSES[cls][2]
    out = []
    for n in FALLBACK_SIZES[cls]:
        rng = np.random.default_rng([n, 129])
        full = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
        out.append(Case(f"fb-{cls}-{n}-const", np.full(n, -7, dtype=np.int64), None))
        out.append(Case(f"fb-{cls}-{n}-two", rng.choice(np.array([-7, (1 << 33) + 3], dtype=np.int64), n), None))
        v = full.copy()  # 129 keys of one bucket (distinct low bits) in otherwise sparse data
        v[rng.choice(n, 129, replace=False)] = ((np.uint64(5) << np.uint64(64 - sb))
                                                | rng.integers(0, 1 << 40, 129, dtype=np.int64).astype(np.uint64)).view(np.int64)
        out.append(Case(f"fb-{cls}-{n}-win129", v, None))
        for kind, run, other in (("maxrun", I64_MAX, I64_MIN), ("minrun", I64_MIN, I64_MAX)):
            v = full.copy()  # the run's u is all ones (= the padding) in one direction, 0 in the other
            idx = rng.choice(n, 130, replace=False)
            v[idx[:129]] = run
            v[idx[129]] = other
            out.append(Case(f"fb-{cls}-{n}-{kind}", v, None))
    return out


def tiny_inputs():
    """n = 1 and 2: one window, no fallback."""
    return [Case("tiny-1", np.array([-7], dtype=np.int64), None),
            Case("tiny-2-const", np.array([I64_MAX, I64_MAX], dtype=np.int64), None),
            Case("tiny-2-two", np.array([5, -7], dtype=np.int64), None),
            Case("tiny-2-extremes", np.array([I64_MAX, I64_MIN], dtype=np.int64), None)]


# ----------------------------------------------------------------------------- several levels
NARROW_HB = (1, 2, 3, 8, 9, 10, 11, 12, 17, 18, 20, 28)
NARROW_N = (24577, 30_000, 200_000)


def narrow_bases(hb):
    return {"zero": 0, "neg": -(1 << 61) + 12345, "min": int(I64_MIN), "max": int(I64_MAX) - (1 << hb) + 1}


def narrow_range(hb, base, n):
    """base + U[0, 2^hb): the first level rebases the digits on the minimum and takes the top
    min(9, hb) bits below bit hb; its sub-segments have hi = hb - 9 varying bits left
    (hi <= 0: equal keys, copied; hi < SB: fewer bits than bucket bits)."""
    rng = np.random.default_rng([hb, n])
    return (np.int64(base) + rng.integers(0, 1 << hb, n, dtype=np.int64)).astype(np.int64)


CLUSTER_N = 60_000
CLUSTER_W = (40, 20, 0)


def cluster(w):
    """Half the keys over the full range, half in [2^50, 2^50 + 2^w), shuffled."""
    rng = np.random.default_rng([50, w])
    v = np.concatenate([rng.integers(I64_MIN, I64_MAX, CLUSTER_N // 2, dtype=np.int64),
                        (1 << 50) + rng.integers(0, 1 << w, CLUSTER_N - CLUSTER_N // 2, dtype=np.int64)])
    rng.shuffle(v)
    return v


TILE_FULL_N = (28671, 28672, 28673, 57343, 57344, 57345, 262143, 262144, 262145)  # scatter 2 x 14336, histogram 2^18
TILE_COPY_N = (65535, 65536, 65537)                                                   # copy tile 2^16


def tile_edge_inputs():
    out = []
    for n in TILE_FULL_N:
        rng = np.random.default_rng(n)
        out.append(Case(f"tile-full-{n}", rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True), None))
    for n in TILE_COPY_N:
        rng = np.random.default_rng(n)
        out.append(Case(f"tile-const-{n}", np.full(n, I64_MIN + 3, dtype=np.int64), None))
        out.append(Case(f"tile-two-{n}", rng.choice(np.array([-7, 11], dtype=np.int64), n), None))
    return out


# ----------------------------------------------------------------------------- pairs
# which of the order-mapped key's 8 bytes vary (byte 0 = least significant): adjacent and
# non-adjacent choices, with and without byte 7, for every pass count 1..8
BYTE_SETS = {1: [(0,), (7,), (3,)],
             2: [(0, 7), (2, 5), (3, 4)],
             3: [(0, 2, 4), (1, 6, 7)],
             4: [(0, 1, 2, 3), (1, 3, 5, 7), (0, 2, 4, 6)],
             5: [(0, 1, 3, 5, 6), (2, 3, 4, 6, 7)],
             6: [(0, 1, 2, 4, 5, 7), (1, 2, 3, 4, 5, 6)],
             7: [(0, 1, 2, 4, 5, 6, 7), (0, 1, 2, 3, 4, 5, 6)],
             8: [(0, 1, 2, 3, 4, 5, 6, 7)]}
BYTE_MASK_N = 20_000


def byte_mask_ukeys(varying, n=BYTE_MASK_N):
    """Order-mapped keys whose bytes in `varying` take every value and whose other bytes are
    the constant 0x5A: nut_sort_pairs executes exactly len(varying) passes on them."""
    rng = np.random.default_rng(list(varying) + [n])
    u = np.zeros(n, dtype=np.uint64)
    for b in range(8):
        byte = rng.integers(0, 256, n).astype(np.uint64) if b in varying else np.full(n, 0x5A, dtype=np.uint64)
        u |= byte << np.uint64(8 * b)
    return u


def byte_mask_keys(varying, f64=False, n=BYTE_MASK_N):
    """int64 (or float64) keys whose ascending order key is byte_mask_ukeys(varying); DESC
    complements every byte, which keeps the same bytes varying."""
    u = byte_mask_ukeys(varying, n)
    if not f64:
        return (u ^ FLIP[False]).view(np.int64)
    b = np.where(u >> np.uint64(63) != 0, u & np.uint64(0x7FFFFFFFFFFFFFFF), ~u)  # inverse of the IEEE total-order map
    return np.ascontiguousarray(b).view(np.float64)
