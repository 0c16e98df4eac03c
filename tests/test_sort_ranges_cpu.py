"""CPU: properties of the sample sort's skew-safe ranges as restated in nutdb_amd/dist.py
(sort_ranges, split_counts).  tests/test_gpu_dist_ranks.py pins the C++ of csrc/dist.cpp to
this restatement at 9 to 64 ranks, so the restatement gets its own pinning here: for every
world size and sample shape, the partition splitters are strictly ascending and at most 63
(what the range partition accepts), every bucket maps to a valid, ordered rank range with a
positive total weight, split_counts moves every key exactly once, and the rank a key lands
on never decreases with the key (so the ranks' outputs concatenate in order)."""
import numpy as np
import pytest

from nutdb_amd.dist import sort_ranges, split_counts

I64_MAX = np.iinfo(np.int64).max
I64_MIN = np.iinfo(np.int64).min
WORLDS = [2, 3, 8, 9, 32, 33, 63, 64]
M = 20_000  # pool size: > 64 quantiles with room for several heavy keys


def _heavy(rng, keys_and_shares):
    pool = rng.integers(I64_MIN, I64_MAX, M, dtype=np.int64, endpoint=True)
    u = rng.random(M)
    at = 0.0
    for k, share in keys_and_shares:
        pool[(u >= at) & (u < at + share)] = k
        at += share
    return pool


POOLS = {
    "uniform": lambda rng: rng.integers(I64_MIN, I64_MAX, M, dtype=np.int64, endpoint=True),
    "small_range": lambda rng: rng.integers(0, 200, M, dtype=np.int64),
    "tiny_range": lambda rng: rng.integers(-3, 4, M, dtype=np.int64),
    "one_heavy": lambda rng: _heavy(rng, [(-77, 0.5)]),
    "one_heavy_max": lambda rng: _heavy(rng, [(I64_MAX, 0.5)]),
    "one_heavy_min": lambda rng: _heavy(rng, [(I64_MIN, 0.5)]),
    "two_heavy_adjacent": lambda rng: _heavy(rng, [(100, 0.3), (101, 0.3)]),
    "two_heavy_extremes": lambda rng: _heavy(rng, [(I64_MIN, 0.3), (I64_MAX, 0.3)]),
    "two_heavy_adjacent_at_max": lambda rng: _heavy(rng, [(I64_MAX - 1, 0.3), (I64_MAX, 0.3)]),
    "three_heavy": lambda rng: _heavy(rng, [(I64_MIN, 0.2), (7, 0.25), (8, 0.2)]),
    "three_heavy_apart": lambda rng: _heavy(rng, [(-5, 0.2), (0, 0.2), (I64_MAX, 0.3)]),
    "all_equal": lambda rng: np.full(M, 42, dtype=np.int64),
    "all_equal_max": lambda rng: np.full(M, I64_MAX, dtype=np.int64),
    "small_pool": lambda rng: rng.integers(-10, 10, 5, dtype=np.int64),  # fewer samples than ranks
}


def _ranges(world, kind):
    rng = np.random.default_rng(1000 * world + sorted(POOLS).index(kind))
    pool = np.sort(POOLS[kind](rng))
    m = len(pool)
    spl = [int(pool[(i * m) // world]) for i in range(1, world)]
    return pool, spl, sort_ranges(spl, pool, world)


@pytest.mark.parametrize("kind", sorted(POOLS))
@pytest.mark.parametrize("world", WORLDS)
def test_ranges_are_valid(world, kind):
    pool, spl, (e, lo, hi, w) = _ranges(world, kind)
    assert e.dtype == np.int64
    assert len(e) <= 63                      # partition_i64_ranges' bound
    assert np.all(e[1:] > e[:-1])            # strictly ascending
    nb = len(e) + 1
    assert len(lo) == len(hi) == len(w) == nb
    for j in range(nb):
        assert 0 <= lo[j] <= hi[j] < world
        assert len(w[j]) == hi[j] - lo[j] + 1
        assert all(x >= 0 for x in w[j]) and sum(w[j]) > 0
    assert all(a <= b for a, b in zip(lo, lo[1:]))
    assert all(a <= b for a, b in zip(hi, hi[1:]))
    # the first bucket starts at rank 0 and the last one ends at the last rank a splitter names
    assert lo[0] == 0 and hi[-1] == world - 1
    # every splitter value is an edge: no key below a splitter shares a bucket with one above it
    assert set(spl) <= set(e.tolist())


@pytest.mark.parametrize("kind", sorted(POOLS))
@pytest.mark.parametrize("world", WORLDS)
def test_key_rank_is_monotone(world, kind):
    """Bucket j's ranks lie at or above bucket j-1's (hi[j-1] <= lo[j]): with a bucket's keys
    spread over lo[j] .. hi[j], a larger key never lands on a lower rank.  A bucket spread
    over more than one rank holds exactly one key value, so the ranks inside it hold equal keys."""
    pool, spl, (e, lo, hi, w) = _ranges(world, kind)
    assert all(h <= l2 for h, l2 in zip(hi, lo[1:]))
    for j in range(len(lo)):
        if hi[j] > lo[j]:
            assert j >= 1 and (j == len(e) or int(e[j]) == int(e[j - 1]) + 1 or int(e[j - 1]) == I64_MAX), j
            if j == len(e):  # an open last bucket may be spread only when it is {INT64_MAX}
                assert int(e[j - 1]) == I64_MAX
    # and through the keys themselves: the rank range of each pool key, by its bucket
    b = np.searchsorted(e, pool, "right")
    klo, khi = np.asarray(lo)[b], np.asarray(hi)[b]
    assert np.all(klo[1:] >= klo[:-1]) and np.all(khi[1:] >= khi[:-1])
    differ = pool[1:] != pool[:-1]
    assert np.all(khi[:-1][differ] <= klo[1:][differ])


@pytest.mark.parametrize("kind", sorted(POOLS))
@pytest.mark.parametrize("world", WORLDS)
def test_split_counts_conserves(world, kind):
    pool, spl, (e, lo, hi, w) = _ranges(world, kind)
    nb = len(e) + 1
    for c in (0, 1, 1_000_003):  # nothing, one key, a large prime
        for j in range(nb):
            counts = [0] * nb
            counts[j] = c
            out = split_counts(counts, lo, w, world)
            assert len(out) == world and sum(out) == c and min(out) >= 0
            assert all(out[r] == 0 for r in range(world) if r < lo[j] or r > hi[j])
        out = split_counts([c] * nb, lo, w, world)
        assert sum(out) == c * nb and min(out) >= 0
    # the pool's own bucket counts: every sample is sent once
    bc = np.bincount(np.searchsorted(e, pool, "right"), minlength=nb).tolist()
    assert sum(split_counts(bc, lo, w, world)) == len(pool)


@pytest.mark.parametrize("world", WORLDS)
def test_heavy_key_is_spread(world):
    """A key holding half the pool: its bucket spans the ranks whose quantiles it fills, and
    splitting the pool's own counts leaves every rank within one quantile's rounding."""
    pool, spl, (e, lo, hi, w) = _ranges(world, "one_heavy")
    j = int(np.searchsorted(e, -77, "right"))
    assert hi[j] - lo[j] >= world // 2 - 1
    bc = np.bincount(np.searchsorted(e, pool, "right"), minlength=len(e) + 1).tolist()
    out = split_counts(bc, lo, w, world)
    assert max(out) <= len(pool) // world + len(lo) + 1


def test_all_mode_threshold():
    """Distinct splitters each get a bucket of their own while that needs <= 63 partition
    splitters: P - 1 distinct, non-adjacent values give 2 (P - 1) edges up to P = 32 (62), and
    from P = 33 on (64 > 63) only repeated values do, which leaves the P - 1 values themselves."""
    for world, want in ((9, 16), (32, 62), (33, 32), (63, 62), (64, 63)):
        pool = np.arange(world * 100, dtype=np.int64) * 1000
        spl = [int(pool[(i * len(pool)) // world]) for i in range(1, world)]
        e, lo, hi, w = sort_ranges(spl, pool, world)
        assert len(e) == want, (world, len(e))
        if want == world - 1:
            assert lo == list(range(world)) and hi == lo
