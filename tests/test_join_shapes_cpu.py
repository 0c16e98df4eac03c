"""CPU proof that tests/join_shapes.py builds what it claims (no GPU): the Python hash
model equals the library's own layout arithmetic (nut_join_layout, csrc/hj_layout.hpp),
and every named builder holds the runs, wraps, region counts and walk lengths its GPU
test (tests/test_gpu_join_paths.py) relies on.  The walk lengths asserted here are derived
from the builders' construction, not measured."""
import ctypes as C

import numpy as np
import pytest

import join_shapes as S

I64_MIN, I64_MAX = S.I64_MIN, S.I64_MAX
NUT_ERR_INVALID_ARG, NUT_ERR_UNSUPPORTED = 1, 4


def layout(nbuild, key, region_built=0):
    from nutdb_amd._lib import lib
    out = [C.c_uint64() for _ in range(5)]
    st = lib.nut_join_layout(nbuild, int(key), region_built, *[C.byref(o) for o in out])
    return (st, *[o.value for o in out])


def slots(occ, lo, n, block=None):
    """Is [lo, lo + n) (wrapping inside `block`) exactly a maximal run of `occ`?"""
    occ = set(occ.tolist()) if not isinstance(occ, set) else occ
    w = (lambda s: s) if block is None else (lambda s: (lo & ~(block - 1)) | (s & (block - 1)))
    inside = all(w(lo + i) in occ for i in range(n))
    return inside and w(lo - 1) not in occ and w(lo + n) not in occ


# ----------------------------------------------------------------------------- the model
@pytest.mark.parametrize("nbuild", [1, 32, 2 ** 17, 2 ** 20 + 1])
def test_home_equals_the_library(nbuild):
    """home() against nut_join_layout for 10^4 random keys and the int64 extremes at
    capacities 64, 2^18 and 2^22 (and 64 again from a one-row build)."""
    cap = S.capacity_of(nbuild)
    assert cap == {1: 64, 32: 64, 2 ** 17: 2 ** 18, 2 ** 20 + 1: 2 ** 22}[nbuild]
    rng = np.random.default_rng(nbuild)
    keys = np.concatenate([rng.integers(I64_MIN, I64_MAX, 10_000, dtype=np.int64),
                           np.array([I64_MIN, I64_MAX, 0, -1, 1], dtype=np.int64)])
    mine = S.home(keys, cap)
    for region in ((0, 1) if cap == 2 ** 22 else (0,)):
        for k, h in zip(keys.tolist(), mine.tolist()):
            assert layout(nbuild, k, region) == (0, cap, h, S.RS if region else cap, S.RS, S.RLIMIT), (k, region)


def test_layout_capacity_rule_and_errors():
    for nb, cap in [(0, 64), (1, 64), (32, 64), (33, 128), (2 ** 20, 2 ** 21), (2 ** 20 + 1, 2 ** 22),
                    (2 ** 28, 2 ** 29), (2 ** 28 + 1, 2 ** 30), (2 ** 31 - 1, 2 ** 32)]:
        assert layout(nb, 5)[:2] == (0, cap) and S.capacity_of(nb) == cap, nb
    # regions exist for 2^22 .. 2^29 slots only
    assert layout(2 ** 20, 5, 1)[0] == NUT_ERR_INVALID_ARG
    assert layout(2 ** 20 + 1, 5, 1)[:2] == (0, 2 ** 22) and layout(2 ** 28, 5, 1)[:2] == (0, 2 ** 29)
    assert layout(2 ** 28 + 1, 5, 1)[0] == NUT_ERR_INVALID_ARG
    assert layout(2 ** 31, 5)[0] == NUT_ERR_UNSUPPORTED
    from nutdb_amd._lib import lib
    assert lib.nut_join_layout(1, 5, 0, None, None, None, None, None) == NUT_ERR_INVALID_ARG


def test_unmix64_inverts_mix64():
    rng = np.random.default_rng(64)
    x = np.concatenate([rng.integers(0, 2 ** 64, 100_000, dtype=np.uint64),
                        np.array([0, 1, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)])
    assert np.array_equal(S.unmix64(S.mix64(x)), x) and np.array_equal(S.mix64(S.unmix64(x)), x)


@pytest.mark.parametrize("cap", [64, 2 ** 18, 2 ** 22])
def test_key_at_lands_on_its_slot(cap):
    rng = np.random.default_rng(cap)
    slot = np.concatenate([[0, cap - 1], rng.integers(0, cap, 1000)])
    k = S.key_at(slot, cap, np.arange(len(slot)))
    assert np.array_equal(S.home(k, cap), slot) and len(np.unique(k)) == len(k)
    same = S.key_at(cap - 1, cap, np.arange(1000))
    assert np.all(S.home(same, cap) == cap - 1) and len(np.unique(same)) == 1000


def test_occupied_equals_sequential_insertion():
    """occupied() against inserting one key at a time, in two different orders, with wrap
    inside the table and inside 16-slot blocks."""
    rng = np.random.default_rng(3)
    for block in (64, 16):
        for trial in range(20):
            keys = np.concatenate([S.key_at(rng.integers(0, 64), 64, 1 + np.arange(rng.integers(1, 7)))
                                   for _ in range(rng.integers(1, 6))])
            keys = keys[:12]  # a 16-slot block stays below 16 keys
            want = None
            for order in (keys, keys[::-1]):
                occ = set()
                for h in S.home(order, 64).tolist():
                    while h in occ:
                        h = S.next_slot(h, block)
                    occ.add(h)
                assert want is None or occ == want
                want = occ
            assert set(S.occupied(keys, 64, block).tolist()) == want, (block, trial)


# ----------------------------------------------------------------------------- 64-slot tables
def test_table_end_run():
    build, probe, _ = S.table_end_run()
    occ = S.occupied(build, 64, 64)
    assert occ.tolist() == [0, 1, 2, 3, 62, 63] and len(np.unique(build)) == 6
    assert sorted(S.home(build, 64).tolist()) == [62, 62, 62, 63, 63, 63]
    absent = probe[len(build):]
    assert not np.isin(absent, build).any()
    # walks: from 62 all six slots, from 63 five, from 0 four, from the empty slot 4 none
    assert S.home(absent, 64).tolist() == [62, 63, 0, 4]
    assert [S.walk_length(k, occ, 64, 64) for k in absent] == [6, 5, 4, 0]


@pytest.mark.parametrize("variant", S.DUP_VARIANTS)
def test_one_duplicate(variant):
    build, probe, _ = S.one_duplicate(variant)
    keys, counts = np.unique(build, return_counts=True)
    assert len(build) == 32 and len(keys) == 31 and sorted(counts.tolist()) == [1] * 30 + [2]
    k = keys[counts == 2][0]
    h = S.DUP_HOME[variant]
    assert S.home(k, 64)[0] == h
    occ = S.occupied(build, 64, 64)
    run = {"adjacent": 2, "same_home": 6, "staggered": 6, "wrapped": 2}[variant]
    assert slots(occ, h, run, 64), occ   # K's run, wrapping for "wrapped" (63, 0), nothing beside it
    inrun = build[np.isin(S.home(build, 64), [(h + i) % 64 for i in range(run)])]
    assert len(inrun) == run and int((inrun == k).sum()) == 2  # the run holds the twins + run - 2 foreign keys
    if variant == "same_home":
        assert np.all(S.home(inrun, 64) == h)
        with pytest.raises(ValueError):  # different keys race for slot 10: no single placement
            S.lockstep(build, 64)
    else:
        at = S.lockstep(build, 64)
        assert sorted(at.tolist()) == occ.tolist()
        twins = sorted(at[build == k].tolist())
        assert twins == {"adjacent": [10, 11], "staggered": [10, 15], "wrapped": [0, 63]}[variant]
        if variant == "staggered":  # the four foreign keys lie between the twins
            assert sorted(at[np.isin(S.home(build, 64), [11, 12, 13, 14])].tolist()) == [11, 12, 13, 14]
    # every other key sits alone
    for s in S.home(build[~np.isin(S.home(build, 64), [(h + i) % 64 for i in range(run)])], 64).tolist():
        assert slots(occ, s, 1, 64)
    absent = probe[32:]
    assert not np.isin(absent, build).any()
    assert [S.walk_length(a, occ, 64, 64) for a in absent] == [run, 1, 0]


@pytest.mark.parametrize("dup", [False, True])
def test_half_table_run(dup):
    build, probe, _ = S.half_table_run(dup)
    assert len(build) == 32 and len(np.unique(build)) == 32 - dup and np.all(S.home(build, 64) == 40)
    occ = S.occupied(build, 64, 64)
    assert occ.tolist() == list(range(0, 8)) + list(range(40, 64))
    absent = probe[32:]
    assert not np.isin(absent, build).any() and S.home(absent, 64).tolist() == [40, 56, 7]
    assert [S.walk_length(a, occ, 64, 64) for a in absent] == [32, 16, 1]


def test_tiny():
    for nb, np_ in S.TINY:
        build, probe, _ = S.tiny(nb, np_)
        assert (len(build), len(probe)) == (nb, np_) and S.capacity_of(nb) == 64
        assert np.isin(probe, build).any() and (np_ == 1 or not np.isin(probe, build).all())


# ----------------------------------------------------------------------------- region-built tables
def region_counts(build):
    return np.bincount(S.home(build, S.REGION_CAP) // S.RS, minlength=S.NREG)


def check_region_build(build, unique=True):
    assert len(build) == S.REGION_NB and S.capacity_of(len(build)) == S.REGION_CAP == S.NREG * S.RS
    assert layout(len(build), 0, 1)[1:] == (S.REGION_CAP, S.home(0, S.REGION_CAP)[0], S.RS, S.RS, S.RLIMIT)
    if unique:
        assert len(np.unique(build)) == len(build)
    return region_counts(build)


def test_region_filler():
    f = S.region_filler()
    cnt = check_region_build(f)
    assert np.all(cnt[S.RESERVED] == 0) and cnt.max() < S.RLIMIT // 2 and (cnt == 0).sum() == len(S.RESERVED)


def test_region_end_runs():
    build, probe, _ = S.region_end_runs()
    cnt = check_region_build(build)
    assert cnt.max() <= S.RLIMIT
    by_region, by_table = S.occupied(build, S.REGION_CAP, S.RS), S.occupied(build, S.REGION_CAP, S.REGION_CAP)
    set_region, set_table = set(by_region.tolist()), set(by_table.tolist())
    assert S.END_REGIONS == (0, 255, S.NREG - 1)  # the last region's wrap is also the table's
    for r in S.END_REGIONS:
        assert cnt[r] == 8
        lo = r * S.RS + 8190
        # region-built: 8190, 8191, then the region's own slots 0..5; nothing else in the region
        assert slots(set_region, lo, 8, S.RS)
        assert by_region[(by_region >= r * S.RS) & (by_region < (r + 1) * S.RS)].tolist() == \
            [r * S.RS + s for s in (0, 1, 2, 3, 4, 5, 8190, 8191)]
        # table-wide: 8190, 8191, then the NEXT region's slots 0..5 (region 511: the table's,
        # in front of region 0's own end run)
        assert slots(set_table, lo, 8, S.REGION_CAP)
        nxt = ((r + 1) % S.NREG) * S.RS
        assert by_table[(by_table >= nxt) & (by_table < nxt + 8190)].tolist() == [nxt + s for s in range(6)]
    absent = probe[~np.isin(probe, build)]
    ha = S.home(absent, S.REGION_CAP)
    for r in S.END_REGIONS:
        # an absent key homed at the last slot walks the run from there under either rule: 7 slots
        a = absent[ha == r * S.RS + 8191]
        assert len(a) == 1
        assert S.walk_length(a[0], set_region, S.REGION_CAP, S.RS) == 7
        assert S.walk_length(a[0], set_table, S.REGION_CAP, S.REGION_CAP) == 7
        # one homed at a region's first slot walks the wrapped six: region-built in the run's
        # own region, table-wide in the next one
        for q in (r, (r + 1) % S.NREG):
            a = absent[ha == q * S.RS]
            assert len(a) == 1
            assert S.walk_length(a[0], set_region, S.REGION_CAP, S.RS) == (6 if q in S.END_REGIONS else 0)
            assert S.walk_length(a[0], set_table, S.REGION_CAP, S.REGION_CAP) == \
                (6 if (q - 1) % S.NREG in S.END_REGIONS else 0)
    assert np.isin(probe, build).sum() >= 24 + 2000


@pytest.mark.parametrize("variant", S.REGION_DUP_VARIANTS)
def test_region_duplicate(variant):
    build, probe, _ = S.region_duplicate(variant)
    cnt = check_region_build(build, unique=False)
    keys, counts = np.unique(build, return_counts=True)
    assert len(keys) == len(build) - 1 and counts.max() == 2
    k = keys[counts == 2][0]
    assert cnt[S.DUP_REGION] == 2 and cnt[S.DUP_REGION + 1] == 0 and cnt.max() <= S.RLIMIT
    s = 4000 if variant == "adjacent" else 8191
    h = S.DUP_REGION * S.RS + s
    assert S.home(k, S.REGION_CAP)[0] == h
    by_region, by_table = S.occupied(build, S.REGION_CAP, S.RS), S.occupied(build, S.REGION_CAP, S.REGION_CAP)
    assert slots(by_region, h, 2, S.RS) and slots(by_table, h, 2, S.REGION_CAP)
    if variant == "wrapped":  # the twin sits in the region's slot 0, or in the next region's
        assert S.DUP_REGION * S.RS in set(by_region.tolist()) and (S.DUP_REGION + 1) * S.RS in set(by_table.tolist())
    assert (probe == k).sum() == 1


@pytest.mark.parametrize("extra", [0, 1])
def test_region_full(extra):
    build, probe, _ = S.region_full(extra)
    cnt = check_region_build(build)
    assert cnt[S.FULL_REGION] == S.RLIMIT + extra == 7168 + extra
    assert np.delete(cnt, S.FULL_REGION).max() < S.RLIMIT   # no other region decides the path
    mine = build[S.home(build, S.REGION_CAP) // S.RS == S.FULL_REGION]
    spread = np.bincount(S.home(mine, S.REGION_CAP) % S.RS, minlength=S.RS)
    assert spread.max() == 1 and (spread > 0).sum() == 7168 + extra   # distinct homes all over the region
    assert np.isin(mine, probe).all()
    absent = probe[~np.isin(probe, build)]
    assert len(absent) == 1000 and np.all(S.home(absent, S.REGION_CAP) // S.RS == S.FULL_REGION)


def test_region_long_run():
    build, probe, _ = S.region_long_run()
    cnt = check_region_build(build)
    assert cnt[S.RUN_REGION] == S.RLIMIT and cnt[S.RUN_REGION + 1] == 0 and np.delete(cnt, S.RUN_REGION).max() < S.RLIMIT
    h = S.RUN_REGION * S.RS + S.RUN_SLOT
    mine = build[S.home(build, S.REGION_CAP) // S.RS == S.RUN_REGION]
    assert np.all(S.home(mine, S.REGION_CAP) == h)
    by_region, by_table = S.occupied(build, S.REGION_CAP, S.RS), S.occupied(build, S.REGION_CAP, S.REGION_CAP)
    assert slots(by_region, h, S.RLIMIT, S.RS) and slots(by_table, h, S.RLIMIT, S.REGION_CAP)
    assert S.RUN_SLOT + S.RLIMIT > S.RS      # region-built, the run wraps
    absent = probe[~np.isin(probe, build)]
    assert len(absent) == S.RUN_ABSENT and (np.isin(probe, mine)).sum() == S.RUN_PRESENT
    # L = 7168: an absent key homed at the run's start reads every slot of the run
    occ_r, occ_t = set(by_region.tolist()), set(by_table.tolist())
    for a in absent[:3]:
        assert S.walk_length(a, occ_r, S.REGION_CAP, S.RS) == 7168
        assert S.walk_length(a, occ_t, S.REGION_CAP, S.REGION_CAP) == 7168
    assert np.all(S.home(absent, S.REGION_CAP) == h)


# ----------------------------------------------------------------------------- tile edges
def matches(build, probe):
    keys, counts = np.unique(build, return_counts=True)
    i = np.searchsorted(keys, probe)
    i[i == len(keys)] = 0
    return np.where(keys[i] == probe, counts[i], 0)


def test_tile_edge_sizes():
    assert S.TILE_NPROBE == sorted({1, 63, 64, 65} | {n for t in (1024, 2048, 4096, 8192)
                                                      for n in (t - 1, t, t + 1, 2 * t + 1)})
    assert all(t % S.EDGE_STEP == 0 for t in S.TILES)


@pytest.mark.parametrize("repeated", [False, True])
def test_tile_edges(repeated):
    top = 3 if repeated else 1
    for n in S.TILE_NPROBE:
        build, probe, _ = S.tile_edges(n, repeated)
        assert len(build) == 25 and len(probe) == n
        m = matches(build, probe)
        assert set(np.unique(m).tolist()) <= ({0, 1, 3} if repeated else {0, 1})
        for t in S.TILES:
            for edge in range(t, n + 1, t):   # the last lane of a tile, the first of the next
                assert m[edge - 1] == top and (edge == n or m[edge] == top), (n, t, edge)
                assert m[edge - 2] == 0 and (edge + 1 >= n or m[edge + 1] == 0)
        if n > 65:
            assert set(np.unique(m).tolist()) == ({0, 1, 3} if repeated else {0, 1})
    build, probe, _ = S.big_probe()
    assert len(probe) == 65 * 8192 + 1 and -(-len(probe) // 8192) == 66 and matches(build, probe).max() == 1
