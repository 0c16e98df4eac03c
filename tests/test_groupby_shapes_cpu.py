"""CPU proof that tests/groupby_shapes.py builds what it claims (no GPU): the Python model
equals the library's own layout arithmetic (nut_groupby_layout, csrc/gb_layout.hpp) over
random and edge tuples, every hint class and every table capacity the directed suite uses;
and for every builder the note is proven FROM THE EXPORT ALONE (`place` below asks the
library, not the model): bucket or slot of each key, chain length, equal words with unequal
tuples, counts exactly at and one past each limit, shard membership, owner part, partition
digit.  The row counts of the loop-size cases are proven from the exported launch figures."""
import ctypes as C

import numpy as np
import pytest

import groupby_shapes as S

I64_MIN, I64_MAX = S.I64_MIN, S.I64_MAX
NUT_ERR_INVALID_ARG = 1


lib_layout = S.library_layout


def place(case, na=4, hint=None, table_cap=0, **kw):
    """The export's view of every tuple of a case: a dict of int arrays."""
    hint = case.hint if hint is None else hint
    cols = [k.tolist() for k in case.keys] + ([[0] * len(case.keys[0])] if case.nk == 1 else [])
    out = [lib_layout(case.nk, na, hint, key=t, table_cap=table_cap, **kw) for t in zip(*cols)]
    return {f: np.array([o[f] for o in out], dtype=np.uint64 if f in ("lds_word", "hash", "owner_hash") else np.int64)
            for f in out[0]}


def chain(homes, cap):
    """Occupied slots after linear probing from `homes` (any insertion order), with wrap."""
    occ = set()
    for h in sorted(int(x) for x in homes):
        while h in occ:
            h = (h + 1) % cap
        occ.add(h)
    # a second pass in reverse order must give the same set (order independence)
    occ2 = set()
    for h in sorted((int(x) for x in homes), reverse=True):
        while h in occ2:
            h = (h + 1) % cap
        occ2.add(h)
    assert occ == occ2
    return occ


def distinct_tuples(case):
    return len(np.unique(np.stack(case.keys, axis=1), axis=0)) == len(case.keys[0])


# ----------------------------------------------------------------------------- the model
HINTS = [0, 1, 3, 8, 9, 100, 512, 1024, 2048, 4096, 16384, 16385, 65537, 131072, 131073, 300000]
EDGE = [(0, 0), (1, 0), (255, 0), (256, 0), (-1, 0), (15, 15), (16, 0), (0, 16), (I64_MIN, 0), (I64_MAX, I64_MIN),
        (I64_MIN, I64_MIN), (-1, -1)]


@pytest.mark.parametrize("nk", [1, 2])
def test_model_equals_the_library(nk):
    """Every field, for each hint class (none, private, shared small and largest, no on-chip
    table, sharded global table, two partition levels) x 0, 1, 4, 5, 8 aggregates x streaming
    and segment mode x both kernel kinds, on edge tuples, random tuples and the tuples of the
    directed cases; launch figures at the tail and loop row counts."""
    rng = np.random.default_rng(nk)
    rnd = [tuple(t) for t in rng.integers(I64_MIN, I64_MAX, (40, 2), dtype=np.int64).tolist()]
    # the one tuple whose lkey<2> hash is the empty marker, and its neighbour
    nudged = [(int(a), int(b)) for a, b in zip(*S.b2_nudged().keys)]
    tuples = EDGE + rnd + nudged
    i = 0
    for hint in HINTS:
        for na in (0, 1, 4, 5, 8):
            for seg in (0, 1):
                for expr in (0, 1):
                    i += 1
                    t = tuples[i % len(tuples)]
                    n = (0, 1, 5, 4099, 1836025, 10 ** 7)[i % 6]
                    kw = dict(key=t, segment=seg, expr=expr, n=n, agg_blocks=i % 3, num_cus=(256, 304, 1)[i % 3],
                              slots=(0, 2, 8)[i % 3])
                    assert lib_layout(nk, na, hint, **kw) == S.layout(nk, na, hint, **kw), (hint, na, kw)
    for t in tuples:
        for cap in (1024, 2048, 4096, 1 << 14, 1 << 18, 1 << 19, 1 << 26):
            assert lib_layout(nk, 4, 9, key=t, table_cap=cap) == S.layout(nk, 4, 9, key=t, table_cap=cap), (t, cap)


def test_layout_rules_and_errors():
    from nutdb_amd._lib import NutGroupbyLayoutInfo, NutGroupbyLayoutQuery, lib
    # hint 9: 64 slots, 48 admitted; hint 0: 4096 slots where they fit (one aggregate), else the largest table
    assert (lib_layout(1, 4, 9)["lds_cap"], lib_layout(1, 4, 9)["lds_limit"]) == (64, 48)
    assert lib_layout(1, 1, 0)["lds_cap"] == 4096 and lib_layout(1, 4, 0)["lds_cap"] == 2048
    assert lib_layout(1, 1, 4096)["lds_cap"] == 8192 and lib_layout(1, 4, 4096)["lds_cap"] == 2048
    for nk, na in ((1, 1), (1, 2), (1, 4), (2, 4)):
        h = S.no_lds_hint(nk, na)
        assert lib_layout(nk, na, h - 1)["lds_cap"] > 0 and lib_layout(nk, na, h)["lds_cap"] == 0, (nk, na)
    # the smallest global table: 1024 slots, overflow flagged at the 769th claim; regrows x 4
    o = lib_layout(1, 4, 1)
    assert (o["table_cap"], o["limit"], o["nshards"], o["limit_shard"]) == (1024, 768, 1, 768)
    assert lib_layout(1, 4, 1, table_cap=4096)["limit"] == 3072
    # 2^18 slots: 256 shards of 816 claims, 1280 arena entries (two keys)
    o = lib_layout(2, 4, S.SHARD_HINT)
    assert (o["table_cap"], o["nshards"], o["limit_shard"], o["arena_shard_limit"]) == (1 << 18, 256, 816, 1280)
    assert lib_layout(1, 4, S.SHARD_HINT + 1)["table_cap"] == 1 << 19 and lib_layout(1, 4, 65536)["nshards"] == 1
    # private accumulators: up to 8 hinted groups; C4: 8 groups fit with 4 aggregates, not with 5
    assert [lib_layout(1, 4, h)["priv"] for h in (0, 1, 3, 8, 9)] == [0, 1, 3, 8, 0]
    assert lib_layout(1, 4, 8)["priv"] == 8 and lib_layout(1, 5, 8)["priv"] == 0
    assert lib_layout(1, 4, 8, segment=1)["priv"] == 0 and lib_layout(1, 0, 8)["priv"] == 0
    assert (lib_layout(1, 4, 8)["threads"], lib_layout(1, 4, 8, expr=1)["threads"], lib_layout(1, 4, 9)["threads"]) == \
        (256, 192, 512)
    q, o = NutGroupbyLayoutQuery(nkeys=1, naggs=4, num_cus=256), NutGroupbyLayoutInfo()
    assert lib.nut_groupby_layout(None, C.byref(o)) == NUT_ERR_INVALID_ARG
    assert lib.nut_groupby_layout(C.byref(q), None) == NUT_ERR_INVALID_ARG
    for bad in (dict(nkeys=0), dict(nkeys=3), dict(naggs=9), dict(num_cus=0), dict(table_cap=1000), dict(table_cap=512),
                dict(slots_per_group=9)):
        q = NutGroupbyLayoutQuery(**{**dict(nkeys=1, naggs=4, num_cus=256), **bad})
        assert lib.nut_groupby_layout(C.byref(q), C.byref(o)) == NUT_ERR_INVALID_ARG, bad


def test_inverses():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 1 << 64, 20000, dtype=np.uint64)
    k2 = rng.integers(I64_MIN, I64_MAX, 20000, dtype=np.int64)
    # lkey<2> (before the nudge), key_hash<2> and owner_hash reach any word from any k2 / k1
    k1 = S.tuple_with_word(x, k2)
    assert np.array_equal(S.lkey2(k1, k2), np.where(x == np.uint64(S.EMPTY), x ^ np.uint64(1), x))
    assert np.array_equal(S.key_hash(2, S.tuple_with_hash(x, k2), k2), x)
    assert np.array_equal(S.owner_hash(1, S.key_with_owner_hash(x)), x)
    assert np.array_equal(S.owner_hash(2, k2, S.tuple_with_owner_hash(x, k2)), x)
    for cap in (32, 64, 2048, 4096, 8192):
        home = rng.integers(0, cap // 4, 2000) * 4
        for hi in (0, 0xFFFFFFFF, 0x12345678):
            w = S.lds_word_at(home, cap, np.arange(2000), hi)
            assert np.array_equal(S.lhome(w, cap), home) and np.all(w >> np.uint64(32) == np.uint64(hi))
            assert len(np.unique(w)) == 2000
    for cap in (1024, 1 << 18):
        slot = np.concatenate([[0, cap - 1], rng.integers(0, cap, 2000)])
        h = S.gkey_at(slot, cap, 1 + np.arange(len(slot)))
        assert np.array_equal(S.slot_of(h, cap), slot) and len(np.unique(h)) == len(h)


# ----------------------------------------------------------------------------- single-key on-chip table
TABLES = [(9, 4, 64), (0, 4, 2048), (4096, 4, 2048), (0, 1, 4096), (4096, 1, 8192), (4096, 2, 4096)]  # hint, na, slots


@pytest.mark.parametrize("hint,na,cap", TABLES)
@pytest.mark.parametrize("hi", S.HIS)
def test_single_key_chains(hint, na, cap, hi):
    assert lib_layout(1, na, hint)["lds_cap"] == cap
    mid = S.MID(cap)
    p = place(S.a1_bucket(cap, hi), na, hint)
    assert np.all(p["lds_home"] == mid) and len(p["lds_home"]) == 4 and p["lds_bucket"][0] == 4
    assert chain(p["lds_home"], cap) == set(range(mid, mid + 4))            # all inside the home bucket
    p = place(S.a2_chain(cap, hi), na, hint)
    assert np.all(p["lds_home"] == mid) and chain(p["lds_home"], cap) == set(range(mid, mid + 12))
    assert 12 <= p["lds_limit"][0]                                          # all admitted
    p = place(S.a3_wrap(cap, hi), na, hint)
    assert np.all(p["lds_home"] == cap - 4)
    assert chain(p["lds_home"], cap) == set(range(cap - 4, cap)) | set(range(8))   # across the table's end
    p = place(S.a4_behind(cap, hi), na, hint)
    assert sorted(p["lds_home"].tolist()) == [mid] * 5 + [mid + 4] * 4
    assert chain(p["lds_home"], cap) == set(range(mid, mid + 9))            # one key past two full buckets
    for c in (S.a1_bucket(cap, hi), S.a2_chain(cap, hi), S.a3_wrap(cap, hi), S.a4_behind(cap, hi)):
        k = c.keys[0].view(np.uint64)
        assert np.all(k >> np.uint64(32) == np.uint64(hi)) and not np.any(k == np.uint64(S.EMPTY))
        assert np.array_equal(place(c, na, hint)["lds_word"], k)            # one key: the word is the key


def test_single_key_counts_extremes_and_folds():
    o = lib_layout(1, 4, 9)
    assert (o["lds_cap"], o["lds_limit"], o["priv"]) == (64, 48, 0)
    for K in (48, 49, 64, 200):                    # at the limit, one past it, the slot count, far past
        c = S.a5_count(K)
        assert len(c.keys[0]) == K and distinct_tuples(c) and c.hint == 9
    c = S.a6_extremes(64)
    p = place(c, 4, 9)
    assert {I64_MIN, I64_MAX, -1, 0} <= set(c.keys[0].tolist()) and len(c.keys[0]) == 16
    assert int(p["lds_word"][c.keys[0] == I64_MIN][0]) == S.EMPTY            # the special slot's key
    assert np.all(p["lds_home"][:12] == S.MID(64))
    c = S.a7_swapped_halves()
    k = c.keys[0].view(np.uint64)
    swapped = (k << np.uint64(32)) | (k >> np.uint64(32))
    assert set(swapped.tolist()) == set(k.tolist()) and not np.any(swapped == k)
    for hint, na, cap in TABLES:
        p = place(c, na, hint)
        assert np.array_equal(p["lds_home"][:6], p["lds_home"][6:])         # each pair shares a home
    c = S.a8_no_table(4)
    o = lib_layout(1, 4, c.hint, n=4099)
    assert o["lds_cap"] == 0 and o["levels"] == 1 and c.hint < 65536 and I64_MIN in c.keys[0]
    assert len(c.keys[0]) == 257 < o["limit"]


# ----------------------------------------------------------------------------- two-key on-chip table
TABLES2 = [(9, 4, 64), (0, 4, 2048)]


@pytest.mark.parametrize("hint,na,cap", TABLES2)
def test_two_key_words_and_chains(hint, na, cap):
    assert lib_layout(2, na, hint)["lds_cap"] == cap
    mid = S.MID(cap)
    for m in (2, 3):
        for across in (False, True):
            c = S.b1_same_word(cap, m, across)
            p = place(c, na, hint)
            assert distinct_tuples(c) and len(set(p["lds_word"][:m].tolist())) == 1   # unequal tuples, one word
            assert np.all(p["lds_home"] == mid)
            n = m + (4 if across else 0)
            assert len(set(p["lds_word"].tolist())) == n - m + 1
            assert chain(p["lds_home"], cap) == set(range(mid, mid + n)) and (n > 4) == across
    for wrap in (False, True):
        c = S.b4_chain(cap, wrap)
        p = place(c, na, hint)
        h = cap - 4 if wrap else mid
        assert np.all(p["lds_home"] == h) and len(set(p["lds_word"].tolist())) == 12
        assert chain(p["lds_home"], cap) == {(h + i) % cap for i in range(12)}


def test_two_key_nudge_and_limit():
    c = S.b2_nudged()
    p = place(c, 4, 9)
    w = p["lds_word"].tolist()
    # the first tuple's hash is the empty marker itself: nudged onto the second tuple's word
    assert int(S.tuple_with_word(S.EMPTY, 5)[0]) == int(c.keys[0][0]) and distinct_tuples(c)
    assert w[0] == w[1] == S.EMPTY ^ 1 and w[2:] == [S.EMPTY ^ 2, S.EMPTY ^ 3] and S.EMPTY not in w
    o = lib_layout(2, 4, 9)
    assert (o["lds_cap"], o["lds_limit"]) == (64, 48)
    assert lib_layout(2, 4, 8)["lds_cap"] == 32 and lib_layout(2, 4, 8)["lds_limit"] == 24 and lib_layout(2, 4, 8)["priv"] == 8
    for K in (24, 25, 48, 49, 200):
        assert len(S.b3_count(K).keys[0]) == K and distinct_tuples(S.b3_count(K))


# ----------------------------------------------------------------------------- private accumulators
def test_private_cases():
    c = S.c1_direct_edge()
    p = place(c, 4)
    assert p["priv"][0] == 8 and p["direct_size"][0] == 256
    assert p["direct_idx"].tolist() == [255, 256, 256, 0, 7]                # 255 inside, 256 and -1 outside
    c = S.c2_direct_edge()
    p = place(c, 4)
    assert p["priv"][0] == 8 and p["direct_idx"].tolist() == [255, 256, 256, 256, 0, 3 * 16 + 4]
    c = S.c3_ids_run_out()
    p = place(c, 4)
    assert p["priv"][0] == 3 < len(c.keys[0]) == 6 <= p["lds_limit"][0]
    c = S.c4_cutoff()
    assert place(c, 4)["priv"][0] == 8 and place(c, 5)["priv"][0] == 0 and len(c.keys[0]) == 8
    assert place(c, 5)["threads"][0] == 512 and place(c, 4)["threads"][0] == 256


# ----------------------------------------------------------------------------- global table
def test_global_run_and_regrow_counts():
    c = S.d1_long_run()
    p = place(c)
    assert p["table_cap"][0] == 1024 and np.all(p["home"] == 1020) and len(c.keys[0]) == 100 < p["limit"][0]
    run = chain(p["home"], 1024)
    assert run == set(range(1020, 1024)) | set(range(96)) and len(run) > 63  # wraps; the 63-probe check is reached
    assert np.array_equal(p["hash"], c.keys[0].view(np.uint64))
    o = lib_layout(1, 4, 1)
    assert (o["table_cap"], o["limit"]) == (1024, 768)
    assert [len(S.d2_regrow(K).keys[0]) for K in (768, 769, 3073)] == [768, 769, 3073]
    # 769 > 768: one regrow to 4096 slots (limit 3072 >= 769); 3073 > 3072: a second one, to 16384
    assert lib_layout(1, 4, 1, table_cap=4096)["limit"] == 3072 and lib_layout(1, 4, 1, table_cap=16384)["limit"] >= 3073


def test_global_shards():
    o = lib_layout(1, 4, S.SHARD_HINT, n=4099)
    assert (o["table_cap"], o["lds_cap"], o["limit_shard"], o["nshards"]) == (1 << 18, 0, 816, 256)
    assert 4099 < 4 * S.SHARD_HINT                                          # too few rows for the partitioned path
    for K in (816, 817):
        c = S.d3_claim_shard(K)
        p = place(c)
        assert np.all(p["claim_shard"] == S.D3_SHARD) and len(set(p["home"].tolist())) == K   # K claims, one shard
    for K in (1280, 1281):
        c = S.d6_arena_shard(K)
        p = place(c)
        assert p["arena_shard_limit"][0] == 1280 and np.all(p["arena_shard"] == S.D6_SHARD) and distinct_tuples(c)
        assert np.bincount(p["claim_shard"], minlength=256).max() < 816     # the claim shards stay far below theirs


def test_global_two_key_collisions():
    for m in (2, 3):
        c = S.d4_same_hash(m)
        p = place(c)
        assert distinct_tuples(c) and len(set(p["hash"][:m].tolist())) == 1 and len(set(p["hash"].tolist())) == 4
    c = S.d5_tag_and_slot(1024)
    p = place(c)
    assert p["table_cap"][0] == 1024 and distinct_tuples(c)
    assert p["tag"][0] == p["tag"][1] and p["home"][0] != p["home"][1]
    assert p["home"][2] == p["home"][3] and p["tag"][2] != p["tag"][3]


# ----------------------------------------------------------------------------- compaction, partition, segments
def test_compaction_and_owner_cases():
    for cap in (2048, 4096):
        c = S.e1_special_chunk(cap)
        p = place(c)
        assert p["table_cap"][0] == cap and cap % 2048 == 0 and I64_MIN in c.keys[0] and len(c.keys[0]) < p["limit"][0]
    for nk in (1, 2):
        for P in (1, 2, 64):
            for spread in (False, True):
                c = S.e2_owners(nk, P, spread)
                part = (place(c)["owner_hash"] % np.uint64(P)).astype(np.int64)
                assert distinct_tuples(c)
                assert part.tolist() == (list(range(P)) if spread else [P - 1] * 40)


def test_segment_partition_cases():
    lim = S.seg_limit()
    per = max(64, 2 * ((S.SEG_HINT + 255) // 256))
    o = lib_layout(1, 4, per, segment=1)
    assert (o["lds_cap"], o["lds_limit"]) == (128, 96) and lim == 96
    for K in (lim, lim + 1):
        c = S.g_partition(K)
        d = (place(c)["owner_hash"] >> np.uint64(64 - S.SEG_BITS)).astype(np.int64)
        assert np.bincount(d, minlength=256).tolist() == [K if x == 93 else 1 for x in range(256)]
    # the export's digit is this one whenever level 0 has 8 bits
    k = S.g_partition(lim).keys[0]
    for key in k[:5].tolist() + k[-5:].tolist():
        o = lib_layout(1, 4, 200000, key=(key, 0))
        assert o["l0_bits"] == 8 and o["l0_digit"] == lib_layout(1, 4, 0, key=(key, 0))["owner_hash"] >> 56


# ----------------------------------------------------------------------------- row counts
LAUNCHES = [  # nk, na, hint, expr, agg_blocks: every kernel shape the GPU suite runs at a loop size
    (1, 4, 9, 0, 1), (1, 4, 0, 0, 1), (1, 4, 4096, 0, 1), (1, 1, 4096, 0, 1), (1, 2, 9, 0, 1), (1, 4, 9, 1, 1),
    (2, 4, 9, 0, 1), (2, 4, 0, 0, 1), (1, 4, 8, 0, 0), (2, 4, 8, 0, 0), (1, 4, 8, 1, 0), (2, 4, 8, 1, 0), (1, 4, 3, 0, 0)]


@pytest.mark.parametrize("num_cus", [256, 304])
@pytest.mark.parametrize("nk,na,hint,expr,agg_blocks", LAUNCHES)
def test_row_counts_reach_loop_and_tails(nk, na, hint, expr, agg_blocks, num_cus):
    """Tail sizes: every lane runs no full step.  Loop size: every lane runs at least three
    full steps; exactly one lane's last step has two pairs, others' one pair, others' none."""
    kw = dict(expr=expr, agg_blocks=agg_blocks, num_cus=num_cus)
    for n in S.TAIL_ROWS:
        o = lib_layout(nk, na, hint, n=n, **kw)
        steps, tail = S.lane_steps(n, o["blocks"], o["threads"])
        assert steps.max() == 0 and tail.max() == 1 and tail.sum() == (n + 1) // 2
    big = lib_layout(nk, na, hint, n=1 << 40, **kw)              # the launch that fills the chip
    n = S.loop_rows(big["blocks"], big["threads"])
    o = lib_layout(nk, na, hint, n=n, **kw)
    assert (o["blocks"], o["threads"]) == (big["blocks"], big["threads"]) == (num_cus * o["blocks_per_cu"], o["threads"])
    steps, tail = S.lane_steps(n, o["blocks"], o["threads"])
    assert steps.min() == 3 and steps.max() == 4 and n % 2 == 1
    assert (tail == 2).sum() == 1 and (tail == 1).sum() > 0 and (tail == 0).sum() == 1000
    assert np.all(tail[steps == 4] == 0) and np.all(tail[steps == 3] >= 1)


def test_lane_steps_against_a_walk():
    """lane_steps against walking the kernel's loop lane by lane."""
    for n, blocks, threads in [(0, 1, 4), (1, 1, 4), (7, 1, 4), (8, 1, 4), (9, 1, 4), (33, 2, 4), (100, 3, 4), (101, 3, 4)]:
        g = blocks * threads
        full, npairs = n // 2, (n + 1) // 2
        want = []
        for q in range(g):
            s = 0
            if q + g < full:
                while True:
                    s += 1
                    q += 2 * g
                    if not q + g < full:
                        break
            want.append((s, 0 if q >= npairs else 2 if q + g < npairs else 1))
        steps, tail = S.lane_steps(n, blocks, threads)
        assert list(zip(steps.tolist(), tail.tolist())) == want, (n, blocks, threads)
