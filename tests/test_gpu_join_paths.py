"""Every branch of the hash join (csrc/join.hip) on directed inputs, bit-exact against the
numpy oracle (oracle.join_i64) with test_gpu_join.check: pairs in probe-row order, each
probe row's build rows compared sorted.

tests/join_shapes.py builds the inputs — keys with chosen home slots, since the home hash
is invertible — and tests/test_join_shapes_cpu.py proves, against the library's own layout
arithmetic (nut_join_layout), that they hold what they claim: runs across the end of a
64-slot table and of regions 0, 255 and 511 of a 2^22-slot table, exactly one duplicated
build key (adjacent, behind foreign keys, behind a wrap), a region of exactly 7168 and of
7169 records, runs of 32 and of 7168 distinct keys, and 3-match probe rows on the last
lane of every probe tile and the first lane of the next.  DESIGN.md §4.4 maps each
kernel branch to its case.  Every join type, both API forms (nut_join_i64_into;
nut_join_i64 + nut_join_write) and the ordered and the unordered probe run on each case
unless it says otherwise; the oracle's result is computed once per input."""
import ctypes as C

import numpy as np
import pytest
import torch

import join_shapes as S
from test_gpu_exec import dev, host
from test_gpu_join import HOW, canon, check

pytestmark = pytest.mark.gpu

NUT_OK, NUT_ERR_CAPACITY = 0, 5
FORMS = [(1, False), (2, False), (1, True), (2, True)]   # (passes, any_order)


class Memo:
    """The oracle with its results kept per (build, probe, type): the arrays are the
    builders' cached ones, so their identity names the input."""

    def __init__(self, orc):
        self.orc, self.seen = orc, {}

    def join_i64(self, b, p, how):
        k = (id(b), id(p), how)
        if k not in self.seen:
            self.seen[k] = (b, p, self.orc.join_i64(b, p, how))
        return self.seen[k][2]


@pytest.fixture(scope="module")
def memo(orc):
    return Memo(orc)


def run(ex, memo, case, hows=HOW, forms=FORMS):
    b, p, note = case
    for how in hows:
        for passes, any_order in forms:
            try:
                check(ex, memo, b, p, how, passes=passes, any_order=any_order)
            except AssertionError as e:
                raise AssertionError(f"{note}: {how}, passes={passes}, any_order={any_order}: {e}") from None


def pairs_per_probe_row(memo, b, p, how):
    return np.bincount(memo.join_i64(b, p, how)[0], minlength=len(p))


# ----------------------------------------------------------------------------- 64-slot tables (global CAS build)
@pytest.mark.parametrize("match", [1, 0])
def test_run_across_the_table_end(ex, memo, opts, match):
    """hj_next's wrap at the table's last slot in the build, the duplicate check and every
    probe: six keys over slots 62, 63, 0..3; absent keys walk 6, 5, 4 and 0 slots."""
    opts(join_match=match)
    run(ex, memo, S.table_end_run())


@pytest.mark.parametrize("match", [1, 0])
@pytest.mark.parametrize("variant", S.DUP_VARIANTS)
def test_one_duplicated_build_key(ex, memo, opts, variant, match):
    """31 distinct build keys and one repeat: hj_dupcheck_kernel must set the flag from
    that one pair — its twin adjacent, behind foreign keys of its run, behind the table's
    wrap — or INNER / LEFT stop at the first match (and take the two-pass write) and drop a
    pair.  INNER / LEFT: two pairs for the repeated key, one for every other build key."""
    opts(join_match=match)
    b, p, note = case = S.one_duplicate(variant)
    k = b[-1]
    for how in ("inner", "left"):
        n = pairs_per_probe_row(memo, b, p, how)
        assert np.all(n[p == k] == 2) and np.all(n[:32][p[:32] != k] == 1) and (p == k).sum() == 2, note
    run(ex, memo, case)


@pytest.mark.parametrize("dup", [False, True])
def test_half_table_run(ex, memo, opts, dup):
    """32 keys homed at one slot: a run over half the table and across its end; probes of
    every key and absent keys that walk 32, 16 and 1 slots.  dup: one of the 32 repeats
    another, somewhere in the run (the duplicate check must walk past foreign keys)."""
    for match in (1, 0):
        opts(join_match=match)
        run(ex, memo, S.half_table_run(dup))


@pytest.mark.parametrize("nb,np_", S.TINY)
def test_tiny_sides(ex, memo, nb, np_):
    run(ex, memo, S.tiny(nb, np_))


# ----------------------------------------------------------------------------- 2^22 slots: region build and its fallback
def run_regions(ex, memo, opts, case, hows=HOW, forms=FORMS):
    """join_region 1 (hj_region_build_kernel, runs wrap inside a region) and 0 (global CAS,
    runs wrap at the table's end): both must equal the oracle, so each other."""
    for region in (1, 0):
        opts(join_region=region)
        run(ex, memo, case, hows, forms)


def test_runs_across_region_ends(ex, memo, opts):
    """Eight keys homed at the last two slots of regions 0, 255 and 511: built in LDS the
    run wraps to the region's own first slots and the probes must wrap there too (t.wmask);
    built table-wide it runs on into the next region, for region 511 across the table's
    end."""
    run_regions(ex, memo, opts, S.region_end_runs())


@pytest.mark.parametrize("variant", S.REGION_DUP_VARIANTS)
def test_one_duplicate_inside_a_region(ex, memo, opts, variant):
    """Unique filler keys and one repeated key: the region build's own duplicate check (and
    hj_dupcheck_kernel on a 2^22-slot table) must flag it.  INNER / LEFT: two pairs."""
    b, p, note = case = S.region_duplicate(variant)
    s = np.sort(b)
    k = s[1:][s[1:] == s[:-1]][0]
    for how in ("inner", "left"):
        assert pairs_per_probe_row(memo, b, p, how)[p == k].tolist() == [2], note
    run_regions(ex, memo, opts, case)


@pytest.mark.parametrize("extra", [0, 1])
def test_region_at_its_record_limit(ex, memo, opts, extra):
    """7168 records in one region: built in LDS with all 7 records of every lane live.
    7169: the whole table falls back to the global CAS build."""
    run_regions(ex, memo, opts, S.region_full(extra), forms=[(1, False), (2, True)])


def test_run_of_7168_distinct_keys(ex, memo, opts):
    """7168 keys homed at one slot: absent keys homed at the run's start walk all 7168 slots
    with one live lane in their wave."""
    run_regions(ex, memo, opts, S.region_long_run(), forms=[(1, False), (2, True)])


# ----------------------------------------------------------------------------- tile edges
@pytest.mark.parametrize("repeated", [False, True])
@pytest.mark.parametrize("cfg", range(5))
def test_tile_edges_ordered_one_pass(ex, memo, opts, cfg, repeated):
    """hj_probe_kernel<WRITE> in every tile shape (join_probe_cfg), one ordered pass."""
    opts(join_match=0, join_probe_cfg=cfg)
    for n in S.TILE_NPROBE:
        run(ex, memo, S.tile_edges(n, repeated), forms=[(1, False)] if cfg else [(1, False), (2, False)])


@pytest.mark.parametrize("repeated", [False, True])
@pytest.mark.parametrize("cfg", range(5))
def test_tile_edges_unordered(ex, memo, opts, cfg, repeated):
    """hj_probe_kernel<WRITE, ANY> in every tile shape (join_any_cfg)."""
    opts(join_any_cfg=cfg)
    for n in S.TILE_NPROBE:
        run(ex, memo, S.tile_edges(n, repeated), forms=[(1, True)] if cfg else [(1, True), (2, True)])


@pytest.mark.parametrize("repeated", [False, True])
@pytest.mark.parametrize("cfg", range(5))
def test_tile_edges_two_pass(ex, memo, opts, cfg, repeated):
    """join_match = 1: hj_match_kernel in every shape (join_any_cfg) and the 512 x 16
    write-out from the match array, wherever no probe row can match two build rows (unique
    build keys, SEMI / ANTI); repeated keys under INNER / LEFT stay on the one-pass kernel."""
    opts(join_match=1, join_any_cfg=cfg)
    for n in S.TILE_NPROBE:
        run(ex, memo, S.tile_edges(n, repeated), forms=[(1, False)] if cfg else [(1, False), (2, False)])


def test_write_out_look_back_second_step(ex, memo, opts):
    """65 x 8192 + 1 probe rows over unique build keys: 66 write-out tiles, so the last
    tiles' look-back reads more than one 64-tile step."""
    opts(join_match=1)
    run(ex, memo, S.big_probe(), forms=[(1, False)])


# ----------------------------------------------------------------------------- capacity
SENTINEL = -0x0123456789ABCDEF
JOIN_TYPES = {"inner": 0, "left": 1, "semi": 2, "anti": 3}
NUT_JOIN_ANY_ORDER = 0x100


def join_into_raw(ex, b, p, how, any_order, out_p, out_b, cap):
    from nutdb_amd._lib import lib
    n = C.c_uint64()
    ex._bind_stream()
    st = lib.nut_join_i64_into(ex.ctx, C.c_void_p(b.data_ptr()), b.numel(), C.c_void_p(p.data_ptr()), p.numel(),
                               JOIN_TYPES[how] | (NUT_JOIN_ANY_ORDER if any_order else 0),
                               C.c_void_p(out_p.data_ptr()) if out_p is not None else None,
                               C.c_void_p(out_b.data_ptr()) if out_b is not None else None, cap, C.byref(n))
    ex.sync()
    return st, n.value


@pytest.mark.parametrize("any_order", [False, True])
@pytest.mark.parametrize("how", ["inner", "left", "semi"])
def test_capacity_writes_nothing_behind_cap(ex, memo, how, any_order):
    """nut_join_i64_into with cap below the pair count P: NUT_ERR_CAPACITY, *npairs = P and
    no entry at or behind cap written (the arrays hold P + 64 sentinels); cap = P: the
    oracle's pairs and the 64 tail entries untouched.  8193 probe rows (three ordered
    tiles) with 0, 1 or 3 matches each; one cap falls inside a 3-pair group."""
    b, p, _ = S.tile_edges(2 * 4096 + 1, True)
    wp, wb = memo.join_i64(b, p, how)
    total = len(wp)
    per_row = np.bincount(wp, minlength=len(p))
    starts = np.cumsum(per_row) - per_row
    rows3 = np.flatnonzero(per_row == (1 if how == "semi" else 3))
    row3 = rows3[len(rows3) // 3]
    inside = int(starts[row3]) + (0 if how == "semi" else 2)   # semi: no groups, a cap inside the pairs
    assert how == "semi" or (per_row[row3] == 3 and starts[row3] < inside < starts[row3] + 3)
    db, dp = dev(b, ex), dev(p, ex)
    out_p = torch.empty(total + 64, dtype=torch.int64, device=ex.device)
    out_b = torch.empty(total + 64, dtype=torch.int64, device=ex.device)
    for cap in (0, 1, total - 1, inside):
        assert cap < total
        out_p.fill_(SENTINEL)
        out_b.fill_(SENTINEL)
        assert join_into_raw(ex, db, dp, how, any_order, out_p, out_b, cap) == (NUT_ERR_CAPACITY, total), cap
        assert np.all(host(out_p[cap:]) == SENTINEL) and np.all(host(out_b[cap:]) == SENTINEL), cap
    assert join_into_raw(ex, db, dp, how, any_order, None, None, 0) == (NUT_ERR_CAPACITY, total)
    out_p.fill_(SENTINEL)
    out_b.fill_(SENTINEL)
    assert join_into_raw(ex, db, dp, how, any_order, out_p, out_b, total) == (NUT_OK, total)
    assert np.all(host(out_p[total:]) == SENTINEL) and np.all(host(out_b[total:]) == SENTINEL)
    gp, gb = host(out_p[:total]), host(out_b[:total])
    if not any_order:
        assert np.all(gp[1:] >= gp[:-1])
    gp, gb = canon(gp, gb)
    assert np.array_equal(gp, wp) and np.array_equal(gb, wb)
