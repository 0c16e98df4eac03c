"""CPU proof that tests/compact_shapes.py builds what it claims (no GPU): the model's tile
constants equal the sources' (csrc/filter.hip, csrc/select_kernel.hpp, csrc/lookback.hpp),
and for every builder the claims its GPU test (tests/test_gpu_compact_paths.py) relies on
are recomputed from the mask alone: per-tile totals, `half`, per-(stripe, wave) and
per-(item, wave) counts, and the parities that decide flush_staged's head and tail stores.
The restated kernels (staged_model, select_model, lookback_walk) are held to the numpy
reference on the named cases."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

import compact_shapes as S

CSRC = Path(__file__).resolve().parent.parent / "nutdb_amd" / "csrc"


def source_constants(name, prefix):
    """constexpr integers of a source whose names start with `prefix`, evaluated in order."""
    env = {"kWave": 64}
    text = (CSRC / name).read_text()
    for m in re.finditer(r"constexpr\s+(?:int|uint32_t|uint64_t)\s+(\w+)\s*=\s*([^;]+);", text):
        expr = re.sub(r"(\d+)u(ll)?\b", r"\1", m.group(2))
        try:
            env[m.group(1)] = int(eval(expr, {"__builtins__": {}}, dict(env)))  # arithmetic over earlier names
        except Exception:
            continue
    return {k: v for k, v in env.items() if k.startswith(prefix)}


# ----------------------------------------------------------------------------- the model
def test_constants_equal_the_sources():
    ft = source_constants("filter.hip", "FT_")
    assert ft == {"FT_THREADS": S.FT_THREADS, "FT_WAVES": S.FT_WAVES, "FT_STRIPES": S.FT_STRIPES,
                  "FT_STRIPE_ROWS": S.FT_STRIPE_ROWS, "FT_TILE": S.FT_TILE}
    fs = source_constants("filter.hip", "FS_")
    assert fs == {"FS_THREADS": S.FS_THREADS, "FS_WAVES": S.FS_WAVES, "FS_STRIPES": S.FS_STRIPES,
                  "FS_STRIPE_ROWS": S.FS_STRIPE_ROWS, "FS_TILE": S.FS_TILE, "FS_HALF": S.FS_HALF,
                  "FS_CAP": S.FS_CAP}
    sel = source_constants("select_kernel.hpp", "SEL_")
    assert sel == {"SEL_THREADS": S.SEL_THREADS, "SEL_WAVES": S.SEL_WAVES, "SEL_ITEMS": S.SEL_ITEMS,
                   "SEL_TILE": S.SEL_TILE}
    lb = source_constants("lookback.hpp", "")
    assert (lb["FLAG_AGG"], lb["FLAG_INC"], lb["VAL_MASK"], lb["LB_PER"]) == (S.FLAG_AGG, S.FLAG_INC, S.VAL_MASK, 1)
    assert S.PAIR == {"staged": (32768, 16, 16), "unstaged": (16384, 16, 8)}


def test_geometry():
    """Thread t holds rows 2t, 2t + 1 of each stripe; a wave covers 128 consecutive rows;
    every row of a tile belongs to exactly one (stripe, wave, lane, half) / (item, wave, lane)."""
    for kind, (tile, stripes, waves) in S.PAIR.items():
        j, w, l, h = np.meshgrid(np.arange(stripes), np.arange(waves), np.arange(64), np.arange(2), indexing="ij")
        rows = S.pair_row(kind, j, w, l, h)
        assert np.array_equal(rows.reshape(-1), np.arange(tile))          # row order = (stripe, wave, lane, half)
        t = 64 * w + l
        assert np.array_equal(rows, j * (tile // stripes) + 2 * t + h)
    i, w, l = np.meshgrid(np.arange(32), np.arange(8), np.arange(64), indexing="ij")
    assert np.array_equal(S.sel_row(i, w, l), 512 * i + (64 * w + l))
    assert np.array_equal(S.sel_row(i, w, l).reshape(-1), np.arange(S.SEL_TILE))
    m = np.zeros(3 * 32768 + 5, dtype=bool)
    m[S.FS_TILE + S.pair_row("staged", 3, 9, 63, 1)] = True
    c = S.pair_counts(m, "staged")
    assert c.shape == (4, 16, 16) and c.sum() == 1 and c[1, 3, 9] == 1
    m = np.zeros(2 * 16384, dtype=bool)
    m[S.SEL_TILE + S.sel_row(31, 7, 0)] = True
    c = S.sel_counts(m)
    assert c.shape == (2, 32, 8) and c.sum() == 1 and c[1, 31, 7] == 1


@pytest.mark.parametrize("op", S.OPS)
def test_column_op(op):
    mask = S.mask_of(S.varied(40_001)[0])
    col, k = S.column_op(mask, op)
    assert np.array_equal(S.apply_op(col, op, k), mask) and 0 < mask.sum() < len(mask)
    if op != "==":      # the selected rows are told apart
        assert len(np.unique(col[mask])) == mask.sum()
    col = S.column(mask, row0=5)
    assert np.array_equal(col[mask], 5 + np.flatnonzero(mask)) and np.array_equal(col[~mask], -6 - np.flatnonzero(~mask))
    assert S.SENTINEL not in col and -S.SENTINEL > 1 << 40


# ----------------------------------------------------------------------------- (a) shaped tiles
def shape_claims(kind, name, m):
    tile, stripes, waves = S.PAIR[kind]
    what, *a = name.split(":")
    a = [int(x) for x in a]
    cnt = S.pair_counts(m, kind)[0]
    if what == "total":
        assert m.sum() == a[0]
        if kind == "staged" and 3 < a[0] < tile:   # spread over both halves
            assert abs(int(S.halves(m)[0]) - a[0] // 2) <= 1
    elif what == "dense":
        assert (int(S.halves(m)[0]), int(m.sum() - S.halves(m)[0])) == tuple(a) and m.sum() > S.FS_CAP
    elif what == "wave":
        assert cnt.sum() == 128 and cnt[a[0], a[1]] == 128 and S.max_rank(m, kind) == 126
    elif what == "stripe":
        assert np.array_equal(cnt.sum(axis=1), np.where(np.arange(stripes) == a[0], tile // stripes, 0))
    elif what == "lane":
        assert np.all(cnt == 2) and S.max_rank(m, kind) == 0
        j, w, h = np.meshgrid(np.arange(stripes), np.arange(waves), np.arange(2), indexing="ij")
        assert np.array_equal(np.sort(S.pair_row(kind, j, w, a[0], h).reshape(-1)), np.flatnonzero(m))
    else:
        assert what == "parity" and np.all(cnt == 64) and np.all(np.flatnonzero(m) % 2 == a[0])


@pytest.mark.parametrize("kind,name", [("staged", n) for n in S.STAGED_SHAPES] + [("unstaged", n) for n in S.UNSTAGED_SHAPES])
def test_shaped_tiles(kind, name):
    tile = S.PAIR[kind][0]
    col, _ = S.one_tile(kind, name)
    m = S.mask_of(col)
    assert len(col) == tile
    shape_claims(kind, name, m)
    assert np.array_equal(col[m], np.flatnonzero(m))
    for prev_odd in (True, False):
        col3, _ = S.three_tiles(kind, name, prev_odd)
        m3 = S.mask_of(col3)
        t = S.totals(m3, tile)
        assert len(col3) == 3 * tile and np.array_equal(m3[tile:2 * tile], m)
        assert t[0] % 2 == int(prev_odd) and t[1] == m.sum() and t[2] == S.NEXT_TOTAL
        if kind == "staged":
            out, n = S.staged_model(col3, word0=1)
            assert n == m3.sum() and np.array_equal(out[:n], col3[m3]) and np.all(out[n:] == S.SENTINEL)
    if kind == "staged":
        for word0 in (0, 1):
            out, n = S.staged_model(col, word0)
            assert n == m.sum() and np.array_equal(out[:n], col[m]) and np.all(out[n:] == S.SENTINEL)


def test_staged_thresholds_and_parities():
    """The totals sit exactly at and beside FS_CAP, cnt of 0..3 is there, and the dense tiles
    cover the four parities of (half, total - half), each above the buffer."""
    assert {S.FS_CAP - 1, S.FS_CAP, S.FS_CAP + 1, 0, 1, 2, 3} <= set(S.STAGED_TOTALS)
    par = {(h % 2, r % 2) for h, r in S.STAGED_DENSE}
    assert par == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert all(h + r > S.FS_CAP and max(h, r) <= S.FS_HALF for h, r in S.STAGED_DENSE)
    assert (3841 + 16384, 16383 + 3842) == (S.FS_CAP + 1, S.FS_CAP + 1)   # just past the buffer, both splits
    # total:20225 spreads over both halves: the two-halves path with a first half below a full one
    h = int(S.halves(S.t_total("staged", 20225))[0])
    assert 0 < h < S.FS_HALF and 20225 - h <= S.FS_HALF


# ----------------------------------------------------------------------------- (b) last rows
@pytest.mark.parametrize("kind,sizes", [("staged", S.STAGED_EDGE_N), ("unstaged", S.UNSTAGED_N)])
def test_last_rows(kind, sizes):
    for n in sizes:
        seen = set()
        for bits in range(8):
            col, _ = S.last_rows(n, bits)
            m = S.mask_of(col)
            assert len(col) == n
            seen.add(tuple(m[-3:].tolist()))
            if n > 3:
                assert np.array_equal(m[:n - 3], np.arange(n - 3) % 2 == 0)
            if kind == "staged" and n >= 2:
                out, cnt = S.staged_model(col)
                assert cnt == m.sum() and np.array_equal(out[:cnt], col[m]) and np.all(out[cnt:] == S.SENTINEL)
        assert len(seen) == 2 ** min(n, 3)
        # rows n - 2 and n - 1 selected differently both ways round, and both selected
        assert n < 2 or {(True, False), (False, True), (True, True)} <= {s[-2:] for s in seen}
    assert any(n % 2 for n in sizes) and any(n % 2 == 0 for n in sizes)
    if kind == "staged":   # the last row in the tile's first pair, inside a stripe, at a stripe's edges
        assert {(n - 1) % S.FS_TILE for n in sizes} >= {0, 1, 2, 2046, 2047, 2048, 32766}


# ----------------------------------------------------------------------------- (c) persistence
def test_staged_persistent():
    assert all(math.gcd(len(S.PERSIST_PATTERN), cus) == 1 for cus in (32, 64, 128, 256, 304))
    assert {t <= S.FS_CAP for t in S.PERSIST_PATTERN} == {True, False}
    for ntiles, ragged in ((11, False), (12, True)):
        col, _ = S.staged_persistent(ntiles, ragged)
        m = S.mask_of(col)
        t = S.totals(m, S.FS_TILE)
        full = ntiles - ragged
        assert len(t) == ntiles and t[:full].tolist() == [S.PERSIST_PATTERN[i % 5] for i in range(full)]
        assert len(col) == (ntiles * S.FS_TILE if not ragged else (ntiles - 1) * S.FS_TILE + S.PERSIST_RAGGED)
        out, cnt = S.staged_model(col, word0=1)
        assert cnt == m.sum() and np.array_equal(out[:cnt], col[m]) and np.all(out[cnt:] == S.SENTINEL)


# ----------------------------------------------------------------------------- (d), (e)
def test_varied_tiles_all_differ():
    """Every full tile of `varied` holds a different count (for more tiles than any test
    uses), so any two tiles a persistent workgroup takes in turn differ."""
    ntiles = 2 * 304 + 1
    col, _ = S.varied((ntiles - 1) * S.SEL_TILE + 7)
    m = S.mask_of(col)
    t = S.totals(m, S.SEL_TILE)
    assert len(t) == ntiles and len(set(t[:-1].tolist())) == ntiles - 1
    assert t[:-1].tolist() == [(i * S.STEP + 1) % 16385 for i in range(ntiles - 1)] and t[-1] <= 7
    c = S.sel_counts(m)
    assert c.shape == (ntiles, 32, 8) and c[:-1].max() > 1 and (c[:-1] > 0).sum(axis=(1, 2)).max() == 256
    for n in S.UNSTAGED_N + S.SELECT_N:
        assert len(S.varied(n)[0]) == n
    assert [-(-n // S.FT_TILE) for n in S.UNSTAGED_N[-2:]] == [66, 131]   # walks of two and three steps


def test_select_builders():
    for n in S.SELECT_N:
        for item, wave in S.SELECT_CORNERS:
            c = S.sel_counts(S.mask_of(S.select_item_wave(n, item, wave)[0]))
            rows_there = np.clip(n - (np.arange(len(c)) * S.SEL_TILE + S.sel_row(item, wave, 0)), 0, 64)
            assert c.sum() == c[:, item, wave].sum() and c[:, item, wave].tolist() == rows_there.tolist()
        assert S.mask_of(S.select_const(n, 1)[0]).all() and not S.mask_of(S.select_const(n, 0)[0]).any()
    assert set(S.SELECT_CORNERS) == {(i, w) for i in (0, S.SEL_ITEMS - 1) for w in (0, S.SEL_WAVES - 1)}
    col, _ = S.select_alternating(6)
    assert S.totals(S.mask_of(col), S.SEL_TILE).tolist() == [16384, 0, 16384, 0, 16384, 0, 5]


@pytest.mark.parametrize("grid,ntiles", [(4, 4), (4, 5), (4, 9), (3, 8)])
def test_select_model_equals_reference(grid, ntiles):
    col, _ = S.varied((ntiles - 1) * S.SEL_TILE + 7)
    m = S.mask_of(col)
    ids, cnt = S.select_model(m, grid)
    assert cnt == m.sum() and np.array_equal(ids, np.flatnonzero(m))


# ----------------------------------------------------------------------------- (f) look-back chains
def all_chains():
    out = [(np.zeros(3, dtype=np.uint64), 0, 12345)]
    out += [S.chain(r) for r in S.LB_RUNS] + [S.chain(r, behind=0) for r in S.LB_RUNS]
    out += [S.chain(p, behind=70) for p in range(64)]
    out += [S.chain_no_inclusive(t) for t in (1, 63, 64, 65, 200)]
    out += [S.chain_no_inclusive(64, value=0xFFFFFFFF), S.chain(63, value=0xFFFFFFFF),
            S.chain_no_inclusive(128, value=0xFFFFFFFF)]
    out += [S.chain_one_huge(100, at) for at in (99, 36, 35, 0)]
    return out


def test_chains_hold_what_they_claim():
    for run in S.LB_RUNS:
        for behind in (5, 0, 70):
            st, tile, total = S.chain(run, behind)
            flags = (st >> np.uint64(62)).astype(int)
            assert tile == behind + 1 + run and np.all(flags[behind + 1:tile] == 1) and flags[behind] == 2
            assert np.all(flags[tile:] == 0) and np.all(np.isin(flags[:tile], (1, 2)))    # every predecessor published
            assert set(flags[:behind].tolist()) == ({1, 2} if behind > 1 else ({2} if behind else set()))
            assert np.all((st[:behind] & np.uint64(S.VAL_MASK)) == S.BIG)
            excl, gran = S.lookback_reference(st, tile, total)
            assert excl == int((st[behind:tile] & np.uint64(S.VAL_MASK)).astype(object).sum()) < 1 << 50
            assert gran == S.FLAG_INC | (excl + total)
    for st, tile, total in all_chains():
        assert tile < len(st) and np.all(np.isin((st[:tile] >> np.uint64(62)).astype(int), (1, 2)))
        excl, _ = S.lookback_reference(st, tile, total)
        assert excl + total <= S.VAL_MASK
        assert S.lookback_walk(st, tile, total) == S.lookback_reference(st, tile, total)
    # the carry: 64 x 0xFFFFFFFF needs bit 32 and up; the huge value is the largest a granule holds
    assert S.lookback_reference(*S.chain_no_inclusive(64, value=0xFFFFFFFF))[0] == 64 * 0xFFFFFFFF > 1 << 32
    assert S.lookback_reference(*S.chain_one_huge(100, 35))[0] == (1 << 62) - 1
    # at 36 the huge value is read by the last lane of the first step (99 - 63), at 35 by lane 0 of the second
    assert (99 - 35, 99 - 36) == (64, 63)
