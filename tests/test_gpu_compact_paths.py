"""Every branch of the order-preserving compaction kernels — filter_i64_staged_kernel and
filter_i64_kernel (csrc/filter.hip), select_kernel (csrc/select_kernel.hpp) — and of the
decoupled look-back (csrc/lookback.hpp) on directed inputs, bit-exact against numpy
(col[mask], np.flatnonzero(mask)) and the C oracle (oracle.filter_i64).

tests/compact_shapes.py builds the inputs from the kernels' tile geometry and
tests/test_compact_shapes_cpu.py proves (no GPU) that they hold what they claim: tile
totals exactly at 20223 / 20224 / 20225 rows, every parity of `half` and `total - half`,
a wave of 128 selected rows (in-wave rank 126), single stripes, lanes and pair halves, the
last rows of a ragged tile selected every way, persistent workgroups whose tiles in turn
differ, and look-back chains of chosen length with the inclusive granule in a chosen lane.
DESIGN.md §4.5 maps each kernel branch to its case.

Every filter case writes into a guarded buffer at both 16-byte parities of the output
base: the word before the output and every word from `count` on keep their sentinel."""
import numpy as np
import pytest
import torch

import compact_shapes as S
from helpers import OPCODE
from test_gpu_exec import dev

pytestmark = pytest.mark.gpu

NUT_ERR_INVALID_ARG = 1
GE0 = [("col", 0), ("i64", 0, 0), ("ge",)]


def guarded_filter(ex, orc, col, note, op=">=", k=0, unaligned=False, oracle=True):
    """col <op> k through nut_filter_i64 with the output at buf[1:] and at buf[2:]."""
    col = np.array(col, dtype=np.int64)   # a writable copy: the builders' cached columns are read-only
    n = len(col)
    want = col[S.apply_op(col, op, k)]
    if oracle:
        assert np.array_equal(orc.filter_i64(col, OPCODE[op], k), want), note
    if unaligned:   # a slice 8 bytes off 16-byte alignment: filter_i64_kernel<ALIGNED = false>
        d = dev(np.concatenate([np.zeros(1, dtype=np.int64), col]), ex)[1:]
        assert d.data_ptr() % 16 == 8
    else:
        d = dev(col, ex)
        assert d.data_ptr() % 16 == 0
    want_d = dev(want, ex)
    for off in (1, 2):
        buf = torch.full((n + 4,), S.SENTINEL, dtype=torch.int64, device=ex.device)
        assert buf.data_ptr() % 16 == 0
        got = ex.filter_i64(d, op, k, out=buf[off:])
        cnt = got.numel()
        assert cnt == len(want), f"{note}: output at +{off}: count {cnt}, want {len(want)}"
        assert bool((buf[:off] == S.SENTINEL).all()), f"{note}: output at +{off}: the word before the output"
        assert bool((buf[off + cnt:] == S.SENTINEL).all()), f"{note}: output at +{off}: written behind count"
        if not torch.equal(buf[off:off + cnt], want_d):
            bad = int(torch.nonzero(buf[off:off + cnt] != want_d)[0])
            raise AssertionError(f"{note}: output at +{off}: row {bad} is {int(buf[off + bad])}, want {int(want[bad])}")


# ----------------------------------------------------------------------------- (a) staged kernel, one shaped tile
@pytest.mark.parametrize("name", S.STAGED_SHAPES)
def test_staged_shaped_tile(ex, orc, name):
    """One tile of a chosen shape: alone (n = 32768), and as the middle one of three behind
    an odd and an even count (the flush offset's two parities).  total:* = the `fits`
    threshold (20224 fits, 20225 goes in two halves) and cnt 0..3 in flush_staged;
    dense:h:r = the parities of half and total - half; wave:s:w = in-wave rank 126;
    stripe:s, lane:l, parity:p = one stripe, one lane of every wave, one row of every pair."""
    guarded_filter(ex, orc, *S.one_tile("staged", name))
    for prev_odd in (True, False):
        guarded_filter(ex, orc, *S.three_tiles("staged", name, prev_odd))


# ----------------------------------------------------------------------------- (b) staged kernel, last-tile edges
@pytest.mark.parametrize("n", S.STAGED_EDGE_N)
def test_staged_last_rows(ex, orc, n):
    """The clamped loads of the last tile: all eight selections of the last three rows.
    Odd n: the pair holding row n - 1 loads (n - 2, n - 1) and takes the upper half — rows
    n - 2 and n - 1 selected differently, both ways round, tell the halves apart.  Even n:
    both last rows selected, and the clamped lanes behind them must not repeat them."""
    for bits in range(8):
        guarded_filter(ex, orc, *S.last_rows(n, bits))


# ----------------------------------------------------------------------------- (c) staged kernel, persistence
@pytest.mark.parametrize("which", ["cus", "cus+1", "2cus+1"])
def test_staged_persistent_tiles(ex, orc, which):
    """More tiles than workgroups (one per CU): a workgroup's tiles in turn hold 0, 1,
    20224, 20225 and 32768 rows, so it switches between the `fits` path and the two-halves
    path with the next tile's loads in flight; 2 cus + 1: the last tile ragged."""
    cus = ex.info()["num_cus"]
    ntiles = {"cus": cus, "cus+1": cus + 1, "2cus+1": 2 * cus + 1}[which]
    col, note = S.staged_persistent(ntiles, ragged=which == "2cus+1")
    assert -(-len(col) // S.FS_TILE) == ntiles and (which == "cus") == (ntiles <= cus)
    guarded_filter(ex, orc, col, note, oracle=False)


# ----------------------------------------------------------------------------- (d) unstaged kernel
@pytest.mark.parametrize("n", S.UNSTAGED_N)
def test_unstaged_sizes(ex, orc, n):
    """filter_i64_kernel on a column 8 bytes off 16-byte alignment: the ragged last tile
    around 16384 rows, and 66 and 131 tiles — look-back walks of two and three steps."""
    guarded_filter(ex, orc, *S.varied(n), unaligned=True)
    for bits in (range(8) if n <= 16385 else (1, 2, 5)):
        guarded_filter(ex, orc, *S.last_rows(n, bits), unaligned=True)


def test_unstaged_aligned_single_row(ex, orc):
    """n = 1 on an aligned column: the only caller of filter_i64_kernel<ALIGNED = true>."""
    for v in (0, -1):
        guarded_filter(ex, orc, np.array([v], dtype=np.int64), f"aligned n = 1, value {v}")


@pytest.mark.parametrize("name", S.UNSTAGED_SHAPES)
def test_unstaged_shaped_tile(ex, orc, name):
    guarded_filter(ex, orc, *S.one_tile("unstaged", name), unaligned=True)
    guarded_filter(ex, orc, *S.three_tiles("unstaged", name, True), unaligned=True)


@pytest.mark.parametrize("kind", ["staged", "unstaged"])
def test_six_operators(ex, orc, kind):
    """One mask under all six operators (two tiles, the second ragged and odd)."""
    n = S.PAIR[kind][0] + 4097
    mask = S.mask_of(S.varied(n)[0])
    for op in S.OPS:
        col, k = S.column_op(mask, op)
        assert np.array_equal(S.apply_op(col, op, k), mask)
        guarded_filter(ex, orc, col, f"{kind}, {op} {k}", op=op, k=k, unaligned=kind == "unstaged")


# ----------------------------------------------------------------------------- (e) select_kernel
def select(ex, cols, where=GE0):
    return ex.select_rows([dev(c, ex) for c in cols], where).cpu().numpy()


def check_select(ex, col, note):
    got = select(ex, [col])
    want = np.flatnonzero(S.mask_of(col))
    assert len(got) == len(want), f"{note}: count {len(got)}, want {len(want)}"
    assert np.array_equal(got, want), f"{note}: first wrong id at {int(np.flatnonzero(got != want)[0])}"


@pytest.mark.parametrize("n", S.SELECT_N)
def test_select_tile_edges(ex, n):
    """One tile short of, exactly and one row past 16384: rows only in item i of wave w at
    the four corners of 32 x 8, all rows, no rows, and a scattered selection."""
    for item, wave in S.SELECT_CORNERS:
        check_select(ex, *S.select_item_wave(n, item, wave))
    for value in (1, 0):
        check_select(ex, *S.select_const(n, value))
    check_select(ex, *S.varied(n))


def test_select_alternating_tiles(ex):
    check_select(ex, *S.select_alternating(6))


@pytest.mark.parametrize("which", ["cus", "cus+1", "2cus+1"])
def test_select_persistent_tiles(ex, opts, which):
    """sel_blocks = 1: one workgroup per CU.  2 cus + 1 tiles (+ 7 rows): every workgroup
    evaluates at least two tiles, so both s_cnt buffers, sel_next and the flip of b run;
    every tile holds a different count, so counts read from the wrong buffer show.  At
    that shape also an int8 column (load_row_typed) and a two-column `and`."""
    cus = ex.info()["num_cus"]
    sel_blocks = 1
    opts(sel_blocks=sel_blocks)
    ntiles = {"cus": cus, "cus+1": cus + 1, "2cus+1": 2 * cus + 1}[which]
    n = ntiles * S.SEL_TILE if which != "2cus+1" else (ntiles - 1) * S.SEL_TILE + 7
    col, note = S.varied(n)
    assert -(-n // S.SEL_TILE) == ntiles
    if which != "cus":
        assert ntiles > cus * sel_blocks, "every workgroup would take one tile only"
    check_select(ex, col, note)
    if which == "2cus+1":
        assert ntiles >= 2 * cus * sel_blocks
        mask = S.mask_of(col)
        got = select(ex, [np.where(mask, 1, -1).astype(np.int8)])
        assert np.array_equal(got, np.flatnonzero(mask)), f"{note}: int8 column"
        other = np.arange(n) % 3 != 0
        got = select(ex, [col, S.column(other)], GE0 + [("col", 1), ("i64", 0, 0), ("ge",), ("and",)])
        assert np.array_equal(got, np.flatnonzero(mask & other)), f"{note}: two columns"


# ----------------------------------------------------------------------------- (f) look-back on constructed chains
def check_chain(ex, status, tile, total, note):
    want = S.lookback_reference(status, tile, total)
    got = ex.lookback_probe(status, tile, total)
    assert got == want, f"{note}: (excl, granule) = ({got[0]:#x}, {got[1]:#x}), want ({want[0]:#x}, {want[1]:#x})"


def test_lookback_tile_0(ex):
    check_chain(ex, np.zeros(3, dtype=np.uint64), 0, 12345, "tile 0")
    assert ex.lookback_probe(np.zeros(1, dtype=np.uint64), 0, 7) == (0, S.FLAG_INC | 7)


@pytest.mark.parametrize("run", S.LB_RUNS)
def test_lookback_runs(ex, run):
    """`run` aggregate granules, then an inclusive one, then older granules of 2^61 under
    both flags: runs of 64 and more need the second and third 64-tile step, and nothing
    behind the inclusive granule may be counted."""
    check_chain(ex, *S.chain(run), f"run {run}")
    check_chain(ex, *S.chain(run, behind=0), f"run {run}, the inclusive granule at index 0")


def test_lookback_inclusive_in_every_lane(ex):
    """The first inclusive granule in lane p of the first step, p = 0..63, with 70 older
    granules behind it: the lanes above p hold 2^61 and are masked out (lane <= first)."""
    for p in range(64):
        check_chain(ex, *S.chain(p, behind=70), f"inclusive in lane {p}")


@pytest.mark.parametrize("tile", [1, 63, 64, 65, 200])
def test_lookback_runs_off_index_0(ex, tile):
    check_chain(ex, *S.chain_no_inclusive(tile), f"{tile} aggregates, no inclusive")


def test_lookback_carries(ex):
    """wave_sum_u64 across the 32-bit halves: 0xFFFFFFFF in all 64 lanes; one value of
    2^62 - 1 in the first, the last and a middle lane of a step."""
    check_chain(ex, *S.chain_no_inclusive(64, value=0xFFFFFFFF), "64 x 0xFFFFFFFF")
    check_chain(ex, *S.chain(63, value=0xFFFFFFFF), "63 x 0xFFFFFFFF and an inclusive one")
    check_chain(ex, *S.chain_no_inclusive(128, value=0xFFFFFFFF), "128 x 0xFFFFFFFF")
    for at in (99, 36, 35, 0):
        check_chain(ex, *S.chain_one_huge(100, at), f"2^62 - 1 at {at}")


def test_lookback_probe_refuses(ex):
    """A predecessor without a flag would make the walk wait, so it is refused before
    anything is launched; so is a tile outside the granules."""
    from nutdb_amd import NutError
    st, tile, total = S.chain(10)
    for bad in (0, 5, tile - 1):
        s = st.copy()
        s[bad] &= np.uint64(S.VAL_MASK)
        with pytest.raises(NutError) as e:
            ex.lookback_probe(s, tile, total)
        assert e.value.status == NUT_ERR_INVALID_ARG
    for t in (len(st), len(st) + 5):
        with pytest.raises(NutError) as e:
            ex.lookback_probe(st, t, total)
        assert e.value.status == NUT_ERR_INVALID_ARG
    check_chain(ex, st, tile, total, "the chain the refusals were cut from")
