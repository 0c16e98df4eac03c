"""GPU: nut_group_pick (csrc/pick.hip), the per-group row pick behind any /
anyLast / argMin / argMax, against a numpy restatement: sizes around the wave, the workgroup
and the per-workgroup tile, a grid-stride tail, 0..2 key words, groups without rows, rows
without a group, int64 and float64 orders with their extremes, ties, and contention of every
row on one and on five groups.  Every result is exact."""
import numpy as np
import pytest
import torch

from nutdb_amd import Executor, NutError

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
THREADS, TILE = Executor.PICK_THREADS, Executor.PICK_TILE
SIGN = np.uint64(1 << 63)


def order_words(order):
    """the unsigned word whose order is the pick's: int64 with the sign bit flipped, float64
    in the IEEE total order"""
    b = np.ascontiguousarray(order).view(np.uint64)
    if order.dtype == np.int64:
        return b ^ SIGN
    return np.where(b >> np.uint64(63) != 0, ~b, b | SIGN)


def reference(row_keys, order, group_keys, want_max, m):
    """numpy restatement: per group the position of the least (greatest) order word, ties to
    the lowest position; order None: the first (last) position; -1 without rows"""
    nk = len(row_keys)
    ng = len(group_keys[0]) if nk else 1
    if nk == 0:
        g = np.zeros(m, np.int64)
    elif nk == 1:
        i = np.minimum(np.searchsorted(group_keys[0], row_keys[0]), ng - 1)
        g = np.where(group_keys[0][i] == row_keys[0], i, -1).astype(np.int64)
    else:
        gt = np.stack(group_keys, axis=1)
        rt = np.stack(row_keys, axis=1) if m else np.zeros((0, nk), np.int64)
        # rank of every row's tuple among the group tuples (lexicographic, signed)
        allt = np.concatenate([gt, rt])
        _, inv = np.unique(allt, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        slot = np.full(inv.max() + 1 if len(inv) else 0, -1, np.int64)
        slot[inv[:ng]] = np.arange(ng)
        g = slot[inv[ng:]]
    pos = np.arange(m, dtype=np.int64)
    keep = g >= 0
    g, pos = g[keep], pos[keep]
    out = np.full(ng, -1, np.int64)
    if order is None:
        if want_max:
            np.maximum.at(out, g, pos)
        else:
            first = np.full(ng, I64_MAX, np.int64)
            np.minimum.at(first, g, pos)
            out = np.where(first == I64_MAX, -1, first)
        return out
    w = order_words(order)[keep]
    if want_max:
        w = ~w
    idx = np.lexsort((pos, w, g))  # by group, then word, then position
    gs = g[idx]
    firsts = np.ones(len(gs), bool)
    firsts[1:] = gs[1:] != gs[:-1]
    out[gs[firsts]] = pos[idx][firsts]
    return out


def run(ex, row_keys, order, group_keys, want_max, m):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ex.device)
    got = ex.group_pick([dev(k) for k in row_keys], None if order is None else dev(order), [dev(k) for k in group_keys],
                        want_max=want_max, nrows=m)
    assert got.dtype == torch.int64
    return got.cpu().numpy()


def check(ex, row_keys, order, group_keys, m, what="", positions=True):
    for want_max in (False, True):
        want = reference(row_keys, order, group_keys, want_max, m)
        got = run(ex, row_keys, order, group_keys, want_max, m)
        assert np.array_equal(got, want), (what, want_max, np.flatnonzero(got != want)[:5], got[:8], want[:8])
    if order is not None and positions:
        for want_max in (False, True):
            want = reference(row_keys, None, group_keys, want_max, m)
            got = run(ex, row_keys, None, group_keys, want_max, m)
            assert np.array_equal(got, want), (what, "positions", want_max)


def make_groups(rng, nk, ng):
    """ng strictly ascending tuples; word values include both extremes"""
    if nk == 1:
        if ng == 1:
            return [np.array([-3], np.int64)]
        inner = rng.choice(np.arange(-2**20, 2**20, dtype=np.int64), ng - 2, replace=False)
        return [np.sort(np.concatenate([np.array([I64_MIN, I64_MAX], np.int64), inner]))]
    side = max(2, int(np.ceil(np.sqrt(ng))))
    a = np.sort(rng.choice(np.arange(-side, side), side, replace=False)).astype(np.int64)
    a[0], a[-1] = I64_MIN, I64_MAX
    t = np.stack(np.meshgrid(a, a, indexing="ij"), axis=-1).reshape(-1, 2)[:ng]  # equal in word 0, differing in word 1
    return [np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1])]


M_SIZES = [0, 1, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, TILE - 1, TILE, TILE + 1]


@pytest.mark.parametrize("m", M_SIZES)
def test_sizes_no_keys(ex, m):
    rng = np.random.default_rng(m)
    check(ex, [], rng.integers(-5, 5, m), [], m, "i64")
    check(ex, [], rng.integers(-3, 3, m).astype(np.float64), [], m, "f64")


@pytest.mark.parametrize("m", M_SIZES)
@pytest.mark.parametrize("nk", [1, 2])
def test_sizes_few_groups(ex, m, nk):
    rng = np.random.default_rng(100 * nk + m)
    gk = make_groups(rng, nk, 3)
    sel = rng.integers(0, 3, m)
    rk = [k[sel] for k in gk]
    check(ex, rk, rng.integers(-4, 4, m), gk, m)


@pytest.mark.parametrize("nk", [1, 2])
@pytest.mark.parametrize("ng", [1, 2, 3, 1000, 2**17])
def test_group_counts(ex, nk, ng):
    """some groups take no row (-1), some rows carry tuples of no group, the groups at index
    0 and ng - 1 both take rows"""
    rng = np.random.default_rng(7 * ng + nk)
    gk = make_groups(rng, nk, ng)
    ng = len(gk[0])
    m = 3 * TILE + 77 if ng <= 1000 else 2**18 + 5
    live = np.unique(np.concatenate([[0, ng - 1], rng.integers(0, ng, max(1, ng // 2))]))
    sel = live[rng.integers(0, len(live), m)]
    sel[:2] = [ng - 1, 0]
    rk = [k[sel].copy() for k in gk]
    absent = rng.random(m) < 0.2
    absent[:2] = False
    rk[-1][absent] += 1  # a neighbouring tuple: mostly of no group (the reference decides)
    order = rng.integers(-50, 50, m)
    want = reference(rk, order, gk, False, m)
    assert want[0] >= 0 and want[-1] >= 0 and (ng < 1000 or (want == -1).any())
    check(ex, rk, order, gk, m)
    check(ex, rk, rng.choice(np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf]), m), gk, m)


def test_every_row_its_own_group(ex):
    m = 2 * TILE + 3
    k = np.arange(-m // 2, -m // 2 + m, dtype=np.int64)
    perm = np.random.default_rng(5).permutation(m)
    for order in (np.zeros(m, np.int64), None):
        for want_max in (False, True):
            got = run(ex, [k[perm]], order, [k], want_max, m)
            assert np.array_equal(got, np.argsort(perm))


def test_grid_stride_tail(ex):
    m = 2**20 + 3
    rng = np.random.default_rng(20)
    gk = make_groups(rng, 1, 1000)
    sel = rng.integers(0, 1000, m)
    check(ex, [gk[0][sel]], rng.integers(I64_MIN, I64_MAX, m, endpoint=True), gk, m)


def test_i64_order_extremes_and_ties(ex):
    rng = np.random.default_rng(31)
    m = TILE + 130
    gk = make_groups(rng, 1, 5)
    rk = [gk[0][rng.integers(0, 5, m)]]
    # extremes present, several times each: ties only at the extreme
    order = rng.integers(-9, 9, m)
    order[rng.integers(0, m, 40)] = I64_MIN
    order[rng.integers(0, m, 40)] = I64_MAX
    check(ex, rk, order, gk, m, "extremes")
    # all rows tied: the lowest position of every group, both directions
    for c in (0, I64_MIN, I64_MAX):
        tied = np.full(m, c, np.int64)
        for want_max in (False, True):
            got = run(ex, rk, tied, gk, want_max, m)
            first = np.array([np.flatnonzero(rk[0] == g)[0] for g in gk[0]])
            assert np.array_equal(got, first), c


def test_f64_total_order(ex):
    """-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN, by bits"""
    bits = np.array([0xFFFFFFFFFFFFFFFF, 0xFFF8000000000000, 0xFFF0000000000000, 0xBFF0000000000000, 0x8000000000000001,
                     0x8000000000000000, 0x0000000000000000, 0x0000000000000001, 0x3FF0000000000000, 0x7FF0000000000000,
                     0x7FF8000000000000, 0x7FFFFFFFFFFFFFFF], dtype=np.uint64)
    rng = np.random.default_rng(64)
    # one group holding every pattern twice, shuffled: min is the first -NaN row, max the first +NaN row
    order = np.concatenate([bits, bits])[rng.permutation(24)].view(np.float64)
    for want_max, b in ((False, bits[0]), (True, bits[-1])):
        got = run(ex, [], order, [], want_max, 24)
        assert got.tolist() == [int(np.flatnonzero(order.view(np.uint64) == b)[0])]
    # -0.0 against +0.0 only
    z = np.array([0.0, -0.0, 0.0, -0.0]).astype(np.float64)
    assert run(ex, [], z, [], False, 4).tolist() == [1] and run(ex, [], z, [], True, 4).tolist() == [0]
    # many rows, several groups, drawn from the patterns
    m = 5 * TILE + 9
    gk = make_groups(rng, 2, 7)
    sel = rng.integers(0, 7, m)
    check(ex, [k[sel] for k in gk], bits[rng.integers(0, len(bits), m)].view(np.float64), gk, m)


@pytest.mark.parametrize("ng", [1, 5])
def test_contention(ex, ng):
    """2^20 rows into one and into five groups: every lane on the same few words"""
    m = 2**20
    rng = np.random.default_rng(ng)
    gk = [np.arange(ng, dtype=np.int64) * 3 - 4]
    rk = [gk[0][rng.integers(0, ng, m)]]
    check(ex, rk, rng.integers(-1000, 1000, m), gk, m, "random")
    check(ex, rk, np.arange(m, dtype=np.int64), gk, m, "ascending", False)   # every row improves a maximum
    check(ex, rk, -np.arange(m, dtype=np.int64), gk, m, "descending", False)  # every row improves a minimum
    check(ex, rk, np.full(m, 7.0), gk, m, "constant", False)


def test_argument_errors(ex):
    import ctypes as C

    from nutdb_amd._lib import check as chk, lib
    k = torch.zeros(4, dtype=torch.int64, device=ex.device)
    out = torch.zeros(2, dtype=torch.int64, device=ex.device)
    ptr = (C.c_void_p * 1)(k.data_ptr())

    def call(keys, nkeys, ng):
        chk(lib.nut_group_pick(ex.ctx, keys, nkeys, 4, C.c_void_p(k.data_ptr()), 0, 0, keys, ng, C.c_void_p(out.data_ptr())),
            "nut_group_pick")
    with pytest.raises(NutError) as e:  # no keys: one group
        call(None, 0, 2)
    assert e.value.status == 1
    with pytest.raises(NutError) as e:  # three key words
        call(ptr, 3, 2)
    assert e.value.status == 1
    with pytest.raises(NutError) as e:  # 2^32 groups: refused before anything is read
        call(ptr, 1, 2**32)
    assert e.value.status == 4
