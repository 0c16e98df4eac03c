"""Every branch of the sort kernels on directed small inputs (msd_sort.hip, sort.hip,
topk.hip), bit-exact against numpy on the host.

tests/sort_shapes.py builds the inputs and tests/test_sort_shapes_cpu.py proves, with a
host model of the local sort's window rule, that they hold the window sizes they claim:
every size 1..128 in every size class (lane, half-wave, 64- and 128-key networks), both LDS
rounds of the L class, and a window over 128 keys (ms_lsd_kernel) in every class.  Where
the ABI reports the path (nut_ctx_sort_stats: algorithmic bytes and scatter levels) the
tests assert it; the expected figures are derived from msd_sort_i64 / device_level here.
DESIGN.md §4.3 maps each branch to its test.  Nothing exceeds 262 145 keys per call except
the one status-array growth call of the epoch test."""
import ctypes as C

import numpy as np
import pytest
import torch

import sort_shapes as S
from helpers import dev, sort_pairs, topk_positions, ukey

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = S.I64_MIN, S.I64_MAX
NUT_ERR_INVALID_ARG, NUT_ERR_CAPACITY = 1, 5


def host(t):
    return t.cpu().numpy()


def check_sort(ex, keys, desc, sliced=False, what=""):
    """ex.sort_i64 against np.sort; `sliced`: the column is a [1:] slice, so its base is
    8-byte but not 16-byte aligned.  Returns sort_stats()."""
    if sliced:
        d = dev(np.concatenate([np.zeros(1, np.int64), keys]), ex)[1:]
        assert d.data_ptr() % 16 == 8
    else:
        d = dev(keys, ex)
    got = host(ex.sort_i64(d, descending=desc))
    stats = ex.sort_stats()
    want = np.sort(keys)
    want = want[::-1] if desc else want
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, desc, sliced, len(keys), len(bad), bad[:4], got[bad[:4]], want[bad[:4]])
    return stats


def check_cases(ex, cases, single_segment):
    for i, c in enumerate(cases):
        for desc in ((False, True) if c.desc is None else (c.desc,)):
            stats = check_sort(ex, c.keys, desc, sliced=(i == 0), what=c.name)
            if single_segment:  # one local-sort segment over all 64 bits: read once, written once
                assert stats == (16 * len(c.keys), 0), (c.name, stats)


# ----------------------------------------------------------------------------- keys only, one segment
@pytest.mark.parametrize("variant", S.NETWORK_VARIANTS)
@pytest.mark.parametrize("cls", list(S.CLASSES))
def test_sort_window_networks(ex, cls, variant):
    """Windows of every size 1..128 in class `cls`, none larger: the lane network (2-16
    keys), the half-wave bitonic network (17-32) and sort_window's 64- and 128-key networks,
    with distinct keys, with duplicates, and with u = 0 / all ones (INT64_MIN / INT64_MAX: the
    networks' padding value) among the keys."""
    check_cases(ex, S.network_inputs(cls, variant), True)


def test_sort_two_lds_rounds(ex):
    """L class above 16384 keys: round 0 in LDS, round 1 parked in `out` and brought back;
    a window start exactly at 16384, a 100-key window across it, n = 16385 and 24576."""
    check_cases(ex, S.two_round_inputs(), True)


@pytest.mark.parametrize("cls", list(S.CLASSES))
def test_sort_lsd_fallback_single_segment(ex, cls):
    """A window over 128 keys sends the segment to ms_lsd_kernel<THREADS, MAXK> of its
    class: constant and two-valued columns, one 129-key window in sparse data, 129-key runs
    of INT64_MAX / INT64_MIN (x = key - min = all ones = the padding, which must stay behind
    the real keys), at the class edges and at sizes that leave padded positions."""
    check_cases(ex, S.fallback_inputs(cls), True)


def test_sort_one_and_two_keys(ex):
    check_cases(ex, S.tiny_inputs(), True)


# ----------------------------------------------------------------------------- keys only, several levels
@pytest.mark.parametrize("n", S.NARROW_N)
@pytest.mark.parametrize("hb", S.NARROW_HB)
def test_sort_narrow_ranges(ex, hb, n):
    """Keys in base + [0, 2^hb) above one local sort.  msd_sort_i64: the first histogram
    (8 B/key) finds the top digit nearly constant and is redone (8 B/key) with base = min and
    the digit at bits [hb - w, hb), w = min(9, hb); that one scatter level (16 B/key) leaves
    sub-segments with hi = hb - w varying bits: hi = 0 (hb <= 9) are runs of equal keys for
    ms_copy_kernel, hi = 1, 2, 3 (hb = 10, 11, 12) local sorts with fewer varying bits than
    bucket bits (2, 4, 8 buckets used), all with the rebased nonzero base.  None exceeds a
    local sort (n / 512 keys on average), so no further level runs: 16 B/key more, in all
    48 B/key and ONE level, for every hb here.  At n = 200 000 and hb = 10 each sub-segment
    holds 2 values of ~195 keys: the LSD fallback with hi = 1."""
    for i, (name, base) in enumerate(S.narrow_bases(hb).items()):
        keys = S.narrow_range(hb, base, n)
        for desc in (False, True):
            stats = check_sort(ex, keys, desc, sliced=(i == 1 and desc), what=f"narrow-{hb}-{name}")
            assert stats == (48 * n, 1), (hb, name, n, desc, stats)


def model_levels(u):
    """(bytes, levels) of msd_sort_i64's exact layout for order-mapped keys `u` whose top
    digit spreads over the range (no rebase), restated from the host code: level 1 (host
    planned) takes bits [55, 64), every further level (device_level) the 9 bits below, the
    last ones bits [1, 10) and then bit 0 alone; a level histograms (8 B/key) and scatters
    (16 B/key) every key of the segments it was given, and hands on only the sub-segments
    of more than 24576 keys; every key is finally written once by a local sort or a copy
    (16 B/key).  After bit 0 the remaining segments are runs of one value: copied."""
    nbytes, levels, segs = 16 * len(u), 0, [u]
    for shift, bits in [(55, 9), (46, 9), (37, 9), (28, 9), (19, 9), (10, 9), (1, 9), (0, 1)]:
        if not segs:
            break
        levels += 1
        nbytes += 24 * sum(len(s) for s in segs)
        nxt = []
        for s in segs:
            d = ((s >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.int64)
            nxt += [s[d == v] for v in np.flatnonzero(np.bincount(d) > S.LS_CAP)]
        segs = nxt
    return nbytes, levels


@pytest.mark.parametrize("w", S.CLUSTER_W)
def test_sort_clusters_device_planned_levels(ex, w):
    """60 000 keys, half of them in [2^50, 2^50 + 2^w): the cluster (30 000 keys > one local
    sort) shares its top 9 bits, so after level 1 it is the one segment handed to the
    device-planned levels (device_level, ms_plan_kernel).  Its keys agree on bits >= w, so
    the levels at bits [46, 55), [37, 46), ... are pass-through levels (one digit value, the
    whole segment handed on) until a digit reaches below bit w:
      w = 40: [46, 55) constant, [37, 46) splits on bits 37-39 into 8 x 3750 keys  -> 3 levels
      w = 20: [46, 55), [37, 46), [28, 37) constant, [19, 28) splits on bit 19     -> 5 levels
      w = 0 : one value: constant at [46,55) [37,46) [28,37) [19,28) [10,19) [1,10) and at
              bit 0 alone, then no bit is left and the run is copied               -> 8 levels
    The bytes follow from the keys each level held (model_levels)."""
    keys = S.cluster(w)
    for desc in (False, True):
        want = model_levels(S.umap(keys, desc))
        assert want[1] == {40: 3, 20: 5, 0: 8}[w]
        stats = check_sort(ex, keys, desc, sliced=desc, what=f"cluster-{w}")
        assert stats == want, (w, desc, stats, want)


def test_sort_tile_edges(ex):
    """+-1 around the scatter tile (2 x 14336 keys; 28672 and 57344), the histogram tile
    (2^18) and, with constant and two-valued keys that end in ms_copy_kernel, the copy tile
    (2^16).  Full-range keys: one level, 512 sub-segments for the local sorts (40 B/key);
    constant keys: one histogram, then the copy (24 B/key, no level); two values: the
    rebased one-bit digit splits them into two runs of equal keys, both copied (48 B/key)."""
    for i, c in enumerate(S.tile_edge_inputs()):
        n = len(c.keys)
        for desc in (False, True):
            stats = check_sort(ex, c.keys, desc, sliced=(i == 0), what=c.name)
            want = (40 * n, 1) if "full" in c.name else (24 * n, 0) if "const" in c.name else (48 * n, 1)
            assert stats == want, (c.name, desc, stats)
            if "full" in c.name:
                assert model_levels(S.umap(c.keys, desc)) == want


# ----------------------------------------------------------------------------- nut_sort_pairs
def check_pairs(ex, keys, desc, vals, np_expected=None, what=""):
    got = sort_pairs(ex, keys, desc, vals)
    order = np.argsort(ukey(keys, desc), kind="stable")
    want = order if vals is None else vals[order]
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, desc, vals is not None, len(bad), bad[:4], got[bad[:4]], want[bad[:4]])
    if np_expected is not None:
        assert ex.sort_stats()[1] == np_expected, (what, ex.sort_stats())


@pytest.mark.parametrize("n", [2, 63, 64, 65, 8191, 16383, 16384, 16385, 24577])
def test_sort_pairs_small_sizes_with_payload(ex, n):
    """Tile (8192) and wave edges of the look-back LSD passes: full-range keys (8 passes), an
    explicit random payload, both directions."""
    rng = np.random.default_rng(n)
    keys = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    keys[:2] = [I64_MAX, I64_MIN]
    vals = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64)
    for desc in (False, True):
        check_pairs(ex, keys, desc, vals, what=f"pairs-{n}")


@pytest.mark.parametrize("m", list(S.BYTE_SETS))
def test_sort_pairs_pass_count_and_payload_parity(ex, m):
    """Keys in which exactly m of the 8 bytes vary: nut_sort_pairs skips the constant bytes
    and executes m passes (sort_stats()[1]), and the payload ping-pong must land the LAST
    pass in vals_out for every m, odd and even.  With and without a payload, both
    directions, int64 and (one byte set per m) float64."""
    rng = np.random.default_rng(m)
    vals = rng.integers(I64_MIN, I64_MAX, S.BYTE_MASK_N, dtype=np.int64)
    for j, varying in enumerate(S.BYTE_SETS[m]):
        for f64 in ((False, True) if j == 0 else (False,)):
            keys = S.byte_mask_keys(varying, f64)
            for desc in (False, True):
                for v in (None, vals):
                    check_pairs(ex, keys, desc, v, np_expected=m, what=f"mask-{varying}-{'f64' if f64 else 'i64'}")


def test_lookback_status_epoch_wrap():
    """The look-back status array is reused across calls under an 8-bit pass epoch and is
    cleared when it is (re)allocated, when a call needs more than was cleared, and when the
    epoch reaches 255 (next_status).  A fresh context runs eight-pass sorts of 3 x 8192 + 1
    keys (4 tiles, so later tiles look back), a partition (one more epoch) after every fifth
    sort.  Every clearing restarts the epoch, so the growth call must come AFTER a wrap to
    see both: calls 0-35 execute 288 + 7 epochs (the wrap falls inside call 31), call 36
    sorts 40 x 8192 + 5 keys, which outgrows the cleared array (cleared again, epoch
    restarted), and calls 37-71 cross the wrap once more on the grown array, where the
    small sorts use its first 4 tiles only.  Every call sorts different keys, so a stale
    granule of an earlier round of epochs would give a wrong prefix."""
    from nutdb_amd import Executor
    e = Executor(0)
    try:
        n = 3 * 8192 + 1
        rng = np.random.default_rng(255)
        spl = np.sort(rng.integers(I64_MIN, I64_MAX, 5, dtype=np.int64))
        for call in range(72):
            nn = 40 * 8192 + 5 if call == 36 else n
            keys = rng.integers(I64_MIN, I64_MAX, nn, dtype=np.int64, endpoint=True)
            vals = rng.integers(I64_MIN, I64_MAX, nn, dtype=np.int64)
            desc = bool(call & 1)
            check_pairs(e, keys, desc, vals if call % 3 else None, np_expected=8, what=f"epoch-call-{call}")
            if call % 5 == 4:
                got, counts = e.partition_i64(dev(keys, e), spl)
                b = np.searchsorted(spl, keys, side="right")
                assert counts == [int(c) for c in np.bincount(b, minlength=6)], call
                assert np.array_equal(host(got), keys[np.argsort(b, kind="stable")]), call
    finally:
        e.close()


# ----------------------------------------------------------------------------- nut_partition_i64
def check_partition(ex, keys, spl, what):
    got, counts = ex.partition_i64(dev(keys, ex), spl)
    b = np.searchsorted(spl, keys, side="right")
    assert counts == [int(c) for c in np.bincount(b, minlength=len(spl) + 1)], what
    assert np.array_equal(host(got), keys[np.argsort(b, kind="stable")]), what


@pytest.mark.parametrize("nsplit", [0, 1, 62, 63])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 8191, 8192, 8193, 16385])
def test_partition_small_sizes(ex, n, nsplit):
    """Stable bucket partition at the wave and tile edges: keys of few values plus
    INT64_MIN / INT64_MAX, splitters equal to keys, repeated splitters (empty buckets), and
    INT64_MIN / INT64_MAX as splitters; counts and the stable order against numpy."""
    rng = np.random.default_rng([n, nsplit])
    keys = rng.integers(-40, 40, n).astype(np.int64)
    keys[::7] = rng.choice(np.array([I64_MIN, I64_MAX], dtype=np.int64), len(keys[::7]))
    if nsplit == 0:
        spls = [np.zeros(0, np.int64)]
    elif nsplit == 1:
        spls = [np.array([x], dtype=np.int64) for x in (I64_MIN, I64_MAX, int(keys[n // 2]), 0)]
    else:
        pool = np.concatenate([np.arange(-40, 40, dtype=np.int64), [I64_MIN, I64_MAX]])
        a = np.sort(rng.choice(pool, nsplit))          # with repeats, equal to keys
        b = a.copy()
        b[0], b[1], b[-2], b[-1] = I64_MIN, I64_MIN, I64_MAX, I64_MAX
        spls = [a, b, np.full(nsplit, 3, dtype=np.int64)]
    for j, spl in enumerate(spls):
        check_partition(ex, keys, spl, (n, nsplit, j))


# ----------------------------------------------------------------------------- nut_topk_positions
def check_topk(ex, keys, k, desc, what):
    """The contract (as test_gpu_order_by.py::test_topk_positions): ascending positions of a
    prefix of the order that holds at least min(k, n) keys and every tie of the k-th."""
    n = len(keys)
    u = ukey(keys, desc)
    st, cnt, pos = topk_positions(ex, keys, k, desc)
    assert st == 0, (what, k, st)
    if k == 0:
        assert cnt == 0
        return
    kth = np.sort(u)[min(k, n) - 1]
    assert cnt >= min(k, n) and len(pos) == cnt and np.all(np.diff(pos) > 0), (what, k, cnt)
    assert int((u <= kth).sum()) <= cnt, (what, k)
    assert np.array_equal(pos, np.flatnonzero(u <= u[pos].max())), (what, k)
    if k >= n:
        assert np.array_equal(pos, np.arange(n)), (what, k)


def topk_columns(n, rng):
    f = rng.standard_normal(n)
    f[::5] = rng.choice(np.array([-0.0, 0.0, np.inf, -np.inf, np.nan]), len(f[::5]))
    full = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    full[::9] = rng.choice(np.array([I64_MIN, I64_MAX], dtype=np.int64), len(full[::9]))
    return {"full": full, "ties": rng.integers(-5, 5, n).astype(np.int64), "f64": f}


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_topk_small_sizes(ex, n):
    """The clamped unrolled loads (4 x 256 keys per block step), the per-wave tail of the
    collection and the k >= n branch at n = 1 and around 64, 256 and 1024."""
    for kind, keys in topk_columns(n, np.random.default_rng(n)).items():
        for desc in (False, True):
            for k in (1, n - 1, n, n + 1):
                check_topk(ex, keys, k, desc, (kind, n, desc))


@pytest.mark.parametrize("kind", ["pm512", "low4", "full", "f64_pm512", "f64_low4"])
def test_topk_multi_level_descent(ex, kind):
    """n = 70 001 > the 65 536 candidates at which the descent stops.  Keys in [-512, 512)
    split on the sign at the first level; keys in [0, 16) (float64: 16 neighbouring values)
    share every digit above the last, so the descent goes 64 -> 52 -> 40 -> 28 -> 16 -> 4 -> 0
    and ends at shift 0 with a 4-bit digit; one full-range column stops at the first level."""
    n = 70_001
    rng = np.random.default_rng(70)
    keys = {"pm512": lambda: rng.integers(-512, 512, n).astype(np.int64),
            "low4": lambda: rng.integers(0, 16, n).astype(np.int64),
            "full": lambda: rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True),
            "f64_pm512": lambda: rng.integers(-512, 512, n).astype(np.float64),
            "f64_low4": lambda: (np.float64(1.0).view(np.uint64) + rng.integers(0, 16, n).astype(np.uint64)).view(np.float64),
            }[kind]()
    for desc in (False, True):
        for k in (1, 1000, 20_000, n - 1, n, n + 1):
            check_topk(ex, keys, k, desc, (kind, desc))


SENTINEL = -0x0123456789ABCDEF


def topk_raw(ex, keys, k, desc, out, cap):
    from nutdb_amd._lib import T_F64, T_I64, lib
    d = dev(keys, ex)
    cnt = C.c_uint64()
    ex._bind_stream()
    st = lib.nut_topk_positions(ex.ctx, C.c_void_p(d.data_ptr()), T_F64 if keys.dtype == np.float64 else T_I64,
                                int(desc), len(keys), k, C.c_void_p(out.data_ptr()) if out is not None else None, cap,
                                C.byref(cnt))
    ex.sync()
    return st, cnt.value


@pytest.mark.parametrize("desc", [False, True])
def test_topk_capacity_leaves_the_buffer_untouched(ex, desc):
    """cap = count succeeds; cap = count - 1 returns NUT_ERR_CAPACITY with the count needed
    and every position slot untouched; so does the k >= n branch with cap < n."""
    rng = np.random.default_rng(4097)
    n = 4097
    keys = rng.integers(-50, 50, n).astype(np.int64)
    st, count, pos = topk_positions(ex, keys, 100, desc)
    assert st == 0 and count >= 100
    buf = torch.full((count + 8,), SENTINEL, dtype=torch.int64, device=ex.device)
    assert topk_raw(ex, keys, 100, desc, buf, count) == (0, count)
    assert np.array_equal(host(buf[:count]), pos) and np.all(host(buf[count:]) == SENTINEL)
    buf.fill_(SENTINEL)
    assert topk_raw(ex, keys, 100, desc, buf, count - 1) == (NUT_ERR_CAPACITY, count)
    assert np.all(host(buf) == SENTINEL)
    for k in (n, n + 1):
        assert topk_raw(ex, keys, k, desc, buf, n - 1) == (NUT_ERR_CAPACITY, n)
        assert np.all(host(buf) == SENTINEL)
        big = torch.full((n + 8,), SENTINEL, dtype=torch.int64, device=ex.device)
        assert topk_raw(ex, keys, k, desc, big, n) == (0, n)
        assert np.array_equal(host(big[:n]), np.arange(n)) and np.all(host(big[n:]) == SENTINEL)


def test_topk_null_output_leaves_the_kernel_timer_alone():
    """nut_topk_positions with k >= n and a NULL output is an argument error.  That path
    begins no timed kernel, so it must not end one either: ending would record the end
    event of the context's previous timed kernel again, after whatever ran since.  Here a
    1000-key sort (one workgroup) is followed by fills that write 64 GiB, which take at
    least 8 ms at the HBM's 8 TB/s peak; the sort's reported time must stay its own (far
    below 2 ms)."""
    from nutdb_amd import Executor
    e = Executor(0)
    try:
        keys = np.random.default_rng(1).integers(I64_MIN, I64_MAX, 1000, dtype=np.int64)
        d = dev(keys, e)
        e.sort_i64(d)  # untimed: scratch allocation and the first launch's code load
        e.sync()
        e.enable_timing(True)
        e.sort_i64(d)
        x = torch.empty(1 << 27, dtype=torch.int64, device=e.device)  # 1 GiB
        for i in range(64):
            x.fill_(i)
        st, cnt = topk_raw(e, keys, len(keys), False, None, len(keys))
        assert (st, cnt) == (NUT_ERR_INVALID_ARG, len(keys))
        ms, launches = e.kernel_time(2)  # NUT_KERNEL_SORT
        assert launches == 1 and 0 < ms < 2.0, (ms, launches)
    finally:
        e.close()
