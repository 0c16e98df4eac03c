"""The inputs of tests/sort_shapes.py hold what they claim (no GPU): every builder is run
through the host model of the local sort's window rule, so that test_gpu_sort_paths.py is
known to reach the half-wave and wave-wide networks, both LDS rounds and the LSD fallback
in every size class, not merely hoped to."""
import numpy as np
import pytest

import sort_shapes as S
from helpers import ukey


def test_model_on_a_hand_computed_layout():
    """S class (SB 9, WS 12): buckets of 5, 20, 1, 1, 9 keys start at 0, 5, 25, 26, 27 and end
    at 36.  Window 1 starts at the first bucket start >= 12 (25), window 2 at the first >= 24
    (25 again: empty), and the last window ends at n: sizes 25 and 11."""
    rng = np.random.default_rng(0)
    for desc in (False, True):
        keys = S._keys_from_buckets([5, 20, 1, 1, 9], 9, rng, "plain", desc)
        assert list(S.window_starts(keys, desc)) == [0, 25, 25, 36]
        assert list(S.window_sizes(keys, desc)) == [25, 11]
        assert not S.takes_fallback(keys, desc)
    # the other direction reverses the buckets (9, 1, 1, 20, 5): starts 0, 9, 10, 11, 31
    assert list(S.window_starts(keys, False)) == [0, 31, 31, 36]


@pytest.mark.parametrize("variant", S.NETWORK_VARIANTS)
@pytest.mark.parametrize("cls", list(S.CLASSES))
def test_network_inputs_hold_every_window_size(cls, variant):
    lo, hi, _, _ = S.CLASSES[cls]
    seen = {False: set(), True: set()}
    cases = S.network_inputs(cls, variant)
    assert len(cases) == 2 * {"S": 6, "M": 2, "M2": 2, "L": 1}[cls]
    for c in cases:
        assert lo <= len(c.keys) <= hi and S.class_of(len(c.keys)) == cls, c.name
        sizes = S.window_sizes(c.keys, c.desc)
        assert sizes.max() <= S.MAX_WINDOW and not S.takes_fallback(c.keys, c.desc), c.name
        seen[c.desc] |= set(int(x) for x in sizes)
    for desc in (False, True):
        assert seen[desc] == set(range(1, S.MAX_WINDOW + 1)), (cls, desc)


@pytest.mark.parametrize("cls", list(S.CLASSES))
def test_network_variants_hold_duplicates_and_extremes(cls):
    for c in S.network_inputs(cls, "dups"):
        _, cnt = np.unique(c.keys, return_counts=True)
        # half of every large bucket is one value: the input's largest window is such a bucket
        assert cnt.max() >= S.window_sizes(c.keys, c.desc).max() // 2, c.name
    ex = S.network_inputs(cls, "extremes")
    for desc in (False, True):
        allu = np.concatenate([S.umap(c.keys, c.desc) for c in ex if c.desc == desc])
        assert (allu == 0).any() and (allu == S.ONES).any()
    allk = np.concatenate([c.keys for c in ex])
    assert (allk == S.I64_MIN).any() and (allk == S.I64_MAX).any()


def test_two_round_inputs_split_at_or_across_16384():
    cases = S.two_round_inputs()
    names = {c.name for c in cases}
    assert {"two-uniform-16385", "two-uniform-24576"} <= names
    for c in cases:
        n = len(c.keys)
        assert S.LDS_KEYS < n <= S.LS_CAP and S.class_of(n) == "L", c.name
        for desc in ((False, True) if c.desc is None else (c.desc,)):
            assert not S.takes_fallback(c.keys, desc), c.name
            win = S.window_starts(c.keys, desc)
            mid, rest = S.round_split(c.keys, desc)
            assert 0 < mid <= S.LDS_KEYS and 0 < rest <= S.LDS_KEYS, c.name
            if "boundary16384" in c.name:  # a window starts exactly at the end of the first round
                assert mid == S.LDS_KEYS and S.LDS_KEYS in win
            if "straddle100" in c.name:    # a 100-key window lies across it and opens round 1
                q = np.flatnonzero((win[:-1] < S.LDS_KEYS) & (win[1:] > S.LDS_KEYS))
                assert len(q) == 1 and win[q[0] + 1] - win[q[0]] == 100 and mid == win[q[0]]
    assert max(len(c.keys) for c in cases) == S.LS_CAP and min(len(c.keys) for c in cases) == S.LDS_KEYS + 1


@pytest.mark.parametrize("cls", list(S.CLASSES))
def test_fallback_inputs_have_a_window_over_128(cls):
    lo, hi, _, _ = S.CLASSES[cls]
    cases = S.fallback_inputs(cls)
    assert len(cases) == len(S.FALLBACK_SIZES[cls]) * len(S.FALLBACK_KINDS)
    assert {len(c.keys) for c in cases} >= {lo if lo > 1 else hi, hi}       # the class edges
    threads = {"S": 256, "M": 512, "M2": 512, "L": 1024}[cls]
    assert any(len(c.keys) % threads for c in cases)                       # padded positions exist
    for c in cases:
        assert S.class_of(len(c.keys)) == cls, c.name
        for desc in (False, True):
            assert S.window_sizes(c.keys, desc).max() > S.MAX_WINDOW and S.takes_fallback(c.keys, desc), c.name
        if c.name.endswith("win129"):  # only just: the smallest window the networks cannot take
            assert S.window_sizes(c.keys, False).max() < 129 + 64
        if c.name.endswith("maxrun"):
            assert (c.keys == S.I64_MAX).sum() >= 129 and (S.umap(c.keys, False) == S.ONES).sum() >= 129
            assert (S.umap(c.keys, False) == 0).any()  # key - min keeps the run at all ones
        if c.name.endswith("minrun"):
            assert (S.umap(c.keys, True) == S.ONES).sum() >= 129 and (S.umap(c.keys, True) == 0).any()


def test_tiny_inputs_are_one_window():
    for c in S.tiny_inputs():
        for desc in (False, True):
            assert len(c.keys) <= 2 and not S.takes_fallback(c.keys, desc)


def test_multi_level_inputs_are_what_they_say():
    for hb in S.NARROW_HB:
        for name, base in S.narrow_bases(hb).items():
            for n in S.NARROW_N:
                v = S.narrow_range(hb, base, n)
                assert n > S.LS_CAP and v.dtype == np.int64 and len(v) == n
                lo, hi = int(v.min()), int(v.max())
                # max - min has exactly hb bits: the rebased first digit starts below bit hb
                assert lo >= base and hi <= base + (1 << hb) - 1 and (hi - lo).bit_length() == hb, (hb, name, n)
    assert S.narrow_range(3, int(S.I64_MAX) - 7, 24577).max() == S.I64_MAX
    assert S.narrow_range(3, int(S.I64_MIN), 24577).min() == S.I64_MIN
    # hb = 10 at 200 000 keys: the first level's 512 sub-segments hold 2 values of ~195 keys
    v = S.narrow_range(10, 0, 200_000)
    assert np.bincount(v).min() > S.MAX_WINDOW
    for w in S.CLUSTER_W:
        v = S.cluster(w)
        inside = (v >= (1 << 50)) & (v < (1 << 50) + (1 << w))
        assert len(v) == S.CLUSTER_N and inside.sum() >= S.CLUSTER_N // 2 > S.LS_CAP
    names = [c.name for c in S.tile_edge_inputs()]
    assert len(names) == len(S.TILE_FULL_N) + 2 * len(S.TILE_COPY_N)
    for t in (2 * 14336, 4 * 14336, 1 << 18, 1 << 16):
        assert {t - 1, t, t + 1} <= set(S.TILE_FULL_N) | set(S.TILE_COPY_N)
    for c in S.tile_edge_inputs():
        if "two" in c.name:
            assert len(np.unique(c.keys)) == 2
        if "const" in c.name:
            assert len(np.unique(c.keys)) == 1


@pytest.mark.parametrize("m", list(S.BYTE_SETS))
def test_byte_mask_keys_vary_in_exactly_m_bytes(m):
    sets = S.BYTE_SETS[m]
    assert all(len(s) == m and len(set(s)) == m for s in sets)
    for varying in sets:
        for f64 in (False, True):
            keys = S.byte_mask_keys(varying, f64)
            assert keys.dtype == (np.float64 if f64 else np.int64) and len(keys) == S.BYTE_MASK_N
            for desc in (False, True):
                u = ukey(keys, desc)
                live = [b for b in range(8) if len(np.unique((u >> np.uint64(8 * b)) & np.uint64(255))) > 1]
                assert tuple(live) == tuple(varying), (varying, f64, desc)
    union = set().union(*[set(s) for s in sets])
    if 1 < m < 8:  # with and without byte 7, and a non-adjacent choice
        assert any(7 in s for s in sets) and any(7 not in s for s in sets)
        assert any(max(s) - min(s) + 1 > m for s in sets)
    assert union
