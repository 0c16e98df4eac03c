"""CPU: the C oracle's f64 SUM / MIN / MAX on NaN, +-inf, subnormal, overflowing and zero
data, against a reference written here in plain Python — the oracle is the checker of every
GPU test in tests/test_gpu_nonfinite.py, so it is pinned first.

Reference, per group: any NaN -> NaN; both infinities -> NaN; one infinity -> it; otherwise
the exact sum as fractions.Fraction rounded once by float() (OverflowError: the infinity of
the sum's sign).  MIN / MAX: the extreme of the values' total-order words (helpers.f64_ord),
decoded.  The values come from helpers.nonfinite_values, whose finite sums are exact in any
order, so every comparison is bit for bit (a NaN sum: isnan only).  Both the per-thread
fold (nthreads 1) and grp_merge (nthreads > 1) are exercised."""
import math
from fractions import Fraction

import numpy as np
import pytest

from helpers import (NF_BOTH_INF, NF_NAN, NF_NINF, NF_PINF, NF_PLAIN, NF_SUBNORMAL, OPCODE, f64_from_ord, f64_ord,
                     nf_check, nf_covers_all, nonfinite_divisors, nonfinite_values)
from oracle.expr import F64, groupby_prog

AGGS4 = [(0, 0, (0,)), (1, 0, ()), (2, 0, (0,)), (3, 0, (0,))]  # SUM, COUNT, MIN, MAX of value 0


def py_sum(vals):
    """IEEE sum of a group in any order, for data whose finite sums are exact"""
    vals = [float(x) for x in vals]
    if any(math.isnan(x) for x in vals):
        return math.nan
    pinf, ninf = math.inf in vals, -math.inf in vals
    if pinf and ninf:
        return math.nan
    if pinf or ninf:
        return math.inf if pinf else -math.inf
    s = sum((Fraction(x) for x in vals), Fraction(0))
    try:
        return float(s)
    except OverflowError:
        return math.inf if s > 0 else -math.inf


def py_groupby(key, val, mask=None):
    """(keys [g, 1], words [g, 4]) of SUM, COUNT, MIN, MAX like oracle.groupby, in Python"""
    if mask is not None:
        key, val = key[mask], val[mask]
    order = np.argsort(key, kind="stable")
    key, val = key[order], val[order]
    uk, start = np.unique(key, return_index=True)
    end = np.append(start[1:], len(key))
    words = np.empty((len(uk), 4), dtype=np.uint64)
    for g, (a, b) in enumerate(zip(start, end)):
        v = val[a:b]
        o = f64_ord(v)
        words[g, 0] = np.array([py_sum(v)], dtype=np.float64).view(np.uint64)[0]
        words[g, 1] = b - a
        words[g, 2] = f64_from_ord(o.min().reshape(1)).view(np.uint64)[0]
        words[g, 3] = f64_from_ord(o.max().reshape(1)).view(np.uint64)[0]
    return uk.reshape(-1, 1), words


def test_py_sum_table():
    """the cases the oracle got wrong before it followed IEEE (1.0 + inf + 2.0 was NaN)"""
    assert py_sum([1.0, math.inf, 2.0]) == math.inf
    assert py_sum([1e308, 1e308]) == math.inf
    assert py_sum([-1.5e308, -1.5e308]) == -math.inf
    assert math.isnan(py_sum([math.inf, -math.inf, 1.0]))
    assert math.isnan(py_sum([math.nan, 1.0]))
    assert py_sum([5e-324, 5e-324, -1.5e-323]) == -5e-324


@pytest.mark.parametrize("nthreads", [1, 2, 7])
@pytest.mark.parametrize("vals,want", [([1.0, np.inf, 2.0], np.inf), ([1e308, 1e308], np.inf),
                                        ([2.0, -np.inf, 1.0, -np.inf], -np.inf), ([-1.5e308, -1.5e308], -np.inf),
                                        ([np.inf, -np.inf, 1.0], np.nan), ([np.nan, 1.0], np.nan),
                                        ([1.0, np.inf, np.nan], np.nan), ([5e-324, 1e-323], 4.5e-323)])
def test_oracle_sum_known_answers(orc, nthreads, vals, want):
    """`want`: the sum of three copies of `vals` (every thread chunk holds some), by hand"""
    val = np.array(vals * 3, dtype=np.float64)
    key = np.zeros(len(val), dtype=np.int64)
    _, w = orc.groupby([key], AGGS4, values=[val], nthreads=nthreads, method="tables")
    got = w[0, 0:1].view(np.float64)[0]
    for ref in (want, py_sum(val)):
        assert (math.isnan(got) and math.isnan(ref)) or got == ref, (got, ref)


@pytest.mark.parametrize("nthreads", [1, 3, 16])
@pytest.mark.parametrize("G", [8, 1000])
def test_oracle_vs_python_reference(orc, nthreads, G):
    rng = np.random.default_rng(100 + G)
    n = 20_011
    key = rng.integers(0, G, n).astype(np.int64) * 7 - 3 * G
    val = nonfinite_values(rng, key)
    pk, pw = py_groupby(key, val)
    nf_covers_all(pw[:, 0])
    for method in ("auto", "tables"):
        ok, ow = orc.groupby([key], AGGS4, values=[val], nthreads=nthreads, method=method)
        nf_check(ok, ow, pk, pw, what=(method, nthreads))
    # a predicate on a second, finite column keeps the classes pure
    f = rng.integers(0, 100, n).astype(np.int64)
    ok, ow = orc.groupby([key], AGGS4, values=[val], preds=[(f, OPCODE[">="], 30)], nthreads=nthreads)
    pk, pw = py_groupby(key, val, f >= 30)
    nf_check(ok, ow, pk, pw, what="pred")


def test_oracle_merge_meets_infinities_from_different_threads(orc):
    """grp_merge: one group whose +inf lies in the first thread's chunk and whose -inf in the
    last one's (NaN), and one whose two halves are each finite but overflow together."""
    n = 4000
    key = np.arange(n, dtype=np.int64) % 2
    val = np.ones(n)
    val[0], val[n - 2] = np.inf, -np.inf           # key 0
    val[1::2] = 1e305                               # key 1: 2000 * 1e305 overflows
    for nthreads in (1, 2, 4):
        _, w = orc.groupby([key], AGGS4, values=[val], nthreads=nthreads, method="tables")
        s = w[:, 0].view(np.float64)
        assert np.isnan(s[0]) and s[1] == np.inf, (nthreads, s)


def test_oracle_finite_sums_keep_their_compensation(orc):
    """The non-finite rule leaves finite sums alone: ill-conditioned finite data still gets
    the compensated result (a plain running sum gives 0 here), with one thread and with a
    merge."""
    val = np.array([1e100] + [1.0] * 10 + [-1e100], dtype=np.float64)
    key = np.zeros(len(val), dtype=np.int64)
    want = math.fsum(val)
    assert want == 10.0 and sum(val) == 0.0
    for nthreads in (1, 4):
        _, w = orc.groupby([key], [(0, 0, (0,))], values=[val], nthreads=nthreads, method="tables")
        assert w[0, 0:1].view(np.float64)[0] == want


def test_expr_oracle_div_mod_by_zero():
    """oracle/expr.py on the same values: f64 `/` and fmod with a divisor column that holds
    0.0 and -0.0 (x / 0 = +-inf, 0 / 0 and fmod(x, 0) NaN), expected values from numpy."""
    rng = np.random.default_rng(7)
    n = 20_011
    G = 16
    key = rng.integers(0, G, n).astype(np.int64)
    f0 = nonfinite_values(rng, key)
    f1 = nonfinite_divisors(rng, key)  # keys 8..15: with 0.0 and -0.0
    div = [("col", 0), ("col", 1), ("div",)]
    mod = [("col", 0), ("col", 1), ("mod",)]
    ok, ow, types = groupby_prog([key], [f0, f1], None, [(0, div, None), (2, div, None), (3, div, None),
                                                           (2, mod, None), (3, mod, None), (1, None, None)])
    assert types[:5] == [F64] * 5
    with np.errstate(all="ignore"):
        q, r = f0 / f1, np.fmod(f0, f1)
    assert np.isinf(q).any() and np.isnan(q).any() and np.isnan(r).any()
    for g, k in enumerate(np.unique(key)):
        m = key == k
        assert ok[g, 0] == k and ow[g, 5] == m.sum()
        s = ow[g, 0:1].view(np.float64)[0]
        want = py_sum(q[m])
        assert (math.isnan(s) and math.isnan(want)) or s == want, (k, s, want)
        for j, x, pick in ((1, q, np.min), (2, q, np.max), (3, r, np.min), (4, r, np.max)):
            assert ow[g, j] == f64_from_ord(pick(f64_ord(x[m])).reshape(1)).view(np.uint64)[0], (k, j)
    # groups without a zero divisor keep their class's sum; with one, x / +-0 meets both signs
    s = ow[:, 0].view(np.float64)
    assert np.all(np.isnan(s[[NF_BOTH_INF, NF_NAN]])) and s[NF_PINF] == np.inf and s[NF_NINF] == -np.inf
    assert np.isfinite(s[NF_PLAIN]) and np.isfinite(s[NF_SUBNORMAL]) and s[NF_SUBNORMAL] != 0
    assert np.all(np.isnan(s[8:]))
