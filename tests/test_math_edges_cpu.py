"""CPU: the Python restatement of the math ops (tests/math_edges.py) against exact arithmetic —
rounding and casts against fractions.Fraction and Python integers, toFloat32 against struct and
numpy, sqrt against `decimal` at 60 digits and against the squares of its neighbours, the NaN
rules by bit pattern — and the transcendental reference: numpy's own exp / log / log2 / log10 /
power must stay inside the ulp bounds on every operand, which shows the reference and the
operand lists are sound."""
import math
import struct
from decimal import Decimal
from fractions import Fraction

import numpy as np
import pytest

import math_edges as M
from expr_edges import DBL_MAX, DENORM_MIN, MAX, MIN

FINITE = [x for x in M.F if x == x and not math.isinf(x)]
NANS = [x for x in M.F if x != x]


def test_operand_lists():
    assert len(NANS) == 3 and {M.fbits(x) for x in NANS} == {M.QNAN, M.NEG_QNAN, M.SNAN}
    for v in (0.0, -0.0, DENORM_MIN, -DENORM_MIN, 0.5, -0.5, 1.5, 2.5, -2.5, 2.0**52 - 0.5, 2.0**53, 1e18, -1e300, DBL_MAX,
              math.inf, -math.inf, 2.0**63, -2.0**63, math.nextafter(2.0**63, 0), math.nextafter(-2.0**63, -math.inf), 2.0**31,
              math.nextafter(2.0**31, 0), 1 + 2.0**-52, -(1 - 2.0**-52)):
        assert M.fbits(v) in M.F_BITS, v
    for v in (5, -5, 15, -15, 25, -25, 5 * 10**17, -5 * 10**17, MIN + 9, MAX - 9, MIN, MAX):
        assert v in M.I
    assert all(len(M.operands(s)[0][0]) % 64 for s in ("F", "I", "EE", "FF", "IF", "exp", "ln", "pow"))
    assert all(1 <= len(p) <= 8 for _, p in M.EVAL_SPECS.values())


# ------------------------------------------------------------------ rounding
def test_round0_against_fractions():
    cells = 0
    for x in FINITE:
        q = Fraction(x)
        want = [math.floor(q), math.ceil(q), math.trunc(q), None]
        fl = math.floor(q)
        d = q - fl  # round half to even
        want[3] = fl + (1 if d > Fraction(1, 2) or (d == Fraction(1, 2) and fl % 2) else 0)
        for mode in range(4):
            r = M.round0(x, mode)
            assert Fraction(r) == want[mode], (x, mode)
            if r == 0:
                assert math.copysign(1, r) == math.copysign(1, x), (x, mode)  # ceil(-0.5) = -0.0
            cells += 1
    assert cells == 4 * len(FINITE)
    assert M.fbits(M.round_f(-0.5, 1, 0)) == 0x8000000000000000 and M.round_f(2.5, 3, 0) == 2.0 and M.round_f(-1.5, 3, 0) == -2.0


def test_round_f_steps_are_single_ieee_operations():
    """op(x * 10^N) / 10^N: the scaling, checked as one correctly rounded operation each
    (float(Fraction) rounds correctly), the not-finite rule, NaN and infinity"""
    cells = 0
    for n in (1, 2, 5, 18, -1, -2, -18):
        s = Fraction(10)**abs(n)
        for x in FINITE:
            t = Fraction(x) * s if n > 0 else Fraction(x) / s
            for mode in range(4):
                got = M.round_f(x, mode, n)
                if abs(t) >= Fraction(DBL_MAX) + Fraction(2)**970:  # x * 10^N rounds to infinity
                    assert got == x
                else:
                    r = Fraction(M.round0(float(t), mode))
                    back = r / s if n > 0 else r * s
                    if abs(back) < Fraction(DBL_MAX):
                        assert got == float(back) and (got != 0 or math.copysign(1, got) == math.copysign(1, x) or r != 0)
                cells += 1
    assert cells == 7 * 4 * len(FINITE)
    for n in M.DIGITS:
        for mode in range(4):
            assert M.round_f(math.inf, mode, n) == math.inf and M.round_f(-math.inf, mode, n) == -math.inf
            assert M.fbits(M.round_f(-0.0, mode, n)) == 0x8000000000000000
            for x in NANS:
                assert M.fbits(M.round_f(x, mode, n)) == M.fbits(x) | M.QUIET
    assert M.round_f(1e300, 0, 18) == 1e300  # the scaled value is infinite: x
    assert M.round_f(0.125, 3, 2) == 0.12 and M.round_f(0.375, 3, 2) == 0.38 and M.round_f(1234.5678, 2, -2) == 1200.0 and M.round_f(1250.0, 3, -2) == 1200.0


def test_round_i_against_integers():
    cells = wraps = 0
    for n in (-1, -2, -18):
        m = 10**-n
        for x in M.I:
            below = max(k * m for k in range(x // m - 1, x // m + 2) if k * m <= x)
            above = min(k * m for k in range(x // m - 1, x // m + 3) if k * m >= x)
            toward = below if x >= 0 else above
            if x - below != above - x:
                nearest = below if x - below < above - x else above
            else:
                nearest = above if x >= 0 else below  # a tie: away from zero
            for mode, w in enumerate((below, above, toward, nearest)):
                got = M.round_i(x, mode, n)
                assert got == M.wrap(w), (x, mode, n)
                if not MIN <= w <= MAX:
                    wraps += 1
                    assert x < MIN + m or x > MAX - m  # only values within m of the ends wrap
                cells += 1
    assert cells == 12 * len(M.I) and wraps >= 10
    for x in M.I:
        assert all(M.round_i(x, mode, n) == x for mode in range(4) for n in (0, 2, 18))
    assert [M.round_i(v, 3, -1) for v in (5, -5, 15, -15, 25, -25, 14, -14)] == [10, -10, 20, -20, 30, -30, 10, -10]
    assert M.round_i(-5 * 10**17, 3, -18) == -10**18 and M.round_i(5 * 10**17 - 1, 3, -18) == 0


# ------------------------------------------------------------------ casts
def test_casts_against_fractions_and_struct():
    cells = 0
    for x in M.F:
        if x != x:
            want = 0
        elif math.isinf(x):
            want = MAX if x > 0 else MIN
        else:
            want = min(max(math.trunc(Fraction(x)), MIN), MAX)
        assert M.cast(x, 0) == want, x
        for c, (size, signed) in {1: (4, True), 2: (2, True), 3: (1, True), 4: (4, False), 5: (2, False), 6: (1, False)}.items():
            low = (want % 2**64).to_bytes(8, "little")[:size]
            assert M.cast(x, c) == int.from_bytes(low, "little", signed=signed), (x, c)
            cells += 1
    for x in M.I:
        for c, (size, signed) in {0: (8, True), 1: (4, True), 3: (1, True), 5: (2, False), 6: (1, False)}.items():
            assert M.cast(x, c) == int.from_bytes((x % 2**64).to_bytes(8, "little")[:size], "little", signed=signed)
            cells += 1
    assert cells == 6 * len(M.F) + 5 * len(M.I)
    assert [M.cast(v, 3) for v in (127.0, 127.5, 128.0, -128.0, -129.0, 255.9, 256.0)] == [127, 127, -128, -128, 127, -1, 0]
    assert [M.cast(v, 0) for v in (math.nan, math.inf, -math.inf, 1e19, -1e19, -0.5, 2.0**63)] == [0, MAX, MIN, MAX, MIN, 0, MAX]


def f32_neighbours(v):
    """the binary32 values next to v on both sides, as Fractions (past the largest: +-2^128)"""
    out = []
    with np.errstate(over="ignore"):
        for to in (-np.inf, np.inf):
            nb = float(np.nextafter(np.float32(v), np.float32(to)))
            out.append(Fraction(2)**128 * (1 if nb > 0 else -1) if math.isinf(nb) else Fraction(nb))
    return out


def test_to_float32_against_struct_and_fractions():
    fmax = Fraction(3.4028234663852886e38)
    half = Fraction(2)**103  # half an ulp at the top binade of binary32
    cells = 0
    for x in FINITE:
        got = M.cast(x, 7)
        if abs(Fraction(x)) >= fmax + half:
            assert math.isinf(got) and math.copysign(1, got) == math.copysign(1, x)
        else:
            assert got == struct.unpack("<f", struct.pack("<f", x))[0] and M.fbits(got) >> 63 == M.fbits(x) >> 63
            for nb in f32_neighbours(got):
                assert abs(Fraction(got) - Fraction(x)) <= abs(nb - Fraction(x)), x
        cells += 1
    for i in M.I:  # an int rounds once, not through float64
        got = Fraction(M.cast(i, 7))
        for nb in f32_neighbours(float(got)):
            assert abs(got - i) <= abs(nb - i), i
        cells += 1
    assert cells == len(FINITE) + len(M.I)
    assert M.cast(2**24 + 1, 7) == 2.0**24 and M.cast(16777217.0, 7) == 2.0**24 and M.cast(1e-46, 7) == 0.0
    # 2^63 - 2^38 - 1 is below the binary32 tie 2^63 - 2^38; through float64 (which rounds it
    # up to the tie) it would round to even, 2^63
    assert M.cast(2**63 - 2**38 - 1, 7) == float(2**63 - 2**39) and float(np.float32(float(2**63 - 2**38 - 1))) == 2.0**63
    for x in NANS:
        assert M.fbits(M.cast(x, 7)) == M.fbits(x) | M.QUIET


# ------------------------------------------------------------------ sqrt, sign, least / greatest
def test_sqrt_is_correctly_rounded():
    cells = 0
    for x in [v for v in FINITE if v > 0] + M.SQRT_X:
        r = M.sqrt(x)
        lo = (Fraction(r) + Fraction(math.nextafter(r, 0))) / 2
        hi = (Fraction(r) + Fraction(math.nextafter(r, math.inf))) / 2
        assert lo * lo <= Fraction(x) <= hi * hi, x
        assert r == float(Fraction(M.CTX.sqrt(Decimal(x)))), x  # 60 digits, rounded once more
        cells += 1
    assert cells > 2000
    assert M.fbits(M.sqrt(-0.0)) == 0x8000000000000000 and M.sqrt(math.inf) == math.inf and M.sqrt(0.0) == 0.0
    for x in (-1.0, -DENORM_MIN, -math.inf):
        assert M.fbits(M.sqrt(x)) == M.NEG_QNAN
    for x in NANS:
        assert M.fbits(M.sqrt(x)) == M.fbits(x) | M.QUIET


def test_sign_least_greatest_rules():
    assert [M.sign(v) for v in (math.nan, 0.0, -0.0, DENORM_MIN, -math.inf, MIN, 0, 7)] == [0, 0, 0, 1, -1, -1, 0, 1]
    cells = 0
    for a, b in zip(*M.FF):
        lo, hi = M.least(a, b), M.least(a, b, True)
        if a != a:
            assert M.fbits(lo) == M.fbits(hi) == M.fbits(a) | M.QUIET  # the first operand's first
        elif b != b:
            assert M.fbits(lo) == M.fbits(hi) == M.fbits(b) | M.QUIET
        elif a == b:
            assert M.fbits(lo) == M.fbits(hi) == M.fbits(a)  # equal (+-0.0 included): the first
        else:
            assert (lo, hi) == (min(a, b), max(a, b))
        cells += 1
    assert cells == 441
    assert M.least(MAX, MAX - 1) == MAX - 1 and isinstance(M.least(3, 4), int) and M.least(3, 2.5) == 2.5
    assert M.least(2**53 + 1, 2.0**53) == 2.0**53 and M.fbits(M.least(2**53 + 1, 2.0**53, True)) == M.fbits(2.0**53)  # as f64: equal


# ------------------------------------------------------------------ the transcendental reference
def test_special_cases_by_bit_pattern():
    nq = M.fval(M.NEG_QNAN)
    sn = M.fval(M.SNAN)
    for fn in ("exp", "ln", "log2", "log10"):
        assert M.fbits(M.special(fn, sn)) == M.SNAN | M.QUIET and M.fbits(M.special(fn, nq)) == M.NEG_QNAN
    for fn in ("ln", "log2", "log10"):
        assert M.special(fn, 0.0) == M.special(fn, -0.0) == -math.inf and M.special(fn, math.inf) == math.inf
        assert M.fbits(M.special(fn, -1.0)) == M.fbits(M.special(fn, -math.inf)) == M.NEG_QNAN
    assert M.special("exp", -math.inf) == 0.0 and M.special("exp", math.inf) == math.inf and M.special("exp", 1.0) is None
    p = M.pow_special
    assert p(sn, 0.0) == p(sn, -0.0) == p(1.0, sn) == p(-1.0, math.inf) == p(-1.0, -math.inf) == 1.0
    assert M.fbits(p(sn, nq)) == M.SNAN | M.QUIET and M.fbits(p(2.0, nq)) == M.NEG_QNAN  # the first operand's first
    assert M.fbits(p(-8.0, 0.5)) == M.NEG_QNAN and p(-8.0, 3.0) is None
    assert (p(0.0, -1.0), p(-0.0, -1.0), p(-0.0, -2.0), p(-0.0, 3.0), p(-0.0, 2.0)) == (math.inf, -math.inf, math.inf, 0.0, 0.0)
    assert M.fbits(p(-0.0, 3.0)) == 0x8000000000000000 and M.fbits(p(-math.inf, -3.0)) == 0x8000000000000000
    assert (p(-math.inf, 3.0), p(-math.inf, 2.0), p(0.5, -math.inf), p(2.0, -math.inf), p(math.inf, -1.0)) == (-math.inf, math.inf, math.inf, 0.0, 0.0)


def test_ulp_error_measures_what_it_says():
    one = Fraction(1)
    assert M.ulp_error(1.0, one) == 0 and M.ulp_error(1 + 2.0**-52, one) == 1 and M.ulp_error(1 - 2.0**-53, one) == 0.5
    assert M.ulp_error(DENORM_MIN, Fraction(0)) == 1 and M.ulp_error(0.0, Fraction(DENORM_MIN) * 3) == 3
    assert M.ulp_error(math.inf, Fraction(2)**1024) == 0 and M.ulp_error(math.inf, Fraction(DBL_MAX)) == 1
    assert M.ulp_error(DBL_MAX, Fraction(2)**1024 * 3) == math.inf and M.ulp_error(-0.0, Fraction(1, 10**400)) == math.inf
    assert M.ulp_error(math.nan, one) == math.inf and M.ulp_error(-1.0, one) == math.inf


NP_FN = {"exp": np.exp, "ln": np.log, "log2": np.log2, "log10": np.log10, "pow": np.power}


@pytest.mark.parametrize("fn", sorted(M.ULP_BOUND))
def test_numpy_stays_within_the_bounds(fn):
    """the host library on the same operands under the same check: classes exactly (numpy
    keeps C99's special values; its NaN signs are its own, so a NaN is compared as a NaN), the
    rest within the bound"""
    cols, _ = M.operands("pow" if fn == "pow" else fn)
    with np.errstate(all="ignore"):
        got = NP_FN[fn](*cols)
    ref = M.reference(fn)
    worst, exact, n = 0.0, 0, 0
    for r, (g, w) in enumerate(zip(got.tolist(), ref)):
        n += 1
        if isinstance(w, float):
            exact += 1
            assert (g != g) if w != w else M.fbits(g) == M.fbits(w), (fn, r, g, w)
            continue
        err = M.ulp_error(g, w)
        worst = max(worst, err)
        assert err <= M.ULP_BOUND[fn], (fn, r, cols[0][r], g, err)
    print(f"{fn}: numpy max {worst:.3f} ulp over {n} operands ({exact} exact by rule)")
    assert n == len(cols[0]) > 2000 and exact >= 5 and 0 < worst
    # the lists reach what they are for
    fin = [w for w in ref if isinstance(w, Fraction)]
    assert any(0 < abs(w) < Fraction(2)**-1022 for w in fin) or fn in ("ln", "log2", "log10")  # subnormal results
    if fn in ("exp", "pow"):
        assert any(abs(w) >= Fraction(2)**1024 for w in fin) and any(0 < abs(w) < Fraction(2)**-1075 for w in fin)
