"""Edge operands of the math program ops (include/nutexec.h: FLOOR CEIL TRUNC ROUND, MATH, POW,
SIGN, LEAST, GREATEST, CAST; csrc/prog_ops.hpp: jroundf, jroundi, jsqrt, jsignf, jleastf, jtoi64,
jnarrow, jtof32; the jit.cpp prelude's jexp .. jpow), and a restatement of each in Python.

oracle/expr.py does not know these ops, so the restatement below is the reference.  Python
floats are IEEE doubles and every + - * / on them is one correctly rounded operation, which is
what the ops' steps are; integers are Python integers, wrapped at the end.
tests/test_math_edges_cpu.py pins the restatement against exact arithmetic (fractions, decimal,
struct); tests/test_gpu_math.py runs the ops on the GPU against it.

The exactly defined ops are compared bit for bit.  exp, ln, log2, log10 and pow are correctly
rounded nowhere; their reference is `decimal` at 60 digits and the check is a distance in ulps
(ulp_error), under the bounds the device math library is built to (OpenCL full profile, double):
3 ulp for exp / ln / log2 / log10, 16 ulp for pow.

  F       f64 edge values (as bit patterns: three NaNs among them)
  I       int64 edge values: expr_edges.E and the rounding ties and wraps of N = -1, -2, -18
  FF, IF  pairs for least / greatest
  TR      per transcendental function its operands: directed ones and about 2000 seeded random
"""
import functools
import math
import struct
from decimal import Context, Decimal
from fractions import Fraction

import numpy as np

from expr_edges import DBL_MAX, DBL_MIN, DENORM_MIN, E, EE, MAX, MIN, i64

QNAN, NEG_QNAN, SNAN = 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000001234
QUIET = 0x0008000000000000
ULP_BOUND = {"exp": 3, "ln": 3, "log2": 3, "log10": 3, "pow": 16}
MF = ["sqrt", "exp", "ln", "log2", "log10"]  # nut_math_fn
CASTS = ["i64", "i32", "i16", "i8", "u32", "u16", "u8", "f32"]  # nut_cast
MODES = ["floor", "ceil", "trunc", "round"]
DIGITS = [0, 2, -2, 18, -18]


def fbits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def fval(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def quiet(x):
    return fval(fbits(x) | QUIET)


def wrap(x):
    return (x + 2**63) % 2**64 - 2**63


def word(v):
    """the 8-byte result word of a value: an int wraps, a float gives its bits"""
    return fbits(v) if isinstance(v, float) else wrap(int(v)) % 2**64


# ------------------------------------------------------------------ the restatement
def round0(x, mode):
    """IEEE floor / ceil / trunc / round-half-to-even of a non-NaN double"""
    if math.isinf(x) or abs(x) >= 2.0**52:
        return x
    r = float([math.floor, math.ceil, math.trunc, round][mode](x))  # (Python's round: half to even, exact)
    return math.copysign(0.0, x) if r == 0.0 else r


def round_f(x, mode, n):
    if x != x:
        return quiet(x)
    if n == 0:
        return round0(x, mode)
    s = float(10**abs(n))
    t = x * s if n > 0 else x / s
    if math.isinf(t):
        return x
    r = round0(t, mode)
    return r / s if n > 0 else r * s


def round_i(x, mode, n):
    if n >= 0:
        return x
    m = 10**-n
    lo, hi = x // m * m, -(-x // m) * m
    if mode == 3:
        q, r = divmod(abs(x), m)
        return wrap((q + (2 * r >= m)) * m * (1 if x >= 0 else -1))
    return wrap([lo, hi, lo if x >= 0 else hi][mode])


def sqrt(x):
    if x != x:
        return quiet(x)
    return fval(NEG_QNAN) if x < 0 else math.sqrt(x)  # (math.sqrt: the C library's, correctly rounded)


def sign(x):
    return 1 if x > 0 else -1 if x < 0 else 0


def least(a, b, greatest=False):
    if isinstance(a, int) and isinstance(b, int):
        return (b if b > a else a) if greatest else (b if b < a else a)
    a, b = float(a), float(b)
    if a != a:
        return quiet(a)
    if b != b:
        return quiet(b)
    return (b if b > a else a) if greatest else (b if b < a else a)


def to_i64(x):
    if isinstance(x, int):
        return x
    if x != x:
        return 0
    return MAX if x >= 2.0**63 else MIN if x <= -2.0**63 else int(x)


def cast(x, c):
    if c == 7:
        if isinstance(x, int):  # an int rounds to binary32 directly
            return float(np.array([x], dtype=np.int64).astype(np.float32)[0])
        if x != x:
            return quiet(x)
        with np.errstate(over="ignore"):
            return float(np.float32(x))
    v = to_i64(x)
    if c == 0:
        return v
    bits_ = {1: 32, 2: 16, 3: 8, 4: 32, 5: 16, 6: 8}[c]
    v %= 2**bits_
    return v - 2**bits_ if c <= 3 and v >= 2**(bits_ - 1) else v


# ---- exp, ln, log2, log10, pow: the result's class by rule, else the true value (60 digits)
CTX = Context(prec=60, Emax=999999999, Emin=-999999999, traps=[])


def is_odd(y):
    return abs(y) < 2.0**53 and y == int(y) and int(y) % 2 == 1


def pow_special(x, y):
    """C99 F.10.4.4 under the NaN rule of include/nutexec.h: the result where it is exact
    (a float), or None where x ** y is a finite computation"""
    if y == 0 or x == 1:
        return 1.0
    if x != x:
        return quiet(x)
    if y != y:
        return quiet(y)
    if x == 0:
        if y < 0:
            return math.copysign(math.inf, x) if is_odd(y) else math.inf
        return math.copysign(0.0, x) if is_odd(y) else 0.0
    if math.isinf(y):
        if x == -1:
            return 1.0
        return math.inf if (abs(x) > 1) == (y > 0) else 0.0
    if math.isinf(x):
        if x > 0:
            return math.inf if y > 0 else 0.0
        if y < 0:
            return -0.0 if is_odd(y) else 0.0
        return -math.inf if is_odd(y) else math.inf
    if x < 0 and y != int(y):
        return fval(NEG_QNAN)
    return None


def special(fn, x, y=None):
    if fn == "pow":
        return pow_special(x, y)
    if x != x:
        return quiet(x)
    if fn == "exp":
        return math.inf if x == math.inf else 0.0 if x == -math.inf else None
    if x < 0:
        return fval(NEG_QNAN)
    return -math.inf if x == 0 else math.inf if x == math.inf else None


def true_value(fn, x, y=None):
    """the function's value as a Fraction (60 correct digits), or +-Fraction(10)**400 / 0 with
    the result's sign where it is beyond every double; only where special() is None"""
    d = Decimal(x)
    if fn == "exp":
        r = CTX.exp(d)
    elif fn == "ln":
        r = CTX.ln(d)
    elif fn == "log10":
        r = CTX.log10(d)
    elif fn == "log2":
        r = CTX.divide(CTX.ln(d), CTX.ln(Decimal(2)))
    else:
        r = CTX.power(abs(d), Decimal(y))
        if x < 0 and is_odd(y):
            r = -r
    if r.is_infinite() or (r != 0 and r.adjusted() > 400):
        return Fraction(10)**400 * (-1 if r < 0 else 1)
    if r != 0 and r.adjusted() < -400:
        return Fraction(1, 10**400) * (-1 if r < 0 else 1)
    return Fraction(r)


TWO1024 = Fraction(2)**1024


def ulp_error(got, true):
    """|got - true| in ulps of true (units of 2^-1074 below the normal range); an infinite got
    counts as the nearest value at or beyond +-2^1024 (one step past the largest double), so it
    is exact for every true value there.  math.inf: a NaN, or a result (a zero or an infinity
    included) of the wrong sign."""
    if got != got:
        return math.inf
    if true != 0 and math.copysign(1.0, got) != (1 if true > 0 else -1):
        return math.inf
    t = abs(true)
    if t >= 2 * TWO1024:
        return 0.0 if math.isinf(got) else math.inf
    g = max(TWO1024, t) * (1 if got > 0 else -1) if math.isinf(got) else Fraction(got)
    e = -1022
    if t:
        e = t.numerator.bit_length() - t.denominator.bit_length()
        if Fraction(2)**e > t:
            e -= 1
        e = min(max(e, -1022), 1023)
    return float(abs(g - true) / Fraction(2)**(e - 52))


def check_transcendental(fn, got_bits, xs, ys=None):
    """every operand: the class exactly, else the ulp distance.  Returns (max ulp error, the
    rows that miss) — no operand is left out"""
    want = reference(fn)
    worst, bad = 0.0, []
    assert len(got_bits) == len(want) == len(xs)
    for r, (g, w) in enumerate(zip(got_bits, want)):
        if isinstance(w, float):  # exact by rule: bit for bit
            if int(g) != fbits(w):
                bad.append((r, xs[r], None if ys is None else ys[r], hex(int(g)), hex(fbits(w))))
            continue
        err = ulp_error(fval(int(g)), w)
        worst = max(worst, err)
        if not err <= ULP_BOUND[fn]:
            bad.append((r, xs[r], None if ys is None else ys[r], fval(int(g)), err))
    return worst, bad


# ------------------------------------------------------------------ operands
def _dedupe_f(vals):
    seen, out = set(), []
    for v in vals:
        b = v if isinstance(v, int) else fbits(v)
        if b not in seen:
            seen.add(b)
            out.append(b)
    return out


def _f_edges():
    pos = [0.0, DENORM_MIN, DBL_MIN, 1.0, 1 + 2.0**-52, 1 - 2.0**-52, 1 - 2.0**-53, 0.5, 1.5, 2.5, 0.005, 0.015, 1.005,
           2.0**52 - 0.5, 2.0**52 + 0.5, 2.0**52 + 1, 2.0**53, 1e18, 1e19, 1e300, DBL_MAX, math.inf,
           2.0**63, math.nextafter(2.0**63, 0), math.nextafter(2.0**63, math.inf),
           2.0**31, 2.0**31 - 1, 2.0**31 - 0.5, 2.0**31 + 0.5, math.nextafter(2.0**31, 0), math.nextafter(2.0**31, math.inf),
           2.0**32, 2.0**32 - 1, 127.0, 127.5, 128.0, 255.9, 256.0, 32767.5, 32768.0, 65535.5, 65536.0,
           150.0, 250.0, 149.99999999999997, 1234.5678, 3.4028234663852886e38, 3.4028235677973366e38, 1e-46, 16777217.0]
    vals = []
    for p in pos:
        vals += [p, -p]
    return _dedupe_f(vals + [QNAN, NEG_QNAN, SNAN])


F_BITS = _f_edges()
F = [fval(b) for b in F_BITS]
assert len(F) % 64 != 0 and len(F) > 100


def _i_edges():
    extra = [5, 15, 25, 50, 149, 150, 151, 5 * 10**17, 10**18, 15 * 10**17, 5 * 10**17 - 1, 5 * 10**17 + 1]
    vals = list(E) + [s * v for v in extra for s in (1, -1)]
    vals += [MIN + k for k in (4, 5, 6, 8, 9, 49, 50, 51, 808)] + [MAX - k for k in (2, 3, 4, 7, 8, 9, 57, 58, 807)]
    vals += [-2**31, 2**31 - 1, 2**15, 2**15 - 1, -2**15 - 1, 128, -128, -129, 255, 256, 2**24 + 1, 2**63 - 2**38, 2**63 - 2**38 - 1]
    return list(dict.fromkeys(vals))


I = _i_edges()
assert len(I) % 64 != 0 and len(I) > 70

_FP = [fval(b) for b in _dedupe_f([0.0, -0.0, 1.0, -1.0, 0.5, -2.5, DENORM_MIN, -DENORM_MIN, DBL_MAX, -DBL_MAX, math.inf, -math.inf,
                                   2.0**53, 2.0**63, -2.0**63, QNAN, NEG_QNAN, SNAN, 0xFFF0000000000007, 3.0, 2.0**53 + 2])]
FF = ([a for a in _FP for _ in _FP], [b for _ in _FP for b in _FP])
IF = ([a for a in E for _ in _FP], [b for _ in E for b in _FP])
assert len(FF[0]) == 441 and len(IF[0]) % 64 != 0


def _ldexp_rand(rng, n, lo, hi):
    """n doubles with full random mantissas and exponents uniform over [lo, hi)"""
    m = 1.0 + rng.integers(0, 2**52, n).astype(np.float64) * 2.0**-52
    return np.ldexp(m, rng.integers(lo, hi, n))


def _tr():
    rng = np.random.default_rng(2026)
    out = {}
    ex = [709.0, 709.78, 709.782712893384, math.nextafter(709.782712893384, 0), 709.7827128933841, 709.79, 710.0, 1000.0,
          -708.3964185322641, -708.4, -745.0, -745.13, -745.1332191019411, -745.1332191019412, -745.14, -746.0, -1000.0,
          -744.4400719213812, 1e-300, -1e-300, 2.0**-53, -2.0**-54, 1.0, -1.0, 0.5, math.log(2), DBL_MAX, -DBL_MAX,
          DENORM_MIN, -DENORM_MIN]
    out["exp"] = [*ex, 0.0, -0.0, math.inf, -math.inf, fval(QNAN), fval(NEG_QNAN), fval(SNAN),
                  *rng.uniform(-750, 715, 1500).tolist(), *(_ldexp_rand(rng, 500, -60, 4) * rng.choice([-1.0, 1.0], 500)).tolist()]
    near1 = [1 + k * 2.0**-52 for k in (1, 2, 3, 1000)] + [1 - k * 2.0**-53 for k in (1, 2, 3, 1000)]
    lg = [*near1, 1.0, 2.0, 10.0, 100.0, 1e15, 1e22, 1e23, 0.1, 0.5, math.e, 2.0**-1022, DBL_MIN, DENORM_MIN, 2 * DENORM_MIN,
          3 * DENORM_MIN, 2.0**-1030, 1e-310, DBL_MAX, 2.0**1023, 8.0, 1024.0, 1000.0,
          0.0, -0.0, -1.0, -DENORM_MIN, -math.inf, math.inf, fval(QNAN), fval(NEG_QNAN), fval(SNAN)]
    lg += _ldexp_rand(rng, 1200, -1022, 1024).tolist() + (1.0 + rng.uniform(-1e-3, 1e-3, 400)).tolist()
    lg += (1.0 + rng.integers(-2000, 2000, 200) * 2.0**-52).tolist() + (rng.integers(1, 2**52, 200) * DENORM_MIN).tolist()
    out["ln"] = out["log2"] = out["log10"] = lg
    bases = [0.0, -0.0, math.inf, -math.inf, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0, -8.0, 10.0, DENORM_MIN, DBL_MAX, fval(QNAN), fval(SNAN)]
    exps = [0.0, -0.0, math.inf, -math.inf, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 0.5, -0.5, 2.5, -2.5, 1e300, -1e300, 2.0**53, 2.0**53 + 2,
            1075.0, -1075.0, fval(NEG_QNAN)]
    px = [b for b in bases for _ in exps]
    py = [e for _ in bases for e in exps]
    x, y = _ldexp_rand(rng, 1200, -20, 20), rng.uniform(-60, 60, 1200)
    px += x.tolist()
    py += y.tolist()
    x, y = _ldexp_rand(rng, 400, -4, 4) * rng.choice([-1.0, 1.0], 400), rng.integers(-30, 31, 400).astype(np.float64)
    px += x.tolist()
    py += y.tolist()
    x, y = -_ldexp_rand(rng, 100, -4, 4), rng.integers(-30, 30, 100) + 0.5  # a negative base, a half-integer: invalid
    px += x.tolist()
    py += y.tolist()
    # results around the overflow and underflow thresholds: x ** (k / log2 x), k near +-1024 and -1074
    x = _ldexp_rand(rng, 300, 1, 12)
    k = rng.choice([1023.0, 1024.0, -1022.0, -1074.0, -1075.0], 300) + rng.uniform(-1.5, 1.5, 300)
    px += x.tolist()
    py += (k / np.log2(x)).tolist()
    out["pow"] = (px, py)
    return out


TR = _tr()
# sqrt beyond the edge list: full mantissas over every exponent, odd and even (correct rounding
# is checkable exactly: tests/test_math_edges_cpu.py)
SQRT_X = _ldexp_rand(np.random.default_rng(1074), 1999, -1022, 1024).tolist() + [n * DENORM_MIN for n in (2, 3, 4, 5, 2**51 + 1)]
for _k, _v in TR.items():
    _n = len(_v[0]) if _k == "pow" else len(_v)
    assert _n % 64 != 0 and _n > 2000, (_k, _n)


@functools.lru_cache(maxsize=None)
def reference(fn):
    """per operand of TR[fn]: a float (the result is exact by rule: compare the bits) or the
    true value as a Fraction (compare by ulp_error); computed once"""
    if fn == "pow":
        return [special(fn, x, y) if special(fn, x, y) is not None else true_value(fn, x, y) for x, y in zip(*TR[fn])]
    return [special(fn, x) if special(fn, x) is not None else true_value(fn, x) for x in TR[fn]]


# ------------------------------------------------------------------ programs
C0, C1 = [("col", 0)], [("col", 1)]


def model(prog, row):
    """evaluate an RPN program of these ops (and col / i64 / f64 / div / mul / add / to_f64) on
    one row of Python ints and floats"""
    st = []
    for node in prog:
        op, arg = node[0], (node[1] if len(node) > 1 else 0)
        if op == "col":
            st.append(row[arg])
        elif op == "i64":
            st.append(int(node[2]))
        elif op == "f64":
            st.append(float(node[2]))
        elif op in MODES:
            x = st.pop()
            st.append(round_i(int(x), MODES.index(op), arg) if isinstance(x, int) else round_f(x, MODES.index(op), arg))
        elif op == "math":
            assert arg == 0  # (the others have no exact model: check_transcendental)
            st.append(sqrt(float(st.pop())))
        elif op == "sign":
            st.append(sign(st.pop()))
        elif op == "cast":
            st.append(cast(st.pop(), arg))
        elif op == "to_f64":
            st.append(float(st.pop()))
        else:
            b, a = st.pop(), st.pop()
            if op in ("least", "greatest"):
                st.append(least(a, b, op == "greatest"))
            elif op == "div":
                a, b = float(a), float(b)
                st.append(a / b if b != 0 else (fval(NEG_QNAN) if a == 0 or a != a else math.copysign(math.inf, a) * math.copysign(1, b)))
            elif op in ("add", "mul"):
                both = isinstance(a, int) and isinstance(b, int)
                r = a + b if op == "add" else a * b
                st.append(wrap(r) if both else float(a) + float(b) if op == "add" else float(a) * float(b))
            else:
                raise ValueError(op)
    assert len(st) == 1
    return st[0]


def un(node, col=C0):
    return col + [node]


# nut_eval_rows specs: name -> (operand set, [program]); at most 8 programs each.  Every
# exactly defined op at N in DIGITS over F and over I, every cast, sign, sqrt, least / greatest
EVAL_SPECS = {
    "f_round_0_2": ("F", [un((m, n)) for n in (0, 2) for m in MODES]),
    "f_round_m2_18": ("F", [un((m, n)) for n in (-2, 18) for m in MODES]),
    "f_round_m18_misc": ("F", [un((m, -18)) for m in MODES] + [un(("sign",)), un(("math", 0)), un(("cast", 7))]),
    "f_cast": ("F", [un(("cast", c)) for c in range(7)]),
    "i_round_m2_m18": ("I", [un((m, n)) for n in (-2, -18) for m in MODES]),
    "i_round_m1_pos": ("I", [un((m, -1)) for m in MODES] + [un(("round", 0)), un(("floor", 2)), un(("ceil", 18)), un(("trunc", 18))]),
    "i_cast_sign": ("I", [un(("cast", c)) for c in range(8)]),
    "i_sign_sqrt": ("I", [un(("sign",)), un(("math", 0))]),
    "ff_pair": ("FF", [C0 + C1 + [("least",)], C0 + C1 + [("greatest",)]]),
    "ii_pair": ("EE", [C0 + C1 + [("least",)], C0 + C1 + [("greatest",)]]),
    "if_pair": ("IF", [C0 + C1 + [("least",)], C0 + C1 + [("greatest",)], C1 + C0 + [("least",)], C1 + C0 + [("greatest",)]]),
}
# the transcendental launches: (operand set, programs, the function of each program)
TR_SPECS = {
    "exp": ("exp", [un(("math", 1))], ["exp"]),
    "logs": ("ln", [un(("math", 2)), un(("math", 3)), un(("math", 4))], ["ln", "log2", "log10"]),
    "pow": ("pow", [C0 + C1 + [("pow",)]], ["pow"]),
}


def f64_bits(bits_):
    return np.array(bits_, dtype=np.uint64).view(np.float64)


def operands(name):
    """(numpy columns, python rows) of an operand set; f64 columns keep every NaN's bits"""
    if name == "F":
        return [f64_bits(F_BITS)], [(x,) for x in F]
    if name == "I":
        return [i64(I)], [(x,) for x in I]
    if name == "EE":
        return list(EE), list(zip(EE[0].tolist(), EE[1].tolist()))
    if name == "FF":
        return [f64_bits([fbits(x) for x in c]) for c in FF], list(zip(*FF))
    if name == "IF":
        return [i64(IF[0]), f64_bits([fbits(x) for x in IF[1]])], list(zip(*IF))
    if name == "pow":
        return [f64_bits([fbits(x) for x in c]) for c in TR["pow"]], list(zip(*TR["pow"]))
    return [f64_bits([fbits(x) for x in TR[name]])], [(x,) for x in TR[name]]


def col_types(name):
    return {"F": "f", "I": "i", "EE": "ii", "FF": "ff", "IF": "if", "pow": "ff"}.get(name, "f")


@functools.lru_cache(maxsize=None)
def eval_want(name):
    """[rows][programs] result words of EVAL_SPECS[name], computed once"""
    src, progs = EVAL_SPECS[name]
    return [[word(model(p, row)) for p in progs] for row in operands(src)[1]]


# nut_groupby computed keys (tests/test_gpu_math.py: test_groupby_paths): toInt64(f / 10), round(i, -2)
KEY_F = C0 + [("f64", 0, 10.0), ("div",), ("cast", 0)]
KEY_I = C1 + [("round", -2)]
