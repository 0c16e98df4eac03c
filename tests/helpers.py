"""Shared test helpers: the golden script's numpy restatement + comparison utilities."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import torch

_spec = importlib.util.spec_from_file_location("make_golden", Path(__file__).parent / "golden" / "make_golden.py")
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)

gen = mg.gen
pos_hash = mg.pos_hash
multiset_hash = mg.multiset_hash
wsum = mg.wsum
OPS = mg.OPS
OPCODE = {"<": 0, "<=": 1, ">": 2, ">=": 3, "==": 4, "!=": 5}


def fromhex(xs):
    return np.array([float.fromhex(x) for x in xs], dtype=np.float64)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    den = np.maximum(np.abs(b), 1e-300)
    return np.max(np.abs(a - b) / den) if len(a) else 0.0


# BASELINE.json north_star: f64 sums within 1e-12 relative.  The bound is for finite,
# non-cancelling sums; NaN, +-inf, subnormal and zero results are exact by class
# (nonfinite_values below, tests/test_gpu_nonfinite.py, tests/test_oracle_nonfinite_cpu.py).
F64_SUM_RTOL = 1e-12


# ----------------------------------------------------------------------------- special values
# NaN bit patterns mixed into a NaN-class group: quiet and signalling, both signs, several
# payloads, and the two all-ones-mantissa patterns that are the f64 MIN / MAX identities
# (agg_init: MIN starts at +NaN 0x7FFF..., MAX at -NaN 0xFFFF... in the total order).
NF_NAN_BITS = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF4000000000123,
                        0x7FF8DEADBEEF0001, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
NF_PLAIN, NF_PINF, NF_NINF, NF_BOTH_INF, NF_NAN, NF_SUBNORMAL, NF_HUGE, NF_ZERO = range(8)
NF_ALL = tuple(range(8))
F64_MIN_NORMAL = 2.2250738585072014e-308


def nonfinite_values(rng, key, classes=NF_ALL, frac=0.3):
    """The one f64 value column of the non-finite tests: every finite sum it can produce is
    exact in any summation order, so results compare bit for bit and no tolerance is needed.

    Row i belongs to class classes[key[i] mod len(classes)] (`key`: the int64 group key, or
    an int64 array that stands in for it), so a group has exactly one class:
      NF_PLAIN      dyadic values, integers in [-4096, 4096) / 64 (exact sums);
      NF_PINF       the same with `frac` of the rows +inf            -> sum +inf;
      NF_NINF       ... -inf                                        -> sum -inf;
      NF_BOTH_INF   ... both infinities                             -> sum NaN (inf - inf);
      NF_NAN        ... NaNs of NF_NAN_BITS (both signs, payloads)  -> sum NaN;
      NF_SUBNORMAL  ONLY subnormals, integers in [-3, 9) * 5e-324: sums and MIN / MAX stay
                    exact multiples of 2^-1074, and a flush to zero shows as 0;
      NF_HUGE       ONLY +-1.5e308, one sign per group (by key): two rows overflow to that
                    sign's infinity in every order;
      NF_ZERO       ONLY -0.0 and +0.0.
    NF_SUBNORMAL and NF_HUGE are pure on purpose — order-independence: a subnormal added to
    a normal value rounds differently in different orders, and huge values of both signs (or
    huge next to plain ones) overflow or cancel depending on the order."""
    key = np.asarray(key, dtype=np.int64)
    n = len(key)
    cls = np.asarray(classes, dtype=np.int64)[key % len(classes)]
    v = rng.integers(-4096, 4096, n).astype(np.float64) / 64.0
    u = rng.random(n)
    hit = u < frac
    v[hit & (cls == NF_PINF)] = np.inf
    v[hit & (cls == NF_NINF)] = -np.inf
    both = hit & (cls == NF_BOTH_INF)
    v[both] = np.where(u[both] < frac / 2, np.inf, -np.inf)
    nan = hit & (cls == NF_NAN)
    v[nan] = NF_NAN_BITS[rng.integers(0, len(NF_NAN_BITS), int(nan.sum()))].view(np.float64)
    sub = cls == NF_SUBNORMAL
    m = rng.integers(-3, 9, n)
    bits = np.abs(m).astype(np.uint64) | np.where(m < 0, np.uint64(1) << np.uint64(63), np.uint64(0))
    v[sub] = bits.view(np.float64)[sub]
    huge = cls == NF_HUGE
    v[huge] = np.where((key[huge] // len(classes)) % 2 == 0, 1.5e308, -1.5e308)
    zero = cls == NF_ZERO
    v[zero] = np.where(u[zero] < 0.5, -0.0, 0.0)
    return v


def nonfinite_divisors(rng, key, classes=NF_ALL):
    """A divisor column for f64 `/` and fmod over nonfinite_values(rng, key, classes): positive
    powers of two (an infinity keeps its sign, so a group keeps its class), and in the groups
    whose key div len(classes) is odd also -4.0, 0.0 and -0.0: there x / 0 gives both
    infinities, 0 / 0 and fmod(x, 0) NaN.  Quotients of the plain dyadic values are exact; a
    subnormal divided by 2 or 4 rounds, so what the bit-for-bit comparison relies on there is
    correctly rounded f64 division on subnormals on both sides — every row's quotient is
    then the same, and the sums of those multiples of 2^-1074 stay exact in any order."""
    key = np.asarray(key, dtype=np.int64)
    pool = np.array([1.0, 2.0, 4.0, 0.5, -4.0, 0.0, -0.0])
    zeros = (key // len(classes)) % 2 == 1
    return pool[np.where(zeros, rng.integers(0, 7, len(key)), rng.integers(0, 4, len(key)))]


def f64_ord(x):
    """The total-order word of f64 MIN / MAX (common.hpp f64_to_ord, oracle.c f64_ord):
    -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN, payload bits significant."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | (np.uint64(1) << np.uint64(63)))


def f64_from_ord(o):
    o = np.asarray(o, dtype=np.uint64)
    b = np.where(o >> np.uint64(63) != 0, o & np.uint64(0x7FFFFFFFFFFFFFFF), ~o)
    return np.ascontiguousarray(b).view(np.float64)


def nf_check(gk, gw, ok, ow, sum_cols=(0,), what=""):
    """The non-finite comparison rule: keys, COUNT and MIN / MAX words bit-equal (NaN sign
    and payload included: MIN / MAX select an input value); SUM words bit-equal except
    where the reference sum is NaN — there only isnan(got): the sign and payload of an
    inf - inf NaN are the hardware's."""
    assert np.array_equal(gk, ok), what
    gw, ow = np.asarray(gw).view(np.uint64), np.asarray(ow).view(np.uint64)
    assert gw.shape == ow.shape, (what, gw.shape, ow.shape)
    for j in range(ow.shape[1]):
        g, o = gw[:, j], ow[:, j]
        if j in sum_cols:
            nan = np.isnan(o.view(np.float64))
            assert np.all(np.isnan(g.view(np.float64)[nan])), (what, j, "NaN sums")
            bad = np.flatnonzero((g != o) & ~nan)
            assert len(bad) == 0, (what, j, bad[:5], g[bad[:5]], o[bad[:5]])
        else:
            bad = np.flatnonzero(g != o)
            assert len(bad) == 0, (what, j, bad[:5], g[bad[:5]], o[bad[:5]])


def nf_covers_all(sum_words, what=""):
    """The reference really has groups of every kind: a NaN sum, each infinity, a non-zero
    subnormal sum and a zero sum."""
    s = np.ascontiguousarray(sum_words).view(np.float64)
    assert np.isnan(s).any(), what
    assert (s == np.inf).any() and (s == -np.inf).any(), what
    assert ((s != 0) & (np.abs(s) < F64_MIN_NORMAL)).any(), what
    assert (s == 0).any(), what


# ----------------------------------------------------------------------------- hash helpers
# (shared by join_shapes.py and groupby_shapes.py: common.hpp mix64 and its inverse)
MIX_C1, MIX_C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
INV_C1, INV_C2 = pow(MIX_C1, -1, 1 << 64), pow(MIX_C2, -1, 1 << 64)


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def mix64(z):
    z = _u64(z)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX_C1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX_C2)
    return z ^ (z >> np.uint64(31))


def unmix64(z):
    """The inverse of mix64: x ^= x >> s is undone by x ^= x >> s ^ x >> 2s (3s >= 64), the
    odd multipliers by their inverses mod 2^64."""
    z = _u64(z)
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(31)) ^ (z >> np.uint64(62))
        z = z * np.uint64(INV_C2)
        z = z ^ (z >> np.uint64(27)) ^ (z >> np.uint64(54))
        z = z * np.uint64(INV_C1)
    return z ^ (z >> np.uint64(30)) ^ (z >> np.uint64(60))


# ----------------------------------------------------------------------------- sort helpers
# (shared by test_gpu_order_by.py and test_gpu_sort_paths.py)
def dev(x, ex):
    return torch.from_numpy(np.ascontiguousarray(x)).to(ex.device)


def ukey(v, desc=False):
    """The sort's unsigned order key: int64 sign-flipped, float64 by the IEEE total order."""
    b = np.ascontiguousarray(v).view(np.uint64)
    if v.dtype == np.float64:
        u = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    else:
        u = b ^ np.uint64(1 << 63)
    return ~u if desc else u


def sort_pairs(ex, keys, desc=False, vals=None):
    from nutdb_amd._lib import T_F64, T_I64, check, lib
    n = len(keys)
    k = dev(keys, ex)
    v = dev(vals, ex) if vals is not None else None
    out = torch.empty(max(n, 1), dtype=torch.int64, device=ex.device)
    ex._bind_stream()
    check(lib.nut_sort_pairs(ex.ctx, C.c_void_p(k.data_ptr() if n else None), T_F64 if keys.dtype == np.float64 else T_I64,
                             int(desc), C.c_void_p(v.data_ptr()) if v is not None else None,
                             C.c_void_p(out.data_ptr()), n), "nut_sort_pairs")
    ex.sync()
    return out[:n].cpu().numpy()


def topk_positions(ex, keys, k, desc=False, cap=None):
    from nutdb_amd._lib import T_F64, T_I64, lib
    n = len(keys)
    d = dev(keys, ex)
    cap = n if cap is None else cap
    out = torch.empty(max(cap, 1), dtype=torch.int64, device=ex.device)
    cnt = C.c_uint64()
    ex._bind_stream()
    st = lib.nut_topk_positions(ex.ctx, C.c_void_p(d.data_ptr()), T_F64 if keys.dtype == np.float64 else T_I64,
                                1 if desc else 0, n, k, C.c_void_p(out.data_ptr()), cap, C.byref(cnt))
    ex.sync()
    return st, cnt.value, out[: cnt.value].cpu().numpy()
