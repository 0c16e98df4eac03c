// prog_ops.hpp — the one definition of the integer, calendar and exact math semantics of the nut_prog
// ops (include/nutexec.h, nut_prog_op), and of every op's arity.
//
// Compiled three ways from this one text: by hipRTC inside the generated scan kernels
// (jit.cpp's prelude brings the integer typedefs; no system header is pulled in), by hipcc
// as host + device functions, and by a plain C++ compiler as inline host functions (the
// planner folds constants with them, sql_lower.cpp; the group-output expressions,
// sql_exec_groupby.cpp; tests/c/test_prog_ops.cpp).  It depends on nutexec.h alone.
#pragma once

#include "nutexec.h"

#if defined(__HIPCC_RTC__) || defined(__HIPCC__)
// (__forceinline__ spelled out: hip_runtime.h defines it, and this header does not need that)
#define NUT_OPFN __host__ __device__ inline __attribute__((always_inline))
#else
#define NUT_OPFN inline
#endif

namespace nut {

// operands every nut_prog_op pops
NUT_OPFN int prog_arity(int op) {
  if (op <= NUT_P_F64) return 0;
  switch (op) {
    case NUT_P_NOT:
    case NUT_P_BITNOT:
    case NUT_P_ABS:
    case NUT_P_TO_F64:
    case NUT_P_LOOKUP:
    case NUT_P_MAP:
    case NUT_P_DATEPART:
    case NUT_P_TIMEPART:
    case NUT_P_DATETRUNC:
    case NUT_P_FLOOR:
    case NUT_P_CEIL:
    case NUT_P_TRUNC:
    case NUT_P_ROUND:
    case NUT_P_MATH:
    case NUT_P_SIGN:
    case NUT_P_CAST: return 1;
    case NUT_P_IF: return 3;
    default: return 2;
  }
}

// integer helpers of the expression semantics (include/nutexec.h, nut_prog_op)
NUT_OPFN int64_t jmod(int64_t a, int64_t b, bool &err) {
  if (b == 0) { err = true; return 0; }
  return b == -1 ? 0 : a % b;
}
NUT_OPFN int64_t jdiv(int64_t a, int64_t b, bool &err) {
  if (b == 0) { err = true; return 0; }
  return b == -1 ? (int64_t)(0 - (uint64_t)a) : a / b;
}
NUT_OPFN int64_t jshl(int64_t a, int64_t b) {
  return (b >= 0 && b < 64) ? (int64_t)((uint64_t)a << b) : 0;
}
NUT_OPFN int64_t jshr(int64_t a, int64_t b) {
  return (b >= 0 && b < 64) ? (a >> b) : (a < 0 ? -1 : 0);
}
NUT_OPFN int64_t jabs(int64_t a) { return a < 0 ? (int64_t)(0 - (uint64_t)a) : a; }
// ---- calendar (proleptic Gregorian; day 0 = 1970-01-01).  Every divisor is a literal: the
// compiler turns each division into multiplies and shifts (the device has no 64-bit divide).
NUT_OPFN int64_t jclamp(int64_t x, const int64_t m) { return x < -m ? -m : x > m ? m : x; }
// floor division by a positive literal g, and the remainder in [0, g)
NUT_OPFN int64_t jfdiv(int64_t a, const int64_t g) {
  const int64_t q = a / g;
  return a - q * g < 0 ? q - 1 : q;
}
NUT_OPFN int64_t jfrem(int64_t a, const int64_t g) { return a - jfdiv(a, g) * g; }
// a civil date: year = y400 + yr (y400 a multiple of 400, yr in [0, 400]), month 1-12, day
// of month 1-31; doy / mp = day and month of the year that starts on March 1
struct JDate {
  int64_t y400;
  uint32_t yr, m, d, doy, mp;
};
NUT_OPFN bool jleap(uint32_t yr) { return (yr % 4 == 0 && yr % 100 != 0) || yr % 400 == 0; }
NUT_OPFN uint32_t jmonth_days(uint32_t yr, uint32_t m) {
  return m == 2 ? (jleap(yr) ? 29u : 28u) : 30u + ((m + (m >> 3)) & 1u);
}
// civil-from-days of a clamped day number: one 64-bit division, the rest in 32 bits
NUT_OPFN JDate jcivil(int64_t d) {
  const int64_t z = d + 719468;
  const int64_t era = jfdiv(z, 146097);
  const uint32_t doe = (uint32_t)(z - era * 146097);
  const uint32_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  JDate c;
  c.doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  c.mp = (5 * c.doy + 2) / 153;
  c.d = c.doy - (153 * c.mp + 2) / 5 + 1;
  c.m = c.mp < 10 ? c.mp + 3 : c.mp - 9;
  c.y400 = era * 400;
  c.yr = yoe + (c.m <= 2 ? 1u : 0u);
  return c;
}
// days-from-civil of year y400 + yr (yr in [0, 400)), month m, day d
NUT_OPFN int64_t jdays(int64_t y400, uint32_t yr, uint32_t m, uint32_t d) {
  if (m <= 2) {  // January and February belong to the March-based year before
    if (yr == 0) y400 -= 400, yr = 399;
    else yr -= 1;
  }
  const uint32_t doy = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5 + d - 1;
  const uint32_t doe = yr * 365 + yr / 4 - yr / 100 + doy;
  return (y400 / 400) * 146097 + (int64_t)doe - 719468;
}
// P = nut_date_part.  d is clamped to +-2^40 days first, so no intermediate overflows.
NUT_OPFN int64_t jdatepart(int64_t d, const int P) {
  d = jclamp(d, 1ll << 40);
  if (P == 4) return jfrem(d + 3, 7) + 1;  // 1970-01-01 was a Thursday (4)
  if (P == 10) return jfdiv(d + 3, 7);
  const JDate c = jcivil(d);
  const int64_t y = c.y400 + (int64_t)c.yr, m = c.m;
  if (P == 0) return y;
  if (P == 1) return m;
  if (P == 2) return c.d;
  if (P == 6) return y * 100 + m;
  if (P == 7) return y * 10000 + m * 100 + c.d;
  if (P == 3) return (m - 1) / 3 + 1;
  if (P == 8) return y * 12 + m;
  if (P == 9) return y * 4 + (m - 1) / 3;
  // day of year: January / February are days 306.. of the March-based year
  return c.doy >= 306 ? (int64_t)c.doy - 305 : (int64_t)c.doy + 60 + (jleap(c.yr) ? 1 : 0);
}
// P = nut_time_part; s (seconds) is clamped to +-2^40 days first
NUT_OPFN int64_t jtimepart(int64_t s, const int P) {
  s = jclamp(s, (1ll << 40) * 86400);
  if (P == 0) return jfdiv(s, 86400);
  if (P == 1) return jfrem(s, 86400) / 3600;
  if (P == 2) return jfrem(s, 3600) / 60;
  if (P == 3) return jfrem(s, 60);
  if (P == 4) return s - jfrem(s, 60);
  if (P == 5) return s - jfrem(s, 300);
  if (P == 6) return s - jfrem(s, 900);
  if (P == 7) return s - jfrem(s, 3600);
  return s - jfrem(s, 86400);
}
// P = nut_date_trunc; a day number
NUT_OPFN int64_t jdatetrunc(int64_t d, const int P) {
  d = jclamp(d, 1ll << 40);
  if (P == 0) return d - jfrem(d + 3, 7);
  if (P == 1) return d - jfrem(d + 4, 7);
  const JDate c = jcivil(d);
  if (P == 2) return d - (int64_t)c.d + 1;
  if (P == 5) return d - (int64_t)c.d + (int64_t)jmonth_days(c.yr, c.m);
  const int64_t jan1 = c.doy >= 306 ? d - ((int64_t)c.doy - 306) : d - ((int64_t)c.doy + 59 + (jleap(c.yr) ? 1 : 0));
  if (P == 4) return jan1;
  // quarter: April, July and October start on days 31, 122 and 214 of the March-based year
  if (c.m <= 3) return jan1;
  const uint32_t q0 = c.m <= 6 ? 31u : c.m <= 9 ? 122u : 214u;
  return d - (int64_t)c.doy + (int64_t)q0;
}
// n months from day d, the day of month clamped to the target month's length
NUT_OPFN int64_t jaddmonths(int64_t d, int64_t n) {
  d = jclamp(d, 1ll << 40);
  n = jclamp(n, 1ll << 36);
  const JDate c = jcivil(d);
  const int64_t t = (c.y400 + (int64_t)c.yr) * 12 + ((int64_t)c.m - 1) + n;
  const int64_t e = jfdiv(t, 4800);  // 400 years of months
  const uint32_t r = (uint32_t)(t - e * 4800), yr = r / 12, m = r - yr * 12 + 1;
  const uint32_t md = jmonth_days(yr, m);
  return jdays(e * 400, yr, m, c.d < md ? c.d : md);
}

// ---- rounding, sign, least / greatest, casts, sqrt (include/nutexec.h: every result here is
// exactly defined, so host and device agree bit for bit).  Compiler builtins only.
NUT_OPFN uint64_t jbits(double x) {
  uint64_t u;
  __builtin_memcpy(&u, &x, 8);
  return u;
}
NUT_OPFN double jdbl(uint64_t u) {
  double x;
  __builtin_memcpy(&x, &u, 8);
  return x;
}
NUT_OPFN double jquiet(double x) { return jdbl(jbits(x) | 0x0008000000000000ull); }
NUT_OPFN double jnegnan() { return jdbl(0xFFF8000000000000ull); }
// 10^n, 0 <= n <= 18: a literal n folds to a literal (the divisions below then compile to
// multiplies and shifts, as the calendar's do)
NUT_OPFN int64_t jpow10(const int n) {
  int64_t m = 1;
  for (int i = 0; i < 18; ++i)
    if (i < n) m *= 10;
  return m;
}
// M: 0 floor, 1 ceil, 2 trunc, 3 round (half to even)
NUT_OPFN double jround0(double x, const int M) {
  return M == 0 ? __builtin_floor(x) : M == 1 ? __builtin_ceil(x) : M == 2 ? __builtin_trunc(x) : __builtin_rint(x);
}
// N digits after (N > 0) or before (N < 0) the point; every step one IEEE operation
NUT_OPFN double jroundf(double x, const int M, const int N) {
  if (x != x) return jquiet(x);
  if (N == 0) return jround0(x, M);
  const double s = (double)jpow10(N < 0 ? -N : N);  // exact: 10^18 < 2^63 and 5^18 < 2^53
  const double t = N > 0 ? x * s : x / s;
  if (t - t != 0.0) return x;  // the scaled value is not finite
  const double r = jround0(t, M);
  return N > 0 ? r / s : r * s;
}
// N < 0: to a multiple of m = 10^-N; ROUND: ties away from zero.  Wraps as the int * does.
NUT_OPFN int64_t jroundi(int64_t x, const int M, const int N) {
  if (N >= 0) return x;
  const int64_t m = jpow10(-N);
  const int64_t q = x / m, r = x - q * m;  // toward zero; r has the sign of x, |r| < m <= 10^18
  const uint64_t t = (uint64_t)(q * m);
  if (M == 0) return (int64_t)(r < 0 ? t - (uint64_t)m : t);
  if (M == 1) return (int64_t)(r > 0 ? t + (uint64_t)m : t);
  if (M == 2) return (int64_t)t;
  if (r >= 0) return (int64_t)(2 * r >= m ? t + (uint64_t)m : t);
  return (int64_t)(-2 * r >= m ? t - (uint64_t)m : t);
}
NUT_OPFN double jsqrt(double x) {
  if (x != x) return jquiet(x);
  if (x < 0.0) return jnegnan();
  return __builtin_sqrt(x);
}
NUT_OPFN int64_t jsignf(double x) { return x > 0.0 ? 1 : x < 0.0 ? -1 : 0; }
NUT_OPFN int64_t jsigni(int64_t x) { return x > 0 ? 1 : x < 0 ? -1 : 0; }
NUT_OPFN int64_t jleasti(int64_t a, int64_t b) { return b < a ? b : a; }
NUT_OPFN int64_t jgreatesti(int64_t a, int64_t b) { return b > a ? b : a; }
NUT_OPFN double jleastf(double a, double b) {
  if (a != a) return jquiet(a);
  if (b != b) return jquiet(b);
  return b < a ? b : a;
}
NUT_OPFN double jgreatestf(double a, double b) {
  if (a != a) return jquiet(a);
  if (b != b) return jquiet(b);
  return b > a ? b : a;
}
// f64 -> int64: toward zero, saturating, NaN = 0 (clamped before the conversion: no value
// reaches it that it does not define)
NUT_OPFN int64_t jtoi64(double x) {
  if (x != x) return 0;
  if (x >= 9223372036854775808.0) return (int64_t)0x7FFFFFFFFFFFFFFFll;
  if (x <= -9223372036854775808.0) return (int64_t)(-0x7FFFFFFFFFFFFFFFll - 1);
  return (int64_t)x;
}
// C = nut_cast (I64 .. U8): the low bits, sign- or zero-extended
NUT_OPFN int64_t jnarrow(int64_t v, const int C) {
  const uint64_t u = (uint64_t)v;
  if (C == 1) return (int64_t)(int32_t)(uint32_t)u;
  if (C == 2) return (int64_t)(short)(uint16_t)u;
  if (C == 3) return (int64_t)(signed char)(uint8_t)u;
  if (C == 4) return (int64_t)(uint32_t)u;
  if (C == 5) return (int64_t)(uint16_t)u;
  if (C == 6) return (int64_t)(uint8_t)u;
  return v;
}
// to binary32 (nearest even; beyond its range: +-inf) and back
NUT_OPFN double jtof32(double x) {
  if (x != x) return jquiet(x);
  return (double)(float)x;
}
NUT_OPFN double jtof32i(int64_t x) { return (double)(float)x; }

}  // namespace nut
