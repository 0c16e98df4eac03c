// pick.hpp — the host + device functions of the per-group row pick (pick.hip, DESIGN.md
// §3.14): where a row's key tuple stands in the sorted group list, and the two maps that
// turn an order value into an unsigned word whose integer order is the order asked for.
//
// Compiled two ways from this one text: by hipcc as host + device functions, and by a plain
// C++ compiler as inline host functions (tests/test_pick_cpu.py).  It depends on <stdint.h>
// alone.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define NUT_PICKFN __host__ __device__ inline __attribute__((always_inline))
#else
#define NUT_PICKFN inline
#endif

namespace nut {

// launch shape of both kernels: threads per workgroup, rows per thread and step
constexpr int PK_THREADS = 256;
constexpr int PK_UNROLL = 4;
constexpr int PK_TILE = PK_THREADS * PK_UNROLL;  // rows a workgroup takes per step
constexpr uint32_t PK_NONE = 0xFFFFFFFFu;        // the group index of a row in no group

// int64 order value -> unsigned word (sign bit flipped)
NUT_PICKFN uint64_t pick_ord_i64(uint64_t b) { return b ^ 0x8000000000000000ull; }
// f64 bits -> unsigned word in the IEEE total order (common.hpp's f64_to_ord, restated so
// that this header stands alone): -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN
NUT_PICKFN uint64_t pick_ord_f64(uint64_t b) { return (b >> 63) ? ~b : (b | 0x8000000000000000ull); }

// The first of ng tuples (g0[i], g1[i]) that is not below (k0, k1), or ng.  Tuples compare
// as signed int64 words, word 0 first (the order nut_groups_to_host returns groups in);
// nkeys = 1 reads g0 alone, nkeys = 0 nothing (empty tuples: 0).  The tuples must ascend.
NUT_PICKFN uint64_t pick_lower_bound(const int64_t *g0, const int64_t *g1, int nkeys, uint64_t ng, int64_t k0,
                                     int64_t k1) {
  uint64_t lo = 0, hi = nkeys ? ng : 0;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    const int64_t a0 = g0[mid];
    const bool below = a0 < k0 || (nkeys == 2 && a0 == k0 && g1[mid] < k1);
    if (below) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the index of the group whose tuple equals (k0, k1), or PK_NONE; nkeys = 0: one group, 0.
// ng < 2^32.
NUT_PICKFN uint32_t pick_find_group(const int64_t *g0, const int64_t *g1, int nkeys, uint64_t ng, int64_t k0,
                                    int64_t k1) {
  if (nkeys == 0) return 0;
  const uint64_t i = pick_lower_bound(g0, g1, nkeys, ng, k0, k1);
  if (i < ng && g0[i] == k0 && (nkeys < 2 || g1[i] == k1)) return (uint32_t)i;
  return PK_NONE;
}

}  // namespace nut
