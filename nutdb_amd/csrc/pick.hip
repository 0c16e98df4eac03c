// pick.hip — the per-group row pick behind any / anyLast / argMin / argMax.
//
// The group-by kernels fold a value into one 64-bit word; these aggregates return a value of
// a chosen ROW of the group, and (order value, row) is a 128-bit accumulator for which
// neither LDS nor HBM has an atomic.  So the pick is two monotone 64-bit folds, each a
// streaming pass of its own over the rows:
//   1. rank + best: every row finds its group by binary search over the sorted group key
//      tuples (pick.hpp) and folds its order word into best[g] (atomicMin / atomicMax);
//   2. pick: every row whose order word equals the final best[g] folds its position into
//      pick[g] (atomicMin: ties go to the lowest position).
// order == NULL (any / anyLast) is pass 2 alone on the positions.
//
// Atomics are not one per row.  Both folds are monotone, so a lane reads the current word
// and issues the atomic only when its value improves it; and a wave whose lanes all hold one
// group (every wave of a global aggregate) reduces across the wave first and issues at most
// one atomic.
//
// Pass 1 stores every row's group index (4 B/row written, 4 B/row read by pass 2) so that
// pass 2 does not search again: measured against reading the key words and searching twice,
// it won at every group count.
#include "common.hpp"
#include "pick.hpp"

namespace nut {

// the current word of a fold.  A relaxed load: it may be served from a line this XCD's L2
// cached before another XCD's atomic changed the word (common.hpp, rmw_load).  The folds
// only ever move a word one way, so a stale word is a worse one: it can cost an atomic that
// turns out not to improve the word, never drop one that would have.
__device__ __forceinline__ uint64_t pick_peek(const unsigned long long *p) { return ld_agent((const uint64_t *)p); }

template <bool MAX>
__device__ __forceinline__ bool pick_better(uint64_t v, uint64_t cur) {
  return MAX ? v > cur : v < cur;
}
template <bool MAX>
__device__ __forceinline__ void pick_atomic(unsigned long long *p, uint64_t v) {
  if (MAX) atomicMax(p, (unsigned long long)v);
  else atomicMin(p, (unsigned long long)v);
}

// fold word u of group g into best[g] for the lanes with act (all lanes of the wave call)
template <bool MAX>
__device__ __forceinline__ void pick_fold(unsigned long long *best, uint32_t g, uint64_t u, bool act, int lane) {
  const uint64_t mask = __ballot(act);
  if (!mask) return;
  const int leader = __builtin_ctzll(mask);
  const uint32_t g0 = (uint32_t)__shfl((int)g, leader, 64);
  if (__ballot(act && g != g0) == 0) {  // one group in the wave: reduce, one atomic at most
    uint64_t v = act ? u : (MAX ? 0ull : ~0ull);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const uint64_t o = __shfl_xor(v, off, 64);
      v = pick_better<MAX>(o, v) ? o : v;
    }
    if (lane == leader && pick_better<MAX>(v, pick_peek(best + g0))) pick_atomic<MAX>(best + g0, v);
  } else if (act && pick_better<MAX>(u, pick_peek(best + g))) {
    pick_atomic<MAX>(best + g, u);
  }
}

// pass 1.  best[] starts at the fold's identity (MAX: 0, else ~0): a row whose word equals
// the identity issues no atomic and still matches best[g] in pass 2.
template <int NK, bool F64, bool MAX>
__global__ __launch_bounds__(PK_THREADS) void pick_best_kernel(const int64_t *__restrict__ rk0,
                                                               const int64_t *__restrict__ rk1,
                                                               const uint64_t *__restrict__ order, uint64_t m,
                                                               const int64_t *__restrict__ gk0,
                                                               const int64_t *__restrict__ gk1, uint64_t ng,
                                                               uint32_t *__restrict__ rank, unsigned long long *best) {
  const int lane = threadIdx.x & 63;
  for (uint64_t base = (uint64_t)blockIdx.x * PK_TILE; base < m; base += (uint64_t)gridDim.x * PK_TILE) {
    int64_t k0[PK_UNROLL], k1[PK_UNROLL];
    uint64_t w[PK_UNROLL];
#pragma unroll
    for (int j = 0; j < PK_UNROLL; ++j) {
      const uint64_t ic = min(base + (uint64_t)j * PK_THREADS + threadIdx.x, m - 1);
      k0[j] = NK >= 1 ? __builtin_nontemporal_load(rk0 + ic) : 0;
      k1[j] = NK == 2 ? __builtin_nontemporal_load(rk1 + ic) : 0;
      w[j] = __builtin_nontemporal_load(order + ic);
    }
#pragma unroll
    for (int j = 0; j < PK_UNROLL; ++j) {
      const uint64_t i = base + (uint64_t)j * PK_THREADS + threadIdx.x;
      const bool in = i < m;
      const uint32_t g = pick_find_group(gk0, gk1, NK, ng, k0[j], k1[j]);
      if (in) rank[i] = g;
      const uint64_t u = F64 ? pick_ord_f64(w[j]) : pick_ord_i64(w[j]);
      pick_fold<MAX>(best, g, u, in && g != PK_NONE, lane);
    }
  }
}

// pass 2.  MODE 0 / 1: rows whose int64 / f64 order word equals best[g] (final: written by the
// launch before this one), lowest position, their groups read from rank[]; MODE 2: every row,
// lowest position; MODE 3: every row, highest position — both search for the group here.
// pick[] starts at -1 (all bits set): the largest unsigned word for the atomicMin of
// positions, below every position for MODE 3's signed atomicMax.
template <int NK, int MODE>
__global__ __launch_bounds__(PK_THREADS) void pick_pos_kernel(const int64_t *__restrict__ rk0,
                                                              const int64_t *__restrict__ rk1,
                                                              const uint64_t *__restrict__ order, uint64_t m,
                                                              const int64_t *__restrict__ gk0,
                                                              const int64_t *__restrict__ gk1, uint64_t ng,
                                                              const uint32_t *__restrict__ rank,
                                                              const unsigned long long *__restrict__ best,
                                                              int64_t *pick) {
  constexpr bool LAST = MODE == 3;
  constexpr bool ORDER = MODE < 2;
  constexpr bool STORED = ORDER;
  const int lane = threadIdx.x & 63;
  for (uint64_t base = (uint64_t)blockIdx.x * PK_TILE; base < m; base += (uint64_t)gridDim.x * PK_TILE) {
    uint32_t gs[PK_UNROLL];
    uint64_t w[PK_UNROLL];
#pragma unroll
    for (int j = 0; j < PK_UNROLL; ++j) {
      const uint64_t ic = min(base + (uint64_t)j * PK_THREADS + threadIdx.x, m - 1);
      if (STORED) {
        gs[j] = __builtin_nontemporal_load(rank + ic);
      } else {
        const int64_t k0 = NK >= 1 ? __builtin_nontemporal_load(rk0 + ic) : 0;
        const int64_t k1 = NK == 2 ? __builtin_nontemporal_load(rk1 + ic) : 0;
        gs[j] = pick_find_group(gk0, gk1, NK, ng, k0, k1);
      }
      w[j] = ORDER ? __builtin_nontemporal_load(order + ic) : 0;
    }
#pragma unroll
    for (int j = 0; j < PK_UNROLL; ++j) {
      const uint64_t i = base + (uint64_t)j * PK_THREADS + threadIdx.x;
      const uint32_t g = gs[j];
      bool hit = i < m && g != PK_NONE;
      if (ORDER && hit) hit = (MODE == 1 ? pick_ord_f64(w[j]) : pick_ord_i64(w[j])) == best[g];
      const uint64_t mask = __ballot(hit);
      if (!mask) continue;
      const int leader = __builtin_ctzll(mask);
      const uint32_t g0 = (uint32_t)__shfl((int)g, leader, 64);
      // one group in the wave: positions ascend with the lane, so its first (LAST: last)
      // hit is the wave's pick
      const bool one = __ballot(hit && g != g0) == 0;
      const int sel = LAST ? 63 - __builtin_clzll(mask) : leader;
      if (one ? lane == sel : hit) {
        if (LAST) {
          long long *p = (long long *)pick + g;
          if ((long long)pick_peek((const unsigned long long *)p) < (long long)i) atomicMax(p, (long long)i);
        } else {
          unsigned long long *p = (unsigned long long *)pick + g;
          if (i < pick_peek(p)) atomicMin(p, (unsigned long long)i);
        }
      }
    }
  }
}

using BestFn = void (*)(const int64_t *, const int64_t *, const uint64_t *, uint64_t, const int64_t *, const int64_t *,
                        uint64_t, uint32_t *, unsigned long long *);
using PosFn = void (*)(const int64_t *, const int64_t *, const uint64_t *, uint64_t, const int64_t *, const int64_t *,
                       uint64_t, const uint32_t *, const unsigned long long *, int64_t *);

template <int NK>
static BestFn best_fn(bool f64, bool mx) {
  return f64 ? (mx ? pick_best_kernel<NK, true, true> : pick_best_kernel<NK, true, false>)
             : (mx ? pick_best_kernel<NK, false, true> : pick_best_kernel<NK, false, false>);
}
template <int NK>
static PosFn pos_fn(int mode) {
  switch (mode) {
    case 0: return pick_pos_kernel<NK, 0>;
    case 1: return pick_pos_kernel<NK, 1>;
    case 2: return pick_pos_kernel<NK, 2>;
    default: return pick_pos_kernel<NK, 3>;
  }
}

}  // namespace nut

using namespace nut;

extern "C" nut_status nut_group_pick(nut_ctx *c, const int64_t *const *row_keys, int nkeys, uint64_t m,
                                     const void *order, int order_type, int want_max,
                                     const int64_t *const *group_keys, uint64_t ng, int64_t *pick) {
  if (!c) return fail(NUT_ERR_INVALID_ARG, "nut_group_pick: NULL context");
  if (nkeys < 0 || nkeys > NUT_MAX_KEYS) return fail(NUT_ERR_INVALID_ARG, "nut_group_pick: 0 to 2 key words");
  if (nkeys == 0 && ng != 1) return fail(NUT_ERR_INVALID_ARG, "nut_group_pick: without keys there is one group");
  if (order && order_type != NUT_T_I64 && order_type != NUT_T_F64)
    return fail(NUT_ERR_INVALID_ARG, "nut_group_pick: order type (int64 or float64)");
  if (ng >= (1ull << 32)) return fail(NUT_ERR_UNSUPPORTED, "nut_group_pick: 2^32 groups or more");
  if (ng == 0) return NUT_OK;
  if (!pick) return fail(NUT_ERR_INVALID_ARG, "nut_group_pick: NULL output");
  const int64_t *rk[NUT_MAX_KEYS] = {nullptr, nullptr}, *gk[NUT_MAX_KEYS] = {nullptr, nullptr};
  for (int j = 0; j < nkeys; ++j) {
    if (!group_keys || !group_keys[j] || (m && (!row_keys || !row_keys[j])))
      return fail(NUT_ERR_INVALID_ARG, "nut_group_pick: NULL key column");
    gk[j] = group_keys[j];
    rk[j] = m ? row_keys[j] : nullptr;
  }
  DeviceGuard g(c->device);
  hipStream_t st = c->stream;
  NUT_HIP(hipMemsetAsync(pick, 0xFF, ng * 8, st));  // -1: no row
  if (m == 0) {
    NUT_HIP(hipStreamSynchronize(st));
    return NUT_OK;
  }
  const unsigned grid = (unsigned)std::min<uint64_t>((m + PK_TILE - 1) / PK_TILE, (uint64_t)c->num_cus * 8);
  unsigned long long *best = nullptr;
  uint32_t *rank = nullptr;
  if (order) {
    if (hipMallocAsync((void **)&best, ng * 8, st) != hipSuccess) {
      (void)hipGetLastError();
      return fail(NUT_ERR_OOM, "nut_group_pick: hipMallocAsync (best words)");
    }
    if (hipMallocAsync((void **)&rank, m * 4, st) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFreeAsync(best, st);
      return fail(NUT_ERR_OOM, "nut_group_pick: hipMallocAsync (row ranks)");
    }
  }
  auto done = [&](hipError_t e, const char *what) -> nut_status {
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (rank) (void)hipFreeAsync(rank, st);
    if (best) (void)hipFreeAsync(best, st);
    return e == hipSuccess ? NUT_OK : hip_fail(e, what);
  };
  if (order) {
    const bool f64 = order_type == NUT_T_F64, mx = want_max != 0;
    hipError_t e = hipMemsetAsync(best, mx ? 0x00 : 0xFF, ng * 8, st);
    if (e != hipSuccess) return done(e, "nut_group_pick: hipMemsetAsync");
    const BestFn bf = nkeys == 0 ? best_fn<0>(f64, mx) : nkeys == 1 ? best_fn<1>(f64, mx) : best_fn<2>(f64, mx);
    c->timer.begin(st, NUT_KERNEL_AGGREGATE);
    hipLaunchKernelGGL(bf, dim3(grid), dim3(PK_THREADS), 0, st, rk[0], rk[1], (const uint64_t *)order, m, gk[0], gk[1],
                       ng, rank, best);
    c->timer.end(st);
    e = hipGetLastError();
    if (e != hipSuccess) return done(e, "nut_group_pick: rank + best launch");
  }
  const int mode = order ? (order_type == NUT_T_F64 ? 1 : 0) : (want_max ? 3 : 2);
  const PosFn pf = nkeys == 0 ? pos_fn<0>(mode) : nkeys == 1 ? pos_fn<1>(mode) : pos_fn<2>(mode);
  c->timer.begin(st, NUT_KERNEL_AGGREGATE);
  hipLaunchKernelGGL(pf, dim3(grid), dim3(PK_THREADS), 0, st, rk[0], rk[1], (const uint64_t *)order, m, gk[0], gk[1], ng,
                     (const uint32_t *)rank, (const unsigned long long *)best, pick);
  c->timer.end(st);
  return done(hipGetLastError(), "nut_group_pick: pick launch");
}
