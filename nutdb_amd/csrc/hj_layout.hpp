// hj_layout.hpp — the hash join's table layout (join.hip), in one place for
// the kernels, the host code that sizes the table, and nut_join_layout (the host-only view
// of it that the tests build their directed inputs from): the capacity rule, the home slot
// of a key, the wrap rule of a run, and the region build's geometry.
#pragma once

#include "common.hpp"

namespace nut {

// home hash = mix64(key ^ 0x3C6EF372FE94F82A), written as the group-by's owner hash of a
// re-keyed key so the partition kernels (gpart.hpp, kx) compute the same digits; it is
// independent of the multi-GPU owner (owner_hash of the key itself)
constexpr uint64_t HJ_KX = 0x6A09E667F3BCC908ull ^ 0x3C6EF372FE94F82Aull;

// region build: the table is cut into regions of HJ_RS slots (128 KB), each built in LDS;
// a region takes at most 7/8 x HJ_RS records (it must keep empty slots), and tables of
// 2^22 .. 2^29 slots have regions (one 16-bit partition of the home hash's top bits)
constexpr uint32_t HJ_RS = 8192;
constexpr uint32_t HJ_RLIMIT = HJ_RS * 7 / 8;
constexpr int HJ_LOG2_MIN = 6, HJ_REGION_LOG2_LO = 22, HJ_REGION_LOG2_HI = 29;

// log2 of the capacity: >= 2 slots per build row, >= 64 slots
__host__ __device__ inline int hj_log2_capacity(uint64_t nb) {
  int log2c = HJ_LOG2_MIN;
  while ((1ull << log2c) < 2 * nb) ++log2c;
  return log2c;
}
__host__ __device__ inline bool hj_has_regions(int log2c) {
  return log2c >= HJ_REGION_LOG2_LO && log2c <= HJ_REGION_LOG2_HI;
}
// shift = 64 - log2(capacity): the home slot is the top bits of the home hash
__host__ __device__ __forceinline__ uint64_t hj_home_slot(int64_t k, int shift) {
  return owner_hash((uint64_t)k ^ HJ_KX, 0, 1) >> shift;
}
// runs wrap inside aligned blocks of wmask + 1 slots (a region, or the table)
__host__ __device__ __forceinline__ uint64_t hj_next_slot(uint64_t s, uint64_t wmask) {
  return (s & ~wmask) | ((s + 1) & wmask);
}

}  // namespace nut
