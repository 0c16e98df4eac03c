// gb_layout.hpp — the group-by tables' layout arithmetic (agg_kernel.hpp, gtable.hpp,
// gpart.hpp, aggregate.hip), in one place for the kernels (compiled and
// run-time compiled), the host code that sizes tables and launches, and nut_groupby_layout
// (the host-only view of it that the tests build their directed inputs from): slot words
// and home buckets of the on-chip table, its capacity and admission limit, the
// private-accumulator decision, the global table's hash, capacity, limits and shards, the
// streaming launch's threads and workgroups, and the partition digit.
#pragma once

#include "common.hpp"

namespace nut {

// ------------------------------------------------------------------ on-chip (LDS) table
constexpr int kPrivMax = 8;        // private groups per thread (upper bound)
constexpr uint32_t kDirect = 256;  // direct-map entries (PRIV): key < 256, or 16 x 16 key pairs
constexpr uint32_t kBucket = 4;    // home bucket (4 slots, 32-B aligned) of a slot word
constexpr int kBdShared = 512;     // threads of a shared-table workgroup
constexpr int kBdPriv = 256;       //   of a private-accumulator workgroup (compiled kernels)
constexpr int kBdPrivTuned = 192, kPrivTunedBlocks = 2;  // run-time compiled private kernels
constexpr size_t kAggLdsMax = 160 * 1024 - 2048;  // the kernel also holds static LDS (spill cursor, histogram)

// Layout (dynamic LDS, this order, 16-B aligned):
//   slot[cap+1] u64 | agg[na][cap+1] u64 | k12[cap+1] {i64,i64} (NK=2) | did[cap+1] u32
//   (PRIV) | dslot[kPrivMax] u32 + dmap[kDirect] u32 (PRIV) | ctl[4] u32 | priv[P][na][BD] u64 (PRIV)
__host__ __device__ inline size_t lds_layout(uint32_t cap, int nk, int na, bool privm, int P, int bd,
                                             size_t *o_k12, size_t *o_did, size_t *o_dslot, size_t *o_ctl,
                                             size_t *o_priv) {
  const size_t stride = cap + 1;
  size_t o = stride * 8 * (1 + (size_t)na);
  o = (o + 15) & ~size_t(15);
  *o_k12 = o;
  if (nk == 2) o += stride * 16;
  *o_did = o;
  if (privm) o += stride * 4;
  *o_dslot = o;
  if (privm) o += (kPrivMax + kDirect) * 4;
  *o_ctl = o;
  o += 16;
  o = (o + 15) & ~size_t(15);
  *o_priv = o;
  if (privm) o += (size_t)P * na * bd * 8;
  return (o + 15) & ~size_t(15);
}
// LDS bytes of a table with `cap` slots (+1 special); 0 slots: no table
__host__ __device__ inline size_t lds_bytes(uint32_t cap, int nk, int na, bool priv, int P, int bd) {
  if (cap == 0) return 0;
  size_t a, b, c, d, e;
  return lds_layout(cap, nk, na, priv, P, bd, &a, &b, &c, &d, &e);
}

// slot word of a key: the key itself (one key) or a 64-bit hash nudged off the empty
// marker (two keys; the tuple is verified against k12)
template <int NK>
__host__ __device__ __forceinline__ uint64_t lkey(uint64_t k1, uint64_t k2) {
  if (NK == 1) return k1;
  uint64_t h = k1 * kGolden ^ ((k2 + 0x632BE59BD9B4E019ull) * 0xC2B2AE3D27D4EB4Full);
  h ^= h >> 29;
  return h == kEmpty ? h ^ 1ull : h;
}
// on-chip table home: Fibonacci hash of the xor-folded key (3 VALU ops; the table has
// at most 2^15 slots, so 32 product bits are plenty)
__host__ __device__ __forceinline__ uint32_t lhome(uint64_t w, int log2cap) {
  const uint32_t f = (uint32_t)w ^ (uint32_t)(w >> 32);
  return ((f * 0x9E3779B1u) >> (32 - log2cap)) & ~(kBucket - 1);
}
// direct-map index of a key (tuple), or kDirect when it is out of the map's range
template <int NK>
__host__ __device__ __forceinline__ uint32_t direct_idx(uint64_t k1, uint64_t k2) {
  if (NK == 1) return k1 < kDirect ? (uint32_t)k1 : kDirect;
  return (k1 | k2) < 16 ? (uint32_t)(k1 << 4 | k2) : kDirect;
}

// the on-chip table of a launch: `slots_per_group` x the expected groups (4: load <= 1/4, a
// key almost always sits in its 4-slot home bucket) within the LDS budget, 4096 slots
// without a hint.  0: hot keys cannot fit on chip
// (32 slots = 8 buckets x 32 B = one pass over the 64 LDS banks: for <= 8 groups two
// home buckets never conflict — distinct buckets hit distinct banks, equal ones broadcast)
__host__ __device__ inline uint32_t gb_lds_cap(int nk, int na, uint64_t group_hint, uint64_t slots_per_group) {
  const uint64_t want = group_hint ? slots_per_group * group_hint : 4096;
  uint32_t lcap = 32;
  while (lcap < want && lds_bytes(lcap * 2, nk, na, false, 0, kBdShared) <= kAggLdsMax) lcap *= 2;
  return group_hint > 8ull * lcap ? 0 : lcap;
}
// claims the block table admits before it closes (its rows then go to the global table)
__host__ __device__ inline uint32_t gb_lds_limit(uint32_t lcap) { return lcap - lcap / 4; }
// private accumulators when every expected group fits P per thread, 2 blocks per CU
__host__ __device__ inline int gb_priv_groups(uint32_t lcap, int nk, int na, uint64_t group_hint, bool seg) {
  int P = 0;
  if (lcap && group_hint && group_hint <= (uint64_t)kPrivMax && na > 0 && !seg) {
    P = (int)group_hint;
    if (lds_bytes(lcap, nk, na, true, P, kBdPriv) > kAggLdsMax / 2) P = 0;
  }
  return P;
}

// ------------------------------------------------------------------ the streaming launch
// threads: shared tables 512, private accumulators 256, or `tuned_bd` for the kernels built
// for several sizes (the compiled Q1 shape, every run-time compiled kernel)
__host__ __device__ inline int gb_threads(bool priv, bool tuned, int tuned_bd) {
  return !priv ? kBdShared : !tuned ? kBdPriv : tuned_bd;
}
// workgroups per CU: as many as `lb` LDS bytes allow, at most 4 (512 threads) or 8; the tuned
// private kernels at most `tuned_blocks`, shared tables at most `agg_blocks` (0: no cap)
__host__ __device__ inline int gb_blocks_per_cu(size_t lb, int bd, bool priv, bool tuned, int tuned_blocks,
                                                int agg_blocks) {
  const size_t most = bd == 512 ? 4 : 8;
  size_t fit = lb ? kAggLdsMax / lb : 4;
  if (lb && fit > most) fit = most;
  if (lb && fit < 1) fit = 1;
  int b = (int)fit;
  if (tuned && tuned_blocks < b) b = tuned_blocks;
  if (!priv && agg_blocks && agg_blocks < b) b = agg_blocks;
  return b;
}
// grid: the chip filled, or one lane per row pair if that is fewer workgroups
__host__ __device__ inline uint64_t gb_grid(int num_cus, int blocks_per_cu, uint64_t n, int bd) {
  const uint64_t pairs = (n + 1) / 2, fill = (uint64_t)num_cus * blocks_per_cu, need = (pairs + bd - 1) / bd;
  const uint64_t blocks = fill < need ? fill : need;
  return blocks ? blocks : 1;
}

// ------------------------------------------------------------------ global (HBM) table
// hash of the key tuple: single key -> the key itself is the slot word; two keys ->
// 64-bit mix (tag = high half, slot from multiply-shift)
template <int NK>
__host__ __device__ __forceinline__ uint64_t key_hash(int64_t k1, int64_t k2) {
  return NK == 1 ? (uint64_t)k1 : mix64((uint64_t)k1 ^ mix64((uint64_t)k2 + kGolden));
}
// multiply-shift slot index
__host__ __device__ __forceinline__ uint32_t slot_of(uint64_t fp, int log2cap) {
  return (uint32_t)((fp * kGolden) >> (64 - log2cap));
}
// slots of a table for `groups` groups: load <= 1/2, 1024 slots at least
__host__ __device__ inline uint64_t table_cap_for(uint64_t groups) {
  uint64_t cap = 1024;
  while (cap < 2 * groups) cap *= 2;
  return cap;
}
// Claim and arena limits of a table of `cap` slots.  Tables of 2^18 slots and more count
// claims and arena entries in 256 shards (claims: by the slot's low bits, arena: by the
// tag's), so that inserts do not all hit one address; a shard's claim limit is the claims
// of a uniformly hashed 1/nsh of the slots, +1/16 for variance.  Two-key arena: one entry
// per claimable slot plus slack for claim races lost by concurrent inserters of the same
// key (each loser leaks at most one entry).
struct GbTableRule {
  uint32_t limit, limit_sh, arena_cap, arena_sh;
  int nsh_log2;
  uint64_t arena;  // entries allocated (arena_cap, unclamped)
};
__host__ __device__ inline GbTableRule gb_table_rule(uint64_t cap, int nk) {
  GbTableRule r;
  r.arena = nk == 2 ? cap + 65536 : 0;
  r.nsh_log2 = cap >= (1ull << 18) ? 8 : 0;
  const uint32_t nsh = 1u << r.nsh_log2;
  const uint64_t lim = cap - cap / 4;
  r.limit = (uint32_t)(lim < 0xFFFFFFF0ull ? lim : 0xFFFFFFF0ull);
  r.arena_cap = (uint32_t)(r.arena < 0xFFFFFFF0ull ? r.arena : 0xFFFFFFF0ull);
  r.limit_sh = nsh == 1 ? r.limit : r.limit / nsh + r.limit / nsh / 16;
  r.arena_sh = r.arena_cap / nsh;
  return r;
}
// shards of a table; a claim counts in the shard of its slot's low bits, an arena entry in
// the shard of its tag's low bits
__host__ __device__ __forceinline__ uint32_t gb_shards(int nsh_log2) { return 1u << nsh_log2; }
__host__ __device__ __forceinline__ uint32_t gb_claim_shard(uint64_t slot, int nsh_log2) {
  return (uint32_t)(slot & (gb_shards(nsh_log2) - 1));
}
__host__ __device__ __forceinline__ uint32_t gb_arena_shard(uint32_t tag, int nsh_log2) {
  return tag & (gb_shards(nsh_log2) - 1);
}

// ------------------------------------------------------------------ partitioned group-by
// a level's digit: 8 bits (or fewer: shift = 64 - bits at level 0) of owner_hash(k ^ kx);
// the group-by partitions with kx = 0, the join with its own (hj_layout.hpp)
__host__ __device__ __forceinline__ uint32_t gb_digit(uint64_t k1, uint64_t k2, int nk, int shift, uint64_t kx) {
  return (uint32_t)(owner_hash(k1 ^ kx, k2, nk) >> shift) & 255u;
}
// level 0's digit bits of the hashed (direct, optimistic) path: 7 for one level up to
// 150 K groups, else 8; `opt_bits` >= 6 overrides
__host__ __device__ inline int gb_l0_bits(int levels, uint64_t group_hint, int opt_bits) {
  return opt_bits >= 6 ? opt_bits : levels == 1 && group_hint <= 150000 ? 7 : 8;
}
__host__ __device__ inline int gb_levels(uint64_t group_hint, int opt_levels) {
  return opt_levels ? opt_levels : group_hint > 256ull * 1024 ? 2 : 1;
}

}  // namespace nut
