// go_plan.hpp — the host's plan of the ordered group-by (aggregate.hip groupby_ordered,
// DESIGN.md §4.2c): the key range from the sample, the admission test, the heavy keys and
// their cuckoo table, the buffer sizes, both levels' regions (capped and exact), the chunks
// with their tile tables, and the heavy keys' partitions — free functions over plain structs
// and vectors, so that tests/test_go_plan_cpu.py runs every branch without a GPU.
//
// Compiled two ways from this one text: by hipcc (gpart.hpp and heavy.hpp include it: the
// kernels share GpRange::cell and hk_slot), and by a plain C++ compiler as host functions.
// It depends on the standard library and nutexec.h's decline reasons alone.
#pragma once

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "nutexec.h"

#if defined(__HIPCC__)
#define NUT_GOFN __host__ __device__ inline __attribute__((always_inline))
#else
#define NUT_GOFN inline
#endif

namespace nut {

constexpr int GP_THREADS = 512;
constexpr int GP_ITEMS = 16;
constexpr uint32_t GP_TILE = GP_THREADS * GP_ITEMS;  // 8192 records per scatter tile

struct GpSeg {  // records [start, start + count) of the current buffer
  uint64_t start, count;
  uint32_t tile0, pad;  // first tile of the segment in the launch's tile table
  // capped layout (no histogram pass): digit d of this segment owns output rows
  // [obase + d * ocap, obase + (d + 1) * ocap)
  uint64_t obase = 0, ocap = 0;
};

// Range digits (the ordered group-by, aggregate.hip groupby_ordered): keys mapped
// monotonically onto 2^14 cells over a sampled range [lo, lo + span] (signed order; keys
// outside are clamped to the end cells, so the order holds and only the balance suffers):
// x = (k ^ 2^63) - lo, clamped to [0, span]; cell = mulhi((x >> t), mul) with mul =
// floor(2^46 / ((span >> t) + 1)).  With the cells split into bits0 + bits1 digits
// (NUT_OPT_GB_L0_BITS, default 7 + 7), level 0's digit is cell >> bits1 and level 1's
// cell & (2^bits1 - 1), so the partitions are in key order.  (The scatter kernel's RANGE
// template flag chooses these digits over the hash's; t is the range shift, 0 included.)
struct GpRange {
  uint64_t lo, span;
  uint32_t mul;
  int t;  // x's shift: (span >> t) < 2^32
  NUT_GOFN uint32_t cell(uint64_t k) const {
    uint64_t x = (k ^ 0x8000000000000000ull) - lo;
    x = (k ^ 0x8000000000000000ull) < lo ? 0 : (x > span ? span : x);
    return (uint32_t)(((uint64_t)(uint32_t)(x >> t) * mul) >> 32);  // (v_mul_hi_u32)
  }
};
constexpr uint32_t GO_CELLS = 1u << 14;

inline uint32_t gp_tiles(std::vector<GpSeg> &segs, uint32_t tile, std::vector<uint32_t> &ts) {
  ts.clear();
  for (uint32_t i = 0; i < segs.size(); ++i) {
    segs[i].tile0 = (uint32_t)ts.size();
    ts.insert(ts.end(), (segs[i].count + tile - 1) / tile, i);
  }
  return (uint32_t)ts.size();
}

// common.hpp's mix64, restated so that this header stands alone
NUT_GOFN uint64_t go_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ------------------------------------------------------------ heavy keys (heavy.hpp)
constexpr int HK_THREADS = 256, HK_ITEMS = 8;
constexpr uint32_t HK_TILE = HK_THREADS * HK_ITEMS;  // rows per tile
constexpr int HK_MAX = 2048;                         // heavy keys at most
constexpr int HK_SLOTS = 8192;                       // cuckoo slots (load <= 1/4), host-built
constexpr int HK_WORDS = 2048;                       // heavy keys x aggregates at most (16 KB)

// a key's two cuckoo slots (the host places every heavy key in one of them: hk_cuckoo)
NUT_GOFN uint32_t hk_slot(uint64_t k, uint64_t seed) {
  return (uint32_t)(go_mix64(k ^ seed) >> 32) & (HK_SLOTS - 1);
}

// host: a cuckoo table of the h keys (slot = key index + 1); false if some key found no
// place (the caller retries with other seeds)
inline bool hk_cuckoo(const int64_t *hk, uint32_t h, uint64_t s1, uint64_t s2, uint16_t *slot) {
  for (int i = 0; i < HK_SLOTS; ++i) slot[i] = 0;
  for (uint32_t j = 0; j < h; ++j) {
    uint16_t cur = (uint16_t)(j + 1);
    uint32_t pos = hk_slot((uint64_t)hk[j], s1);
    int steps = 0;
    for (;;) {
      const uint16_t old = slot[pos];
      slot[pos] = cur;
      if (!old) break;
      if (++steps > 1000) return false;
      cur = old;  // the evicted key moves to its other slot
      const uint64_t k = (uint64_t)hk[old - 1];
      const uint32_t a = hk_slot(k, s1), b = hk_slot(k, s2);
      pos = pos == a ? b : a;
    }
  }
  return true;
}

// ------------------------------------------------------------ the plan
// Every function that can decline returns the reason (NUT_GB_DECLINE_*), 0 if it does not.
constexpr uint32_t kGoSample = 65536;  // keys in the strided sample

// the key range from a strided sample (+ 1/1024 of the span on either side)
inline uint32_t go_range(int64_t smin, int64_t smax, GpRange *rg) {
  uint64_t lo = (uint64_t)smin ^ 0x8000000000000000ull, hi = (uint64_t)smax ^ 0x8000000000000000ull;
  const uint64_t margin = (hi - lo) >> 10;
  lo = lo > margin ? lo - margin : 0;
  hi = hi < ~0ull - margin ? hi + margin : ~0ull;
  *rg = GpRange{};
  rg->lo = lo;
  rg->span = hi - lo;
  if (rg->span < (1ull << 16)) return NUT_GB_DECLINE_SHAPE;  // (mul must fit 32 bits; tiny spans hash fine)
  rg->t = rg->span >> 32 ? 32 - __builtin_clzll(rg->span) : 0;
  rg->mul = (uint32_t)((1ull << 46) / ((rg->span >> rg->t) + 1));
  return 0;
}

// the sample's keys counted in an open-addressing table (2x the sample): distinct keys
// for the admission, repeated ones for the heavy-key split (a sort of the 64 Ki keys took
// milliseconds of host time ahead of every call's first kernel)
struct GoSample {
  static constexpr uint32_t kSlots = 2 * kGoSample;
  std::vector<int64_t> tk;
  std::vector<uint32_t> tc;  // (0: an empty slot)
};
inline void go_sample_table(const std::vector<int64_t> &smp, GoSample *t) {  // (<= kGoSample keys)
  constexpr uint32_t kSlots = GoSample::kSlots;
  t->tk.assign(kSlots, 0);
  t->tc.assign(kSlots, 0);
  for (int64_t k : smp) {
    uint32_t q = (uint32_t)(go_mix64((uint64_t)k) >> 32) & (kSlots - 1);
    while (t->tc[q] && t->tk[q] != k) q = (q + 1) & (kSlots - 1);
    t->tk[q] = k;
    ++t->tc[q];
  }
}

// admission: the sample's distinct keys spread over the level-0 partitions.  Keys
// clustered inside the sampled range would overfill some partitions' tables (each
// holds ~2x its share of groups) and send the call to the hashed path after all the
// work; decline up front instead.  Repeated keys count once: a heavy key is rows,
// not groups (the heavy-key split or the overflow arenas below take its rows).
inline uint32_t go_admit(const GoSample &t, const GpRange &rg, int bits0) {
  const int bits1 = 14 - bits0;
  const uint32_t np0 = 1u << bits0, bound = 2 * kGoSample / np0 + 16;
  std::vector<uint32_t> distinct(np0, 0);
  for (uint32_t q = 0; q < GoSample::kSlots; ++q)
    if (t.tc[q]) ++distinct[rg.cell((uint64_t)t.tk[q]) >> bits1];
  for (uint32_t p = 0; p < np0; ++p)
    if (distinct[p] > bound) return NUT_GB_DECLINE_CLUSTERED;
  return 0;
}

// ---- heavy keys (heavy.hpp): a key the sample saw >= 3 times (expected rows >= ~1/22000
// of the rows, most of a level-1 partition's share; a key of twice that share is still
// sampled < 3 times one time in ten) would overflow its partition.  When such keys
// hold >= 5 % of the sample, the <= HK_MAX most frequent are aggregated in one streaming
// pass and the other rows, compacted into B2, are what the levels partition.
struct GoHeavy {
  std::vector<int64_t> keys;   // ascending; empty: no heavy pass
  std::vector<uint16_t> slot;  // [HK_SLOTS] the pass's cuckoo table
  uint64_t seed1 = 0, seed2 = 0;
};
inline void go_heavy_keys(const GoSample &t, int na, GoHeavy *h) {
  std::vector<std::pair<uint32_t, int64_t>> cand;  // (sample count, key)
  for (uint32_t q = 0; q < GoSample::kSlots; ++q)
    if (t.tc[q] >= 3) cand.emplace_back(t.tc[q], t.tk[q]);
  std::sort(cand.begin(), cand.end(), [](const auto &x, const auto &y) {
    return x.first > y.first || (x.first == y.first && x.second < y.second);
  });
  const size_t hmax = std::min<size_t>(HK_MAX, HK_WORDS / na);
  if (cand.size() > hmax) cand.resize(hmax);
  uint64_t cover = 0;
  for (const auto &x : cand) cover += x.first;
  if (cover * 20 >= kGoSample) {
    for (const auto &x : cand) h->keys.push_back(x.second);
    std::sort(h->keys.begin(), h->keys.end());
    // the pass's lookup table: a cuckoo table (two slots per key) built here, so every
    // lookup is two reads; new seeds if a key finds no place (at load <= 1/4, rare)
    h->slot.assign(HK_SLOTS, 0);
    bool placed = false;
    for (uint64_t attempt = 0; attempt < 8 && !placed; ++attempt) {
      h->seed1 = go_mix64(0x9E3779B97F4A7C15ull + 2 * attempt);
      h->seed2 = go_mix64(0x9E3779B97F4A7C15ull + 2 * attempt + 1);
      placed = hk_cuckoo(h->keys.data(), (uint32_t)h->keys.size(), h->seed1, h->seed2, h->slot.data());
    }
    if (!placed) h->keys.clear();  // (the overflow arenas take them)
  }
}

// the heavy pass's grid: workgroup b reads tiles [b chunk, (b + 1) chunk) (per_cu: the
// occupancy query's workgroups per CU)
struct GoHeavyGrid {
  uint64_t ntiles, hgrid, chunk;
};
inline uint32_t go_heavy_grid(uint64_t n, int num_cus, int per_cu, GoHeavyGrid *hg) {
  hg->ntiles = (n + HK_TILE - 1) / HK_TILE;
  hg->hgrid = std::min<uint64_t>(hg->ntiles, (uint64_t)num_cus * per_cu);
  hg->chunk = (hg->ntiles + hg->hgrid - 1) / hg->hgrid;
  if (hg->chunk * HK_TILE * 8 >= (1ull << 32)) return NUT_GB_DECLINE_CAPACITY;  // (a chunk's buffer resource)
  return 0;
}

// ---- partition buffers: level 0 capped over O (2 x rows per array), level 1 into B2
struct GoSizes {
  bool exact;
  double slack1;
  uint64_t rows, arena1, b2rows;
  uint64_t ocap, abase0, acap0;  // level 0's capped regions and its arena, rows of O
  size_t data_bytes;             // gp_data
};
// heavy: heavy keys were chosen; keep_capped: NUT_OPT_GB_HEAVY = 2; nstore: stored arrays
// (the key and the value columns)
inline GoSizes go_sizes(uint64_t n, int bits0, int nstore, double lam, bool heavy, bool keep_capped) {
  const int bits1 = 14 - bits0;
  GoSizes z{};
  z.rows = (n + 2 * 65536 + 64 + 31) & ~31ull;
  // Exact layout (heavy keys split off): the data is skewed below the heavy keys too
  // (Zipf-like: keys of ~1/2 to 2 partition shares remain), so the heavy pass's kept rows are
  // counted per range cell (go_cell_hist_kernel, 8 B per kept row) and both levels' regions
  // are laid out from the counts — no overflow, no arenas, no arena group-by or host fold.
  // NUT_OPT_GB_HEAVY = 2 keeps the capped layout behind the heavy pass (A/B, tests).
  z.exact = heavy && !keep_capped;
  // capped level-1 regions: the even share x slack1 (six standard deviations of a Poisson
  // count of lambda keys per partition); behind the heavy pass 2.5 x (1e9-row Zipf G = 1e7:
  // 62 M arena rows at 1.24 x)
  z.slack1 = z.exact ? 1.0 : !heavy ? 1.0 + 6.0 / sqrt(lam) : 2.5;
  // B2: the level-1 regions (n x slack1 + per-region slack), then level 1's overflow arena
  // (n / 2 rows, n / 4 with the wider regions, none exact), then one tile of scratch for
  // runs an exhausted arena cannot take
  z.arena1 = ((z.exact ? 0 : !heavy ? n / 2 : n / 4) + 31) & ~31ull;
  z.b2rows = ((uint64_t)ceil(n * z.slack1) + (66ull << (bits0 + bits1)) + z.arena1 + 2 * GP_TILE + 64 + 31) & ~31ull;
  z.data_bytes = (2 * (size_t)nstore * z.rows + (size_t)nstore * z.b2rows) * 8 + 256;
  // ---- level 0 (range digit = cell >> bits1): 1.5 x the even share per partition, the rest
  // of O (~n / 2 rows) its arena
  z.ocap = ((3 * z.rows / 2) >> bits0) & ~1ull;
  z.abase0 = z.ocap << bits0;
  z.acap0 = 2 * z.rows - z.abase0 - 2 * GP_TILE;
  return z;
}

// level 0: its input segments, and its non-empty partitions p0 ([start, end) pairs of O)
// with their digits dig0
struct GoLevel0 {
  std::vector<GpSeg> segs;
  std::vector<uint64_t> p0;
  std::vector<uint32_t> dig0;  // the level-0 digit of each non-empty level-0 partition
  // exact: level 0 is launched after the metadata upload (its layout is known before)
  std::vector<uint32_t> ts0;
  std::vector<uint64_t> cur0;
};
// hcount (heavy pass: the rows each workgroup kept, at hchunk-row strides of B2); empty: no
// heavy pass, the n input rows
inline void go_l0_segs(uint64_t n, const std::vector<uint64_t> &hcount, uint64_t hchunk, uint64_t ocap,
                       std::vector<GpSeg> *segs) {
  if (hcount.empty()) {
    segs->push_back(GpSeg{0, n, 0, 0});
  } else {  // the heavy pass's per-workgroup runs, gathered into one set of regions
    for (size_t b = 0; b < hcount.size(); ++b)
      if (hcount[b]) segs->push_back(GpSeg{b * hchunk, hcount[b], 0, 0});
    if (segs->empty()) segs->push_back(GpSeg{0, 0, 0, 0});
  }
  for (GpSeg &sg : *segs) sg.ocap = ocap;
}
// capped: p0 is what the scatter's cursors gave (gp_level); region d starts at row d * ocap
inline void go_l0_capped(uint64_t ocap, GoLevel0 *l) {
  for (size_t i = 0; i < l->p0.size(); i += 2) l->dig0.push_back((uint32_t)(l->p0[i] / ocap));
}
// exact: from the kept rows per range cell
inline uint32_t go_l0_exact(const std::vector<uint64_t> &cells, int bits0, uint64_t rows, GoLevel0 *l) {
  const int bits1 = 14 - bits0;
  const uint32_t nb0 = 1u << bits0, nb1 = 1u << bits1;
  // digit d's rows start at a 32-row boundary of O after digit d - 1's (256-B aligned)
  l->cur0.assign(nb0 + 1, 0);  // + the (unused) overflow flag
  uint64_t at = 0;
  for (uint32_t d = 0; d < nb0; ++d) {
    uint64_t cnt = 0;
    for (uint32_t q = 0; q < nb1; ++q) cnt += cells[(d << bits1) | q];
    l->cur0[d] = at;
    if (cnt) {
      l->p0.push_back(at);
      l->p0.push_back(at + cnt);
      l->dig0.push_back(d);
    }
    at = (at + cnt + 31) & ~31ull;
  }
  if (at + 2 * GP_TILE > 2 * rows) return NUT_GB_DECLINE_CAPACITY;
  for (GpSeg &sg : l->segs) sg.ocap = 0;
  gp_tiles(l->segs, 2 * GP_TILE, l->ts0);
  return 0;
}

// level 1, the chunks it runs in, and what the aggregation and the heavy keys need of it
struct GoLevel1 {
  std::vector<GpSeg> s2;  // one segment per level-0 partition
  uint64_t ovf1 = 0;      // the regions' end: level 1's arena is rows [ovf1, ovf1 + acap1) of B2
  uint64_t acap1 = 0;
  uint64_t nparts = 0;                     // final partitions, np0 << bits1
  std::vector<uint32_t> cb;                // chunk j: level-0 partitions [cb[j], cb[j + 1])
  std::vector<uint32_t> tiles, tile0, ntile;  // chunk j's tile table: tiles[tile0[j] .. + ntile[j])
  std::vector<uint64_t> init, rend;        // final partition q's region [init[q], rend[q]) (init: + one overflow flag per chunk)
  std::vector<int64_t> hq;                 // each heavy key's final partition, or -1
  uint32_t nch() const { return (uint32_t)cb.size() - 1; }
};
// ---- level-1 regions, as the hashed path sizes them (capped), or from the cell counts
inline uint32_t go_level1(const GoLevel0 &l0, const std::vector<uint64_t> &cells, bool exact, int bits0, double slack1,
                          uint64_t b2rows, int l1_threads, const GpRange &rg, const std::vector<int64_t> &hkeys,
                          GoLevel1 *l) {
  const int bits1 = 14 - bits0;
  const uint32_t nb1 = 1u << bits1;
  const std::vector<uint64_t> &p0 = l0.p0;
  const std::vector<uint32_t> &dig0 = l0.dig0;
  const uint32_t np0 = (uint32_t)(p0.size() / 2);
  std::vector<GpSeg> &s2 = l->s2;
  uint64_t ovf1 = 0;
  for (uint32_t i = 0; i < np0; ++i) {
    GpSeg sg{p0[2 * i], p0[2 * i + 1] - p0[2 * i], 0, 0};
    sg.obase = ovf1;
    if (exact) {
      sg.ocap = 0;
      for (uint32_t q = 0; q < nb1; ++q) ovf1 += (cells[(dig0[i] << bits1) | q] + 1) & ~1ull;
    } else {
      sg.ocap = ((uint64_t)ceil((double)sg.count / nb1 * slack1) + 64 + 1) & ~1ull;
      ovf1 += sg.ocap << bits1;
    }
    s2.push_back(sg);
  }
  l->ovf1 = ovf1;
  if (ovf1 + 2 * GP_TILE > b2rows) return NUT_GB_DECLINE_CAPACITY;
  l->acap1 = b2rows - ovf1 - 2 * GP_TILE;  // level 1's arena: rows [ovf1, ovf1 + acap1) of B2
  const uint64_t nparts = l->nparts = (uint64_t)np0 * nb1;
  if (nparts == 0) return NUT_GB_DECLINE_CAPACITY;  // (no kept row reached level 0: not reached)
  // chunks of level-0 partitions (in key order) shrinking — 3/8, 1/4, 3/16, 1/16, 1/16,
  // 1/16: a chunk's transfer (~0.4x its compute) hides behind the next, smaller chunk, and
  // only the last 1/16 crosses after the work; each launch costs a tail, so few chunks.
  // The first chunk at 3/8 instead of 1/2 starts the transfers earlier: same-box A/Bs on two
  // boxes, Zipf-like keys 17.88-17.90 vs 18.33-18.76 and 18.37-18.58 vs 19.12-19.22 ms,
  // uniform 18.21-18.24 vs 18.34-18.62 and 20.75-21.16 vs 20.90; three 1/16 chunks at the
  // end instead of 1/8 + 1/16, a third box: Zipf-like 18.42-18.56 vs 19.43-19.59, uniform
  // 20.18 vs 20.18-20.23 (profiles/r06/groupby1e7/ab_chunks.txt)
  std::vector<uint32_t> &cb = l->cb;
  cb.assign(1, 0);
  for (uint32_t f : {6u, 10u, 13u, 14u, 15u, 16u}) {
    const uint32_t e1 = (uint32_t)((uint64_t)np0 * f / 16);
    if (e1 > cb.back()) cb.push_back(e1);
  }
  const uint32_t nch = l->nch();
  l->tiles.clear();
  l->tile0.assign(nch + 1, 0);
  l->ntile.assign(nch, 0);
  for (uint32_t j = 0; j < nch; ++j) {
    std::vector<GpSeg> sub(s2.begin() + cb[j], s2.begin() + cb[j + 1]);
    std::vector<uint32_t> ts;
    l->ntile[j] = gp_tiles(sub, (uint32_t)l1_threads * GP_ITEMS, ts);
    for (uint32_t i = 0; i < sub.size(); ++i) s2[cb[j] + i].tile0 = sub[i].tile0;
    l->tile0[j] = (uint32_t)l->tiles.size();
    l->tiles.insert(l->tiles.end(), ts.begin(), ts.end());
  }
  std::vector<uint64_t> &init = l->init, &rend = l->rend;
  init.assign(nparts + nch, 0);  // + one overflow flag per chunk
  rend.assign(nparts, 0);
  for (uint32_t i = 0; i < np0; ++i) {
    uint64_t at = s2[i].obase;  // (exact: digit d's rows after digit d - 1's, even starts)
    for (uint32_t d = 0; d < nb1; ++d) {
      const uint64_t q = (uint64_t)i * nb1 + d;
      if (exact) {
        const uint64_t cnt = cells[(dig0[i] << bits1) | d];
        init[q] = at;
        rend[q] = at + cnt;
        at += (cnt + 1) & ~1ull;
      } else {
        init[q] = s2[i].obase + (uint64_t)d * s2[i].ocap;
        rend[q] = s2[i].obase + (uint64_t)(d + 1) * s2[i].ocap;
      }
    }
  }
  // each heavy key's partition (heavy pass): level-0 digit -> its index among the non-empty
  // level-0 partitions (region d starts at row d * ocap), then the level-1 digit; -1: its
  // level-0 partition holds no rows (the host folds that key's group)
  const uint32_t nh = (uint32_t)hkeys.size();
  l->hq.assign(nh, -1);
  if (nh) {
    std::vector<int64_t> idx0((size_t)1 << bits0, -1);
    for (uint32_t i = 0; i < np0; ++i) idx0[dig0[i]] = i;
    for (uint32_t j = 0; j < nh; ++j) {
      const uint32_t cell = rg.cell((uint64_t)hkeys[j]);
      const int64_t i0 = idx0[cell >> bits1];
      if (i0 >= 0) l->hq[j] = i0 * nb1 + (cell & (nb1 - 1));
    }
  }
  return 0;
}

}  // namespace nut
