// Stand-alone driver of nutdb_amd/csrc/go_plan.hpp for tests/test_go_plan_cpu.py (plain C++, no
// HIP).  stdin, one command at a time; every command prints one line "<name> <why> ..." (why:
// the decline reason, 0 = none) and then one line per list it made ("<list> v v v ...").
//   range <min> <max>                     -> range why lo span t mul
//   cell <k> then k keys                  -> cell 0 + the keys' cells (current range)
//   sample <p> then p pairs <key> <mult>  -> sample 0 total
//   admit <bits0>                         -> admit why
//   heavy <na>                            -> heavy 0 nh seed1 seed2; hk: key a slot[a] b slot[b] per key
//   hkeys <k> then k keys                 -> hkeys 0 k          (sets the heavy keys directly)
//   sizes <n> <bits0> <nstore> <lam> <heavy> <keep_capped>
//                                         -> sizes 0 exact slack1 rows arena1 b2rows ocap abase0 acap0 data_bytes
//   counts <p> then p pairs <cell> <rows> -> counts 0 total     (the other cells: 0 rows)
//   hcount <k> <hchunk> then k counts     -> hcount 0 k         (k = 0: no heavy pass)
//   l0 <exact> <n> <bits0> <rows> <ocap> [capped: <np> then np pairs <start> <end>]
//                                         -> l0 why; segs (5 words each), p0, dig0, cur0, ts0
//   l1 <exact> <bits0> <slack1> <b2rows> <l1_threads>
//                                         -> l1 why ovf1 acap1 nparts; cb, tile0, ntile, tiles, s2 (5 words each),
//                                            init, rend, hq
// Bulk commands for tests/test_gorder_shapes_cpu.py (whole columns, read from binary files of int64):
//   samplef <file>                        -> samplef 0 total min max   (the sample: the file's first 65536 keys)
//   hist <file> <count>                   -> hist 0 kept heavy nonzero; cells: cell rows per non-empty cell
//                                            (the keys that are not heavy keys, counted per range cell: sets `counts`)
//   slots <k> then k keys                 -> slots 0 k; sl: key a slot[a] b slot[b] per key (the heavy pass's lookups)
//   grid <n> <num_cus> <per_cu>           -> grid why ntiles hgrid chunk
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "go_plan.hpp"

using namespace nut;

template <class T>
static void line(const char *name, const std::vector<T> &v) {
  printf("%s", name);
  for (const T &x : v) printf(" %lld", (long long)x);
  printf("\n");
}
static void segs_line(const char *name, const std::vector<GpSeg> &v) {
  printf("%s", name);
  for (const GpSeg &s : v)
    printf(" %" PRIu64 " %" PRIu64 " %u %" PRIu64 " %" PRIu64, s.start, s.count, s.tile0, s.obase, s.ocap);
  printf("\n");
}
static bool u64(uint64_t *x) { return scanf("%" SCNu64, x) == 1; }
static bool i64(int64_t *x) { return scanf("%" SCNd64, x) == 1; }

int main() {
  GpRange rg{};
  GoSample tab;
  GoHeavy hv;
  std::vector<uint64_t> cells(GO_CELLS, 0), hcount;
  uint64_t hchunk = 0;
  GoLevel0 l0;
  char cmd[16];
  while (scanf("%15s", cmd) == 1) {
    if (!strcmp(cmd, "range")) {
      int64_t a, b;
      if (!i64(&a) || !i64(&b)) return 2;
      const uint32_t why = go_range(a, b, &rg);
      printf("range %u %" PRIu64 " %" PRIu64 " %d %u\n", why, rg.lo, rg.span, rg.t, rg.mul);
    } else if (!strcmp(cmd, "cell")) {
      uint64_t k;
      if (!u64(&k)) return 2;
      printf("cell 0");
      for (uint64_t i = 0; i < k; ++i) {
        int64_t key;
        if (!i64(&key)) return 2;
        printf(" %u", rg.cell((uint64_t)key));
      }
      printf("\n");
    } else if (!strcmp(cmd, "sample")) {
      uint64_t p;
      if (!u64(&p)) return 2;
      std::vector<int64_t> smp;
      for (uint64_t i = 0; i < p; ++i) {
        int64_t key;
        uint64_t mult;
        if (!i64(&key) || !u64(&mult)) return 2;
        smp.insert(smp.end(), mult, key);
      }
      if (smp.size() > kGoSample) return 4;
      go_sample_table(smp, &tab);
      printf("sample 0 %zu\n", smp.size());
    } else if (!strcmp(cmd, "admit")) {
      int bits0;
      if (scanf("%d", &bits0) != 1) return 2;
      printf("admit %u\n", go_admit(tab, rg, bits0));
    } else if (!strcmp(cmd, "heavy")) {
      int na;
      if (scanf("%d", &na) != 1) return 2;
      hv = GoHeavy{};
      go_heavy_keys(tab, na, &hv);
      printf("heavy 0 %zu %" PRIu64 " %" PRIu64 "\n", hv.keys.size(), hv.seed1, hv.seed2);
      for (int64_t k : hv.keys) {
        const uint32_t a = hk_slot((uint64_t)k, hv.seed1), b = hk_slot((uint64_t)k, hv.seed2);
        printf("hk %" PRId64 " %u %u %u %u\n", k, a, (unsigned)hv.slot[a], b, (unsigned)hv.slot[b]);
      }
    } else if (!strcmp(cmd, "hkeys")) {
      uint64_t k;
      if (!u64(&k)) return 2;
      hv = GoHeavy{};
      hv.keys.resize(k);
      for (auto &x : hv.keys)
        if (!i64(&x)) return 2;
      printf("hkeys 0 %zu\n", hv.keys.size());
    } else if (!strcmp(cmd, "sizes")) {
      uint64_t n;
      int bits0, nstore, heavy, keep;
      double lam;
      if (!u64(&n) || scanf("%d %d %lf %d %d", &bits0, &nstore, &lam, &heavy, &keep) != 5) return 2;
      const GoSizes z = go_sizes(n, bits0, nstore, lam, heavy != 0, keep != 0);
      printf("sizes 0 %d %.17g %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %zu\n", (int)z.exact,
             z.slack1, z.rows, z.arena1, z.b2rows, z.ocap, z.abase0, z.acap0, z.data_bytes);
    } else if (!strcmp(cmd, "counts")) {
      uint64_t p, total = 0;
      if (!u64(&p)) return 2;
      cells.assign(GO_CELLS, 0);
      for (uint64_t i = 0; i < p; ++i) {
        uint64_t q, r;
        if (!u64(&q) || !u64(&r) || q >= GO_CELLS) return 2;
        cells[q] = r;
        total += r;
      }
      printf("counts 0 %" PRIu64 "\n", total);
    } else if (!strcmp(cmd, "hcount")) {
      uint64_t k;
      if (!u64(&k) || !u64(&hchunk)) return 2;
      hcount.resize(k);
      for (auto &x : hcount)
        if (!u64(&x)) return 2;
      printf("hcount 0 %zu\n", hcount.size());
    } else if (!strcmp(cmd, "l0")) {
      int exact, bits0;
      uint64_t n, rows, ocap;
      if (scanf("%d", &exact) != 1 || !u64(&n) || scanf("%d", &bits0) != 1 || !u64(&rows) || !u64(&ocap)) return 2;
      l0 = GoLevel0{};
      go_l0_segs(n, hcount, hchunk, ocap, &l0.segs);
      uint32_t why = 0;
      if (exact) {
        why = go_l0_exact(cells, bits0, rows, &l0);
      } else {
        uint64_t np;
        if (!u64(&np)) return 2;
        l0.p0.resize(2 * np);
        for (auto &x : l0.p0)
          if (!u64(&x)) return 2;
        go_l0_capped(ocap, &l0);
      }
      printf("l0 %u\n", why);
      segs_line("segs", l0.segs);
      line("p0", l0.p0);
      line("dig0", l0.dig0);
      line("cur0", l0.cur0);
      line("ts0", l0.ts0);
    } else if (!strcmp(cmd, "l1")) {
      int exact, bits0, l1_threads;
      double slack1;
      uint64_t b2rows;
      if (scanf("%d %d %lf", &exact, &bits0, &slack1) != 3 || !u64(&b2rows) || scanf("%d", &l1_threads) != 1) return 2;
      GoLevel1 l1;
      const uint32_t why = go_level1(l0, cells, exact != 0, bits0, slack1, b2rows, l1_threads, rg, hv.keys, &l1);
      printf("l1 %u %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", why, l1.ovf1, l1.acap1, l1.nparts);
      line("cb", l1.cb);
      line("tile0", l1.tile0);
      line("ntile", l1.ntile);
      line("tiles", l1.tiles);
      segs_line("s2", l1.s2);
      line("init", l1.init);
      line("rend", l1.rend);
      line("hq", l1.hq);
    } else if (!strcmp(cmd, "samplef")) {
      char path[1024];
      if (scanf("%1023s", path) != 1) return 2;
      FILE *f = fopen(path, "rb");
      if (!f) return 5;
      std::vector<int64_t> smp(kGoSample);
      smp.resize(fread(smp.data(), 8, kGoSample, f));
      fclose(f);
      if (smp.empty()) return 5;
      go_sample_table(smp, &tab);
      const auto mm = std::minmax_element(smp.begin(), smp.end());
      printf("samplef 0 %zu %" PRId64 " %" PRId64 "\n", smp.size(), *mm.first, *mm.second);
    } else if (!strcmp(cmd, "hist")) {
      char path[1024];
      uint64_t count;
      if (scanf("%1023s", path) != 1 || !u64(&count)) return 2;
      FILE *f = fopen(path, "rb");
      if (!f) return 5;
      cells.assign(GO_CELLS, 0);
      uint64_t kept = 0, heavy = 0, nonzero = 0;
      std::vector<int64_t> buf(1 << 16);
      while (count) {
        const size_t got = fread(buf.data(), 8, (size_t)std::min<uint64_t>(count, buf.size()), f);
        if (!got) break;
        count -= got;
        for (size_t i = 0; i < got; ++i) {
          if (std::binary_search(hv.keys.begin(), hv.keys.end(), buf[i])) {
            ++heavy;
          } else {
            ++kept;
            ++cells[rg.cell((uint64_t)buf[i])];
          }
        }
      }
      fclose(f);
      if (count) return 5;
      for (uint64_t x : cells) nonzero += x != 0;
      printf("hist 0 %" PRIu64 " %" PRIu64 " %" PRIu64 "\ncells", kept, heavy, nonzero);
      for (uint32_t q = 0; q < GO_CELLS; ++q)
        if (cells[q]) printf(" %u %" PRIu64, q, cells[q]);
      printf("\n");
    } else if (!strcmp(cmd, "slots")) {
      uint64_t k;
      if (!u64(&k) || hv.slot.size() != HK_SLOTS) return 2;
      printf("slots 0 %" PRIu64 "\n", k);
      for (uint64_t i = 0; i < k; ++i) {
        int64_t key;
        if (!i64(&key)) return 2;
        const uint32_t a = hk_slot((uint64_t)key, hv.seed1), b = hk_slot((uint64_t)key, hv.seed2);
        printf("sl %" PRId64 " %u %u %u %u\n", key, a, (unsigned)hv.slot[a], b, (unsigned)hv.slot[b]);
      }
    } else if (!strcmp(cmd, "grid")) {
      uint64_t n;
      int cus, per_cu;
      if (!u64(&n) || scanf("%d %d", &cus, &per_cu) != 2) return 2;
      GoHeavyGrid hg;
      const uint32_t why = go_heavy_grid(n, cus, per_cu, &hg);
      printf("grid %u %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", why, hg.ntiles, hg.hgrid, hg.chunk);
    } else {
      return 3;
    }
  }
  return 0;
}
