// Stand-alone driver of nutdb_amd/csrc/pick.hpp for tests/test_pick_cpu.py (plain C++, no HIP).
// stdin, one command a line:
//   g <nkeys> <ng>        then ng lines "<word0> <word1>": the sorted group tuples
//   q <k0> <k1>           -> "<lower bound> <group index or -1>"
//   i <hex bits>          -> the int64 order word, hex
//   f <hex bits>          -> the f64 order word, hex
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "pick.hpp"

int main() {
  std::vector<int64_t> g0, g1;
  int nkeys = 0;
  char cmd[8];
  while (scanf("%7s", cmd) == 1) {
    if (!strcmp(cmd, "g")) {
      unsigned long long ng;
      if (scanf("%d %llu", &nkeys, &ng) != 2) return 2;
      g0.assign(ng, 0);
      g1.assign(ng, 0);
      for (unsigned long long i = 0; i < ng; ++i)
        if (scanf("%" SCNd64 " %" SCNd64, &g0[i], &g1[i]) != 2) return 2;
    } else if (!strcmp(cmd, "q")) {
      int64_t k0, k1;
      if (scanf("%" SCNd64 " %" SCNd64, &k0, &k1) != 2) return 2;
      const uint64_t lb = nut::pick_lower_bound(g0.data(), g1.data(), nkeys, g0.size(), k0, k1);
      const uint32_t f = nut::pick_find_group(g0.data(), g1.data(), nkeys, g0.size(), k0, k1);
      printf("%" PRIu64 " %lld\n", lb, f == nut::PK_NONE ? -1ll : (long long)f);
    } else if (!strcmp(cmd, "i") || !strcmp(cmd, "f")) {
      uint64_t b;
      if (scanf("%" SCNx64, &b) != 1) return 2;
      printf("%016" PRIx64 "\n", cmd[0] == 'i' ? nut::pick_ord_i64(b) : nut::pick_ord_f64(b));
    } else {
      return 3;
    }
  }
  return 0;
}
