// The exactly defined math functions of nutdb_amd/csrc/prog_ops.hpp (rounding, sign, least /
// greatest, casts, sqrt) on the host, with a plain C++ compiler (tests/test_math_ops_cpu.py
// builds this, once more under UBSan with the float-cast check, and compares bit for bit).
// stdin: rows "function p q a b", p and q the function's literals, a and b the operand words
// in hex (an f64: its bits); stdout: per row the result word in hex.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "prog_ops.hpp"

int main() {
  char fn[16];
  int p, q;
  uint64_t a, b;
  long rows = 0;
  while (scanf("%15s %d %d %" SCNx64 " %" SCNx64, fn, &p, &q, &a, &b) == 5) {
    const double x = nut::jdbl(a), y = nut::jdbl(b);
    const int64_t i = (int64_t)a, j = (int64_t)b;
    uint64_t r;
    if (!strcmp(fn, "roundf")) r = nut::jbits(nut::jroundf(x, p, q));
    else if (!strcmp(fn, "roundi")) r = (uint64_t)nut::jroundi(i, p, q);
    else if (!strcmp(fn, "sqrt")) r = nut::jbits(nut::jsqrt(x));
    else if (!strcmp(fn, "signf")) r = (uint64_t)nut::jsignf(x);
    else if (!strcmp(fn, "signi")) r = (uint64_t)nut::jsigni(i);
    else if (!strcmp(fn, "leastf")) r = nut::jbits(nut::jleastf(x, y));
    else if (!strcmp(fn, "greatestf")) r = nut::jbits(nut::jgreatestf(x, y));
    else if (!strcmp(fn, "leasti")) r = (uint64_t)nut::jleasti(i, j);
    else if (!strcmp(fn, "greatesti")) r = (uint64_t)nut::jgreatesti(i, j);
    else if (!strcmp(fn, "castf")) r = p == NUT_CAST_F32 ? nut::jbits(nut::jtof32(x)) : (uint64_t)nut::jnarrow(nut::jtoi64(x), p);
    else if (!strcmp(fn, "casti")) r = p == NUT_CAST_F32 ? nut::jbits(nut::jtof32i(i)) : (uint64_t)nut::jnarrow(i, p);
    else {
      fprintf(stderr, "unknown function '%s'\n", fn);
      return 2;
    }
    printf("%" PRIx64 "\n", r);
    ++rows;
  }
  if (!feof(stdin)) {
    fprintf(stderr, "malformed row after %ld rows\n", rows);
    return 2;
  }
  return 0;
}
