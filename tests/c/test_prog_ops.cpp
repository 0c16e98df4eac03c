// The expression-op functions of nutdb_amd/csrc/prog_ops.hpp on the host, with a plain C++
// compiler (tests/test_prog_ops_cpu.py builds this, once more under UBSan, and compares).
// stdin: rows "function part a b"; stdout: per row the result word in decimal, and for
// div / mod the zero-divisor flag after it.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "prog_ops.hpp"

int main() {
  char fn[16];
  int part;
  int64_t a, b;
  long rows = 0;
  while (scanf("%15s %d %" SCNd64 " %" SCNd64, fn, &part, &a, &b) == 4) {
    bool err = false;
    int64_t r;
    if (!strcmp(fn, "div")) r = nut::jdiv(a, b, err);
    else if (!strcmp(fn, "mod")) r = nut::jmod(a, b, err);
    else if (!strcmp(fn, "shl")) r = nut::jshl(a, b);
    else if (!strcmp(fn, "shr")) r = nut::jshr(a, b);
    else if (!strcmp(fn, "abs")) r = nut::jabs(a);
    else if (!strcmp(fn, "datepart")) r = nut::jdatepart(a, part);
    else if (!strcmp(fn, "timepart")) r = nut::jtimepart(a, part);
    else if (!strcmp(fn, "datetrunc")) r = nut::jdatetrunc(a, part);
    else if (!strcmp(fn, "addmonths")) r = nut::jaddmonths(a, b);
    else {
      fprintf(stderr, "unknown function '%s'\n", fn);
      return 2;
    }
    if (!strcmp(fn, "div") || !strcmp(fn, "mod")) printf("%" PRId64 " %d\n", r, (int)err);
    else printf("%" PRId64 "\n", r);
    ++rows;
  }
  if (!feof(stdin)) {
    fprintf(stderr, "malformed row after %ld rows\n", rows);
    return 2;
  }
  return 0;
}
