// sort_plan_check — prints the sort plan for one columnar input (bedops_amd/csrc/bg_sortplan.h)
// for given widths, on the CPU: tests/test_sort_plan.py reads the line.
//
//   sort_plan_check <rows> <names> <max start> <max length>
//   -> packed=<0|1> br=<b> bs=<b> bl=<b> bits=<r0>,<r1> passes=<r0>,<r1>
#include <stdio.h>
#include <stdlib.h>

#include "../bedops_amd/csrc/bg_sortplan.h"

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: %s <rows> <names> <max start> <max length>\n", argv[0]);
    return 2;
  }
  const uint64_t n = strtoull(argv[1], nullptr, 0), names = strtoull(argv[2], nullptr, 0);
  const uint64_t ms = strtoull(argv[3], nullptr, 0), ml = strtoull(argv[4], nullptr, 0);
  const bg_sort_plan p = bg_sort_columns_plan(n, (uint32_t)names, ms, ml);
  printf("packed=%d br=%d bs=%d bl=%d bits=%d,%d passes=%d,%d\n", p.packed ? 1 : 0, p.br, p.bs, p.bl, p.bits[0],
         p.bits[1], p.passes[0], p.passes[1]);
  return 0;
}
