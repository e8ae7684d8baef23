// bg_sortplan.h — how a sort of one columnar input (chrom, start, end[, score]; DESIGN.md
// §3.4) into the order bg_load_columns wants is laid out, decided on the host from three
// numbers a key pass over the columns would reduce: the number of names, the largest start and
// the largest end - start. Host-only and free of HIP, so tools/sort_plan_check.cpp checks it on
// the CPU (tests/test_sort_plan.py). bg_sort_columns (bg_sortcols.hip) reduces the three numbers
// in its key pass and runs exactly the digit passes planned here.
//
// (rank, start, end) orders rows exactly as (rank, start, end - start) does, and the length is
// the narrower number. With br = bits(nnames - 1), bs = bits(max start), bl = bits(max len):
//   br + bs + bl <= 64   one packed key  rank << (bs + bl) | start << bl | len  with the row
//                        index as payload, sorted in ceil((br + bs + bl) / 8) digit passes;
//   otherwise            two stable rounds: by len (bl bits), then by rank << bs | start
//                        (br + bs bits; at most 22 + 40).
#pragma once
#include <stdint.h>

struct bg_sort_plan {
  int br, bs, bl;  // bits of the largest rank, start and length
  bool packed;     // one packed key (round 0 only)
  int bits[2];     // key width of each round (two rounds: 0 = by length, 1 = by rank and start)
  int passes[2];   // 8-bit digit passes of each round
};

static inline int bg_bits_u64(uint64_t v) {
  int b = 0;
  while (b < 64 && (v >> b) != 0) ++b;
  return b;
}

// n rows over nnames names; fewer than two rows need no pass at all
static inline bg_sort_plan bg_sort_columns_plan(uint64_t n, uint32_t nnames, uint64_t max_start, uint64_t max_len) {
  bg_sort_plan p;
  p.br = bg_bits_u64(nnames ? (uint64_t)nnames - 1 : 0);
  p.bs = bg_bits_u64(max_start);
  p.bl = bg_bits_u64(max_len);
  p.packed = p.br + p.bs + p.bl <= 64;
  p.bits[0] = p.packed ? p.br + p.bs + p.bl : p.bl;
  p.bits[1] = p.packed ? 0 : p.br + p.bs;
  if (n < 2) p.bits[0] = p.bits[1] = 0;
  for (int r = 0; r < 2; ++r) p.passes[r] = (p.bits[r] + 7) / 8;
  return p;
}
