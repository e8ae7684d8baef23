// bg_mapstat.hip — every numeric bedmap operation as a column of doubles (include/bedgpu.h,
// bg_result_export_map_values): per reference row the double render() of bg_format.hip prints
// for the operation, NaN where it prints NAN.
//
//   k_map_stat    the operations whose per-row aggregates the result already holds (count, sums,
//                 sums of squares, extremes, bases, uniq): one thread per row does render()'s
//                 arithmetic, the same double expressions in the same order.
//   k_seg_select  --median / --kth / --mad, which have no stored value. The pair fill
//                 (bg_pairs_scores) first writes every member's score at its pair's slot, so row
//                 r's scores are the contiguous doubles V[off[r] .. off[r + 1]); the order
//                 statistics are then a segmented selection, with no membership test in it. A
//                 wave owns 64 consecutive rows:
//                   rows of <= small members: each lane resolves its own row by counting (x is at
//                     sorted positions [#{< x}, #{<= x}), window_rank's rule);
//                   longer rows: one at a time by the whole wave, a radix select on
//                     order-preserving 64-bit keys, 8 passes of 8 bits with a 256-bin histogram
//                     of the wave's own in LDS; lanes stride the segment, so the loads coalesce.
//                     The rank after (kth's and MAD's second element) comes from the last
//                     histogram where the found value's count covers it, else from one more pass
//                     for the least key above. MAD selects among |x - med| computed on the fly.
//                 No segment is copied or sorted.
// -0.0 and +0.0 are one value of the reference's multiset; both tiers read a zero as +0.0.
#include <cstdlib>

#include "bg_internal.h"

// rows of at most this many members are selected by counting, one lane each. Measured (DESIGN.md
// §3.5): counting wins 6 to 1 on rows of ~8 members, the radix select on rows of ~26 and more
#define SEL_SMALL 16

struct StatArgs {
  int op;
  const int32_t* cnt;
  const int64_t* RS;
  const int64_t* RE;
  const int64_t* isum;
  const int64_t* isq;
  const double* dsum;
  const double* dsq;
  const double* vmin;
  const double* vmax;
  const uint64_t* bases;
  const uint32_t* uniq;
  uint64_t n;
  double* out;
};

// NAN of the text: a NaN with the sign bit clear. A value that is itself a NaN (the text's
// "-nan", put_real of bg_format.hip: the square root of a variance rounded below zero, 0 / 0
// for a reference row of no length): a NaN with the sign bit set, so the two can be told apart
__device__ __forceinline__ double stat_out(double v, bool na) {
  if (na) return __longlong_as_double(0x7ff8000000000000LL);
  return v != v ? __longlong_as_double((long long)0xfff8000000000000ULL) : v;
}

__global__ void __launch_bounds__(BG_NT) k_map_stat(StatArgs A) {
  const uint64_t k = (uint64_t)blockIdx.x * BG_NT + threadIdx.x;
  if (k >= A.n) return;
  const int op = A.op;
  const int32_t c = A.cnt[k];
  bool na = false;  // the text has NAN: no value
  double v = 0.0;
  if (op == BG_MAP_COUNT) v = (double)c;
  else if (op == BG_MAP_INDICATOR) v = c > 0 ? 1.0 : 0.0;
  else if (op == BG_MAP_BASES) v = (double)A.bases[k];
  else if (op == BG_MAP_BASES_UNIQ) v = (double)A.uniq[k];
  else if (op == BG_MAP_ECHO_SIZE) v = (double)(uint64_t)(A.RE[k] - A.RS[k]);
  else if (op == BG_MAP_BASES_UNIQ_F) v = (double)A.uniq[k] / (double)(A.RE[k] - A.RS[k]);
  else if (c <= 0) na = true;
  else if (op == BG_MAP_MEAN) v = (A.dsum ? A.dsum[k] : (double)A.isum[k]) / (double)c;
  else if (op == BG_MAP_SUM) v = A.dsum ? A.dsum[k] : (double)A.isum[k];
  else if (op == BG_MAP_VARIANCE || op == BG_MAP_STDEV || op == BG_MAP_CV) {
    if (c <= 1) {
      na = true;
    } else {
      const double cnt = (double)c;
      const double sum = A.dsum ? A.dsum[k] : (double)A.isum[k];
      const double sq = A.dsq ? A.dsq[k] : (double)A.isq[k];
      const double numer = (cnt * sq) - (sum * sum);
      const double denom = (cnt * (cnt - 1));
      v = numer / denom;
      if (op != BG_MAP_VARIANCE) v = sqrt(v);
      if (op == BG_MAP_CV) {
        const double mean = sum / cnt;
        if (mean == 0) na = true;
        else v = v / mean;
      }
    }
  } else {
    v = (op == BG_MAP_MIN) ? A.vmin[k] : A.vmax[k];
  }
  A.out[k] = stat_out(v, na);
}

struct SelArgs {
  int op;
  double arg;         // --kth's value / --mad's multiplier
  const double* V;    // every pair's score (bg_pairs_scores)
  const uint64_t* off;
  uint64_t n;
  uint32_t small;     // SEL_SMALL, or BEDGPU_SEL_SMALL
  double* out;
};

// the selected value: the score, or its absolute deviation from med (mad_dev, bg_format.hip)
__device__ __forceinline__ double sel_x(double x, bool dev, double med) {
  if (dev) {
    const double d = x - med;
    x = d < 0 ? -d : d;
  }
  return x == 0 ? 0.0 : x;
}
// monotone for the finite doubles (and the infinities), zeros already made +0.0
__device__ __forceinline__ uint64_t sel_key(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | (1ULL << 63));
}
__device__ __forceinline__ double sel_unkey(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ULL << 63)) : ~k));
}
__device__ __forceinline__ void wave_lds_order() {  // (the wave's LDS operations complete in order)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one lane, by counting: the value at sorted position p of the c values at V (0.0 for p >= c,
// as window_rank)
__device__ __forceinline__ double lane_rank(const double* __restrict__ V, uint32_t c, uint32_t p, bool dev,
                                            double med) {
  for (uint32_t i = 0; i < c; ++i) {
    const double x = sel_x(V[i], dev, med);
    uint32_t lt = 0, le = 0;
#pragma unroll 4  // (independent loads in flight: the counters are the only carried values)
    for (uint32_t j = 0; j < c; ++j) {
      const double y = sel_x(V[j], dev, med);
      lt += y < x;
      le += y <= x;
    }
    if (lt <= p && p < le) return x;
  }
  return 0.0;
}
// the elements at p and, with two, at p + 1 as well
__device__ __forceinline__ void lane_rank2(const double* __restrict__ V, uint32_t c, uint32_t p, bool two, bool dev,
                                           double med, double& one, double& nxt) {
  one = lane_rank(V, c, p, dev, med);
  nxt = two ? lane_rank(V, c, p + 1, dev, med) : 0.0;
}

// the whole wave (every lane with the same arguments; h: the wave's 256 bins): the same
__device__ __forceinline__ void wave_rank2(const double* __restrict__ V, uint32_t c, uint32_t p, bool two, bool dev,
                                           double med, uint32_t* h, double& one, double& nxt) {
  one = nxt = 0.0;
  if (p >= c) return;
  const int lane = bg_lane();
  uint64_t prefix = 0;  // the key's digits found so far
  uint32_t rem = p;     // the position among the values that share them
  uint32_t eq = 0;      // after the last pass: how many values have the key
  for (int shift = 56; shift >= 0; shift -= 8) {
#pragma unroll
    for (int k = 0; k < 4; ++k) h[lane + 64 * k] = 0;
    wave_lds_order();
    const uint64_t himask = shift == 56 ? 0 : ~0ULL << (shift + 8);
    for (uint32_t base = 0; base < c; base += 64) {
      const uint32_t i = base + lane;
      bool in = i < c;
      uint64_t key = 0;
      if (in) {
        key = sel_key(sel_x(V[i], dev, med));
        in = (key & himask) == prefix;
      }
      const uint32_t d = (uint32_t)(key >> shift) & 255u;
      const uint64_t act = __ballot(in);
      if (act) {
        // one digit in all of them (the high bytes of scores of one magnitude): one add, not 64
        // adds to one address in turn
        const int first = __ffsll((unsigned long long)act) - 1;
        const uint32_t d0 = __shfl(d, first, 64);
        if (__ballot(in && d != d0) == 0) {
          if (lane == first) atomicAdd(&h[d0], (uint32_t)__popcll(act));
        } else if (in) {
          atomicAdd(&h[d], 1u);
        }
      }
    }
    wave_lds_order();
    // the bin that holds position rem: lane l scans bins 4l .. 4l + 3
    uint32_t b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = h[4 * lane + k];
    const uint32_t sum = b[0] + b[1] + b[2] + b[3];
    const uint32_t incl = wave_incl_scan(sum, OpSum());
    uint32_t below = incl - sum;
    const bool hit = below <= rem && rem < incl;  // (one lane: the bins hold every candidate, rem < their number)
    uint32_t dig = 4 * lane, cntb = b[0];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (rem >= below + cntb) {
        below += cntb;
        cntb = b[k + 1];
        ++dig;
      }
    const uint64_t hm = __ballot(hit);
    const int src = hm ? __ffsll((unsigned long long)hm) - 1 : 0;
    dig = __shfl(dig, src, 64);
    below = __shfl(below, src, 64);
    eq = __shfl(cntb, src, 64);
    prefix |= (uint64_t)dig << shift;
    rem -= below;
    wave_lds_order();  // (the bins are cleared next)
  }
  one = sel_unkey(prefix);
  if (!two || p + 1 >= c) return;
  if (rem + 1 < eq) {
    nxt = one;
    return;
  }
  uint64_t best = ~0ULL;  // the least key above
  for (uint32_t i = lane; i < c; i += 64) {
    const uint64_t key = sel_key(sel_x(V[i], dev, med));
    if (key > prefix && key < best) best = key;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)best, d, 64);
    best = o < best ? o : best;
  }
  nxt = sel_unkey(best);
}

// RollingKthAverage::DoneReference and MedianAbsoluteDeviation::DoneReference as window_kth and
// render() of bg_format.hip apply them, over a rank function R(p, two, dev, med, one, nxt)
template <typename R>
__device__ __forceinline__ double sel_kth(uint32_t n, double kth, R rank) {
  double one, two;
  if (n == 1) {
    rank(0u, false, false, 0.0, one, two);
    return one;
  }
  uint64_t up = (uint64_t)ceil(kth * (double)n), down = (uint64_t)floor(kth * (double)n);
  if (up > 0) --up;
  if (down > 0) --down;
  rank((uint32_t)up, up == down, false, 0.0, one, two);
  if (up == down) return (one + two) / 2.0;
  return one;
}
template <typename R>
__device__ __forceinline__ double sel_value(int op, double arg, uint32_t c, R rank) {
  if (op != BG_MAP_MAD) return sel_kth(c, op == BG_MAP_MEDIAN ? 0.5 : arg, rank);
  if (c <= 1) return 0.0;  // (NAN: the caller's)
  const double med = sel_kth(c, 0.5, rank);
  double mad, two;
  if (c % 2 == 0) {
    rank(c / 2 - 1, true, true, med, mad, two);
    mad += two;
    mad /= 2.0;
  } else {
    rank(c / 2, false, true, med, mad, two);
  }
  return mad * (arg > 0 ? arg : 1.0);
}

// LDS: 1 KiB of bins per wave
__global__ void __launch_bounds__(BG_NT) k_seg_select(SelArgs A) {
  __shared__ uint32_t hist[BG_NT / 64][256];
  const int lane = bg_lane();
  uint32_t* h = hist[bg_wave()];
  const uint64_t r = (uint64_t)blockIdx.x * BG_NT + threadIdx.x;
  const bool live = r < A.n;
  const uint64_t o = live ? A.off[r] : 0;
  const uint64_t cw = live ? A.off[r + 1] - o : 0;  // (a row's count is an int32: bg_result::cnt)
  const uint32_t c = (uint32_t)cw;
  double v = 0.0;
  const bool big = c > A.small;
  if (c > 0 && !big) {
    const double* V = A.V + o;
    v = sel_value(A.op, A.arg, c, [&](uint32_t p, bool two, bool dev, double med, double& one, double& nxt) {
      lane_rank2(V, c, p, two, dev, med, one, nxt);
    });
  }
  // the long rows, one at a time by all 64 lanes (the mask is the same in every lane)
  for (uint64_t todo = __ballot(big); todo; todo &= todo - 1) {
    const int l = __ffsll((unsigned long long)todo) - 1;
    // (through readfirstlane: the compiler then keeps the row's base and length in scalars)
    const uint32_t olo = __builtin_amdgcn_readfirstlane(__shfl((uint32_t)o, l, 64));
    const uint32_t ohi = __builtin_amdgcn_readfirstlane(__shfl((uint32_t)(o >> 32), l, 64));
    const double* V = A.V + ((uint64_t)ohi << 32 | olo);
    const uint32_t cl = __builtin_amdgcn_readfirstlane(__shfl(c, l, 64));
    const double x = sel_value(A.op, A.arg, cl, [&](uint32_t p, bool two, bool dev, double med, double& one, double& nxt) {
      wave_rank2(V, cl, p, two, dev, med, h, one, nxt);
    });
    if (lane == l) v = x;
  }
  if (live) A.out[r] = stat_out(v, c == 0 || (A.op == BG_MAP_MAD && c <= 1));
}

// BEDGPU_SEL_SMALL is a test hook (bedgpu.h): 0 sends every row with members to
// the wave's radix select, a huge value every row to the counting lanes; read at every call so a
// test can set it between calls
static uint32_t sel_small() {
  const char* s = getenv("BEDGPU_SEL_SMALL");
  if (!s || !*s) return SEL_SMALL;
  const long long v = atoll(s);
  return v < 0 ? 0u : (v > 0x7fffffffLL ? 0x7fffffffu : (uint32_t)v);
}

extern "C" int bg_result_export_map_values(bg_ctx* c, bg_result* r, int op_index, double* values) {
  if (!c || !r || !values) return BG_E_ARG;
  if (r->kind != RES_MAP) return bg_fail(c, BG_E_ARG, "values: not a bedmap result");
  if (op_index < 0 || op_index >= r->mopts.n_ops) return bg_fail(c, BG_E_ARG, "values: no such operation in the result");
  if (r->mopts.skip_unmapped)
    return bg_fail(c, BG_E_ARG, "values: the result was built with --skip-unmapped (filter by the count instead)");
  if ((uintptr_t)values & 15) return bg_fail(c, BG_E_ARG, "values: device columns must be 16-byte aligned");
  const int op = r->mopts.ops[op_index];
  bool select = false;
  switch (op) {
    case BG_MAP_COUNT: case BG_MAP_INDICATOR: case BG_MAP_SUM: case BG_MAP_MEAN: case BG_MAP_MIN: case BG_MAP_MAX:
    case BG_MAP_BASES: case BG_MAP_BASES_UNIQ: case BG_MAP_BASES_UNIQ_F: case BG_MAP_ECHO_SIZE:
    case BG_MAP_VARIANCE: case BG_MAP_STDEV: case BG_MAP_CV: break;
    case BG_MAP_MEDIAN: case BG_MAP_KTH: case BG_MAP_MAD: select = true; break;
    case BG_MAP_TMEAN: case BG_MAP_WMEAN:
      return bg_fail(c, BG_E_UNSUPPORTED, "values: --tmean and --wmean sum in the order of the reference's heap addresses, "
                                          "which only the text route replays");
    case BG_MAP_ECHO_NAME: case BG_MAP_ECHO_REF_ROW_ID:
      return bg_fail(c, BG_E_UNSUPPORTED, "values: --echo-ref-name and --echo-ref-row-id print text, not a number");
    default:
      return bg_fail(c, BG_E_UNSUPPORTED, "values: the element and echo operations print text, not a number");
  }
  if (!r->n) return 0;
  const dim3 g(bg_blocks(r->n, BG_NT)), b(BG_NT);
  if (!select) {
    const bg_table* R = r->set->t[r->tab];
    StatArgs A;
    A.op = op;
    A.cnt = r->cnt;
    A.RS = R->ks, A.RE = R->ke;
    A.isum = r->isum, A.isq = r->isq, A.dsum = r->dsum, A.dsq = r->dsq;
    A.vmin = r->vmin, A.vmax = r->vmax;
    A.bases = r->bases, A.uniq = r->uniq;
    A.n = r->n, A.out = values;
    BG_LAUNCH(c, "k_map_stat", k_map_stat, g, b, A);
    BG_HIP(c, hipGetLastError());
    return 0;
  }
  // the count, kept by the result when the caller ran it (bg_result_map_pairs); run here it is a
  // temporary of this call, so that the call leaves bg_live as it found it
  struct OwnOff {
    bg_ctx* c;
    bg_result* r;
    bool mine;
    ~OwnOff() {
      if (mine && r->poff) {
        bg_release(c, r->poff);
        r->poff = nullptr;
        r->ptotal = 0;
      }
    }
  } own{c, r, r->poff == nullptr};
  uint64_t total = 0;
  int rc = bg_result_map_pairs(c, r, &total);
  if (rc) return rc;
  BgHold hold(c);
  double* V = total ? hold.alloc<double>(total) : nullptr;
  if (!hold.ok()) return BG_E_NOMEM;
  if (total && (rc = bg_pairs_scores(c, r, V))) return rc;
  SelArgs S;
  S.op = op, S.arg = r->mopts.op_arg[op_index];
  S.V = V, S.off = r->poff, S.n = r->n;
  S.small = sel_small();
  S.out = values;
  BG_LAUNCH(c, "k_seg_select", k_seg_select, g, b, S);
  BG_HIP(c, hipGetLastError());
  // one round trip: the fill's status (no member anywhere: no fill, and nothing to wait for)
  if (total && (rc = bg_pairs_status(c))) return rc;
  bg_mark(c, "values");
  return 0;
}
