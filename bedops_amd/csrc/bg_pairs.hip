// bg_pairs.hip — the overlap join behind a bedmap result as index columns (include/bedgpu.h,
// bg_result_map_pairs / bg_result_export_map_pairs): for every reference row r the rows of the
// map table in S(r) (bg_map.hip), ascending, at [offsets[r], offsets[r + 1]).
//
// Count: bg_result::cnt (k_map_ops) widened to 64 bits and scanned (bg_scan.hip) into the
// result's own offsets. Fill: a second walk over the candidates k_map_ops walked, with the same
// membership test (bg_map_live && bg_map_in), writing indices instead of aggregates:
//   k_pairs_flat  no long-row classes (LongRows::ncls == 0): every row's candidates are one range
//                 of the map table. A workgroup flattens the ranges of its BG_NT consecutive rows
//                 into one list and compacts it in rounds of BG_NT slots, so that a wave's stores
//                 are contiguous (thread-per-row stores at offsets[r] + j scatter every one).
//   k_pairs_rows  long rows by class: one thread per reference row merges the class ranges in
//                 index order, as bg_map_cands does for the formatter's --echo-map walk.
// Either writes, besides or instead of the indices, the member's score at the pair's slot
// (bg_pairs_scores: the segments bg_mapstat.hip selects the order statistics from).
// Both check on the device that they wrote what the offsets give them (ERR_PAIRS): the count
// pass and the fill pass must agree, and a row that disagrees cannot write outside its slots.
#include <climits>

#include "bg_internal.h"

struct PairArgs {
  const int64_t* RS;
  const int64_t* RE;
  uint64_t nr;
  const int64_t* MS;
  const int64_t* ME;
  uint64_t nm;
  int crit;        // the criterion as k_map_ops resolved it (BG_OVR_FAST for --faster)
  int64_t ovr;
  int64_t range;
  double perc;
  int64_t L;       // bg_result::win_L / win_touch
  int64_t touch;
  const uint64_t* wlo;  // the ranges k_map_ops kept (NEED_WIN, --faster); null: derived here
  const uint64_t* whi;
  const int64_t* zin;
  const int64_t* zout;
  LongRows lrows;
  const uint64_t* off;  // bg_result::poff
  int64_t* ref_rows;    // null: skipped
  int64_t* map_rows;
  const double* SC;     // the map table's scores and, at every pair's slot, the member's score
  double* vals;         //   (bg_pairs_scores, for bg_mapstat.hip); null: skipped
  bg_dstatus* st;
};

// the key range that bounds row [s, e)'s candidate starts: k_map_ops' klo / khi
__device__ __forceinline__ void pairs_keys(const PairArgs& A, int64_t s, int64_t e, int64_t& klo, int64_t& khi) {
  const int64_t g = s & ~BG_COORD_MASK;
  const int64_t pad = A.crit == BG_OVR_RANGE ? A.range : 0;
  klo = max(g, s - pad - A.L + 1 - A.touch);
  khi = min(g + (1LL << BG_KEY_SHIFT), e + pad + (A.crit == BG_OVR_EXACT ? 1 : A.touch));
}
__device__ __forceinline__ bool pairs_member(const PairArgs& A, uint64_t r, int64_t s, int64_t e, uint64_t m) {
  return bg_map_live(A.zin, A.zout, r, m) && bg_map_in(A.crit, A.ovr, A.range, A.perc, s, e, A.MS[m], A.ME[m]);
}

// LDS: 2 KiB of scan + 2 KiB of range starts + 4 KiB of reference rows (+ the small words)
__global__ void __launch_bounds__(BG_NT) k_pairs_flat(PairArgs A) {
  __shared__ uint64_t start[BG_NT + 1];  // exclusive scan of the rows' range lengths
  __shared__ uint64_t rlo[BG_NT];
  __shared__ int64_t rs[BG_NT], re[BG_NT];
  __shared__ uint64_t sh[BG_NT / 64 + 1];
  __shared__ int64_t wmax[BG_NT / 64];
  __shared__ uint64_t bnd[2];
  __shared__ uint32_t wc[2][BG_NT / 64];  // members per wave, by round parity
  const int lane = bg_lane(), w = bg_wave();
  const uint64_t r0 = (uint64_t)blockIdx.x * BG_NT;
  const uint64_t r = r0 + threadIdx.x;
  const bool live = r < A.nr;
  const int64_t s = live ? A.RS[r] : 0, e = live ? A.RE[r] : 0;
  uint64_t lo = 0, hi = 0;
  if (A.wlo) {
    if (live) {
      lo = A.wlo[r];
      hi = A.whi[r];
    }
  } else {  // as k_map_ops: the workgroup's range by two searches of the table, each row's inside it
    int64_t klo, khi;
    pairs_keys(A, s, e, klo, khi);
    int64_t hm = live ? khi : LLONG_MIN;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) hm = max(hm, (int64_t)__shfl_xor(hm, d, 64));
    if (lane == 0) wmax[w] = hm;
    __syncthreads();
    if (threadIdx.x == 0) bnd[0] = lower_bound_i64(A.MS, A.nm, klo);  // row r0 is live
    if (threadIdx.x == 64) {
      int64_t m = wmax[0];
      for (int k = 1; k < BG_NT / 64; ++k) m = max(m, wmax[k]);
      bnd[1] = lower_bound_i64(A.MS, A.nm, m);
    }
    __syncthreads();
    const uint64_t blo = bnd[0], bhi = max(bnd[0], bnd[1]);
    if (live) {
      lo = lower_bound_in(A.MS, blo, bhi, klo);
      hi = lower_bound_in(A.MS, lo, bhi, khi);
    }
  }
  uint64_t T;
  const uint64_t pre = block_excl_scan(hi > lo ? hi - lo : (uint64_t)0, OpSum(), (uint64_t)0, sh, &T);
  start[threadIdx.x] = pre;
  if (threadIdx.x == 0) start[BG_NT] = T;
  rlo[threadIdx.x] = lo;
  rs[threadIdx.x] = s;
  re[threadIdx.x] = e;
  __syncthreads();
  // the workgroup's slots [obase, obase + room): its rows are consecutive and members ascend in
  // a row, so its output is the compaction of the flat candidate list, in list order
  const uint64_t obase = A.off[r0];
  const uint64_t room = A.off[min(r0 + BG_NT, A.nr)] - obase;
  uint64_t run = 0;  // members of the rounds before
  uint32_t round = 0;
  // (the list has no bound: one reference row can hold the whole map table)
  for (uint64_t base = 0; base < T; base += BG_NT, ++round) {
    const uint64_t slot = base + threadIdx.x;
    bool mem = false;
    uint64_t m = 0;
    uint32_t j = 0;
    if (slot < T) {
      uint32_t b = BG_NT - 1;  // the row whose range holds the slot: first j with start[j + 1] > slot
      while (j < b) {
        const uint32_t mid = (j + b) >> 1;
        if (start[mid + 1] <= slot) j = mid + 1;
        else b = mid;
      }
      m = rlo[j] + (slot - start[j]);
      mem = pairs_member(A, r0 + j, rs[j], re[j], m);
    }
    const uint64_t mask = __ballot(mem);
    if (lane == 0) wc[round & 1][w] = (uint32_t)__popcll(mask);
    // one barrier per round: a parity's words are next written two rounds on, after the barrier
    // in between, which every read of them precedes
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < BG_NT / 64; ++k) {
      const uint32_t x = wc[round & 1][k];
      before += k < w ? x : 0;
      all += x;
    }
    if (mem) {
      const uint64_t k = run + before + (uint32_t)__popcll(mask & ((1ULL << lane) - 1));
      if (k < room) {  // (a fill that disagrees with the count stays inside the workgroup's slots)
        if (A.ref_rows) A.ref_rows[obase + k] = (int64_t)(r0 + j);
        if (A.map_rows) A.map_rows[obase + k] = (int64_t)m;
        if (A.vals) A.vals[obase + k] = A.SC[m];
      }
    }
    run += all;
  }
  if (threadIdx.x == 0 && run != room) bg_report(A.st, r0, ERR_PAIRS);
}

// bg_map_cands (bg_internal.h) with the class cursors in registers: its arrays are indexed by a
// run-time class count and live in scratch memory; here every loop over the classes has a
// compile-time bound NC >= ncls and is unrolled, so q / qe stay in VGPRs. Same candidates in
// the same (map-row) order.
template <int NC, typename F>
__device__ __forceinline__ void pairs_cands(const PairArgs& A, uint64_t lo, uint64_t hi, int64_t s, int64_t e, F f) {
  const LongRows& LR = A.lrows;
  const int64_t pad = A.crit == BG_OVR_RANGE ? A.range : 0;
  const int64_t g = s & ~BG_COORD_MASK;
  const int64_t khi = min(g + (1LL << BG_KEY_SHIFT), e + pad);
  uint64_t q[NC], qe[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    q[c] = qe[c] = 0;
    if (c < LR.ncls) {
      const int64_t klo = max(g, s - pad - (LR.thr << (c + 1)) + 1);
      q[c] = bg_lb_range(LR.ls, LR.coff[c], LR.coff[c + 1], klo);
      qe[c] = bg_lb_range(LR.ls, q[c], LR.coff[c + 1], khi);
    }
  }
  uint64_t m = lo;
  for (;;) {
    while (m < hi && A.ME[m] - A.MS[m] > LR.thr) ++m;  // long rows come from their class
    uint64_t best = m < hi ? m : ~0ULL;
    int bc = -1;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (q[c] < qe[c]) {
        const uint64_t x = LR.idx[q[c]];
        if (x < best) { best = x; bc = c; }
      }
    if (best == ~0ULL) break;
    f(best);
    if (bc < 0) ++m;
#pragma unroll
    for (int c = 0; c < NC; ++c) q[c] += bc == c ? 1 : 0;
  }
}

template <int NC>
__global__ void __launch_bounds__(BG_NT) k_pairs_rows(PairArgs A) {
  const uint64_t r = (uint64_t)blockIdx.x * BG_NT + threadIdx.x;
  if (r >= A.nr) return;
  const int64_t s = A.RS[r], e = A.RE[r];
  uint64_t lo, hi;
  if (A.wlo) {
    lo = A.wlo[r];
    hi = A.whi[r];
  } else {
    int64_t klo, khi;
    pairs_keys(A, s, e, klo, khi);
    lo = lower_bound_i64(A.MS, A.nm, klo);
    hi = lower_bound_in(A.MS, lo, A.nm, khi);
  }
  const uint64_t o = A.off[r], room = A.off[r + 1] - o;
  uint64_t j = 0;
  pairs_cands<NC>(A, lo, hi, s, e, [&](uint64_t m) {
    if (!pairs_member(A, r, s, e, m)) return;
    if (j < room) {  // (a fill that disagrees with the count stays inside the row's slots)
      if (A.ref_rows) A.ref_rows[o + j] = (int64_t)r;
      if (A.map_rows) A.map_rows[o + j] = (int64_t)m;
      if (A.vals) A.vals[o + j] = A.SC[m];
    }
    ++j;
  });
  if (j != room) bg_report(A.st, r, ERR_PAIRS);
}

// cnt widened for the scan (entry n: 0, so that the exclusive scan leaves the total there)
__global__ void __launch_bounds__(BG_NT) k_pairs_widen(const int32_t* __restrict__ cnt, uint64_t n,
                                                       uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * BG_NT + threadIdx.x;
  if (i <= n) out[i] = i < n ? (uint64_t)cnt[i] : 0;
}
// (kernels, not hipMemcpy, write the caller's buffers: see k_cols_key, bg_columns.hip)
__global__ void __launch_bounds__(BG_NT) k_pairs_offsets(const uint64_t* __restrict__ in, uint64_t n,
                                                         int64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * BG_NT + threadIdx.x;
  if (i < n) out[i] = (int64_t)in[i];
}

static int pairs_check(bg_ctx* c, const bg_result* r) {
  if (r->kind != RES_MAP) return bg_fail(c, BG_E_ARG, "pairs: not a bedmap result");
  if (r->mopts.skip_unmapped)
    return bg_fail(c, BG_E_ARG, "pairs: the result was built with --skip-unmapped (filter by the count instead)");
  return 0;
}

extern "C" int bg_result_map_pairs(bg_ctx* c, bg_result* r, uint64_t* total) {
  if (!c || !r || !total) return BG_E_ARG;
  int rc = pairs_check(c, r);
  if (rc) return rc;
  if (r->poff) {
    *total = r->ptotal;
    return 0;
  }
  const uint64_t n1 = r->n + 1;
  BgHold hold(c);
  uint64_t* off = hold.alloc<uint64_t>(n1);
  if (!hold.ok()) return BG_E_NOMEM;
  BG_LAUNCH(c, "k_pairs_widen", k_pairs_widen, dim3(bg_blocks(n1, BG_NT)), dim3(BG_NT), (const int32_t*)r->cnt, r->n,
            off);
  BG_HIP(c, hipGetLastError());
  if ((rc = bg_scan_sum_u64(c, off, off, n1, nullptr))) return rc;
  uint64_t tot = 0;
  if ((rc = bg_fetch_u64(c, off + r->n, &tot))) return rc;
  r->poff = hold.give(off);
  r->ptotal = *total = tot;
  return 0;
}

// the fill: one launch on ctx's stream that writes, at every pair's slot, whichever of the
// columns is asked for; r->poff is there (bg_result_map_pairs) and the total is not 0. The
// status word is cleared before and read by bg_pairs_status
static int pairs_fill(bg_ctx* c, bg_result* r, int64_t* ref_rows, int64_t* map_rows, double* vals) {
  const bg_table* R = r->set->t[r->tab];
  const bg_table* M = r->set->t[r->map_tab];
  PairArgs A;
  A.RS = R->ks, A.RE = R->ke, A.nr = r->n;
  A.MS = M->ks, A.ME = M->ke, A.nm = M->n;
  A.crit = r->mopts.faster ? BG_OVR_FAST : r->mopts.criterion;  // --faster: the deque is the window
  A.ovr = (int64_t)r->mopts.overlap_bp;
  A.range = (int64_t)r->mopts.range_bp;
  A.perc = r->perc;
  A.L = r->win_L, A.touch = r->win_touch;
  A.wlo = r->wlo, A.whi = r->whi;
  A.zin = r->zin, A.zout = r->zout;
  A.lrows = r->lrows;
  A.off = r->poff;
  A.ref_rows = ref_rows, A.map_rows = map_rows;
  A.SC = M->score, A.vals = vals;
  A.st = c->dstat;
  BG_HIP(c, hipMemsetAsync(&c->dstat->first_bad, 0xff, 8, c->stream));
  const dim3 g(bg_blocks(r->n, BG_NT)), b(BG_NT);
  if (A.lrows.ncls > 16) BG_LAUNCH(c, "k_pairs_rows", k_pairs_rows<BG_LONG_MAXC>, g, b, A);
  else if (A.lrows.ncls > 4) BG_LAUNCH(c, "k_pairs_rows", k_pairs_rows<16>, g, b, A);
  else if (A.lrows.ncls) BG_LAUNCH(c, "k_pairs_rows", k_pairs_rows<4>, g, b, A);
  else BG_LAUNCH(c, "k_pairs_flat", k_pairs_flat, g, b, A);
  BG_HIP(c, hipGetLastError());
  return 0;
}
int bg_pairs_scores(bg_ctx* c, bg_result* r, double* vals) {
  if (!r->set->t[r->map_tab]->score) return bg_fail(c, BG_E_INTERNAL, "pairs: the map table has no scores");
  return pairs_fill(c, r, nullptr, nullptr, vals);
}
int bg_pairs_status(bg_ctx* c) {
  BG_HIP(c, hipMemcpyAsync(c->hstat, c->dstat, sizeof(bg_dstatus), hipMemcpyDeviceToHost, c->stream));
  BG_HIP(c, hipStreamSynchronize(c->stream));
  if (c->hstat->first_bad != ~0ULL)
    return bg_fail(c, BG_E_INTERNAL, "pairs: reference row " + std::to_string(c->hstat->first_bad >> 8) +
                                         " on: another number of members written than counted");
  return 0;
}

extern "C" int bg_result_export_map_pairs(bg_ctx* c, bg_result* r, int64_t* offsets, int64_t* ref_rows,
                                          int64_t* map_rows, uint64_t cap) {
  if (!c || !r) return BG_E_ARG;
  uint64_t total = 0;
  int rc = bg_result_map_pairs(c, r, &total);
  if (rc) return rc;
  const bool fill = ref_rows || map_rows;
  if (fill && cap < total)
    return bg_fail(c, BG_E_ARG, "pairs: room for " + std::to_string(cap) + " pairs, the result has " +
                                    std::to_string(total));
  for (const void* p : {(const void*)offsets, (const void*)ref_rows, (const void*)map_rows})
    if ((uintptr_t)p & 15) return bg_fail(c, BG_E_ARG, "pairs: device columns must be 16-byte aligned");
  if (offsets) {
    BG_LAUNCH(c, "k_pairs_offsets", k_pairs_offsets, dim3(bg_blocks(r->n + 1, BG_NT)), dim3(BG_NT),
              (const uint64_t*)r->poff, r->n + 1, offsets);
    BG_HIP(c, hipGetLastError());
  }
  if (!fill || !total) return 0;
  if ((rc = pairs_fill(c, r, ref_rows, map_rows, nullptr))) return rc;
  if ((rc = bg_pairs_status(c))) return rc;
  bg_mark(c, "pairs");
  return 0;
}
