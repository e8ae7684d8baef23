// bg_closest_export.hip — a closest-features result as columns (include/bedgpu.h,
// bg_result_export_closest): per reference row the query rows the text route prints on the left
// and on the right (bg_result::left / right, bg_closest.hip), the distances --dist prints for
// them, and the one element and distance --shortest --dist prints. No text is read, so the
// tables may come from bg_load_columns (bg_closest_rows).
//
// k_closest_export: one pass over the reference rows, a persistent grid over chunks of
// BG_COL_CHUNK rows (bg_colkern.h). A lane takes 4 consecutive rows: the reference keys, left
// and right come in and every asked-for column goes out in 16-byte accesses (row by row among
// the last rows). The candidates' keys cs[L], ce[L], cs[R], ce[R] are gathers; L and R are
// near-monotone in the row, so neighbouring lanes hit the same lines. A column that is not
// asked for costs no store, and a candidate no asked-for column depends on costs no gather:
// left_rows / right_rows need none, left_dist the left one, right_dist the right one, the
// shortest pair both. An index outside [-1, nc) is never dereferenced, and a candidate on
// another chromosome than its row gives no distance; either is reported (ERR_CLOSEST).
#include <climits>

#include "bg_colkern.h"

struct ClxArgs {
  const int64_t* qs;  // reference rows, keyed
  const int64_t* qe;
  uint64_t nq;
  const int64_t* cs;  // query rows (the candidates), keyed
  const int64_t* ce;
  uint64_t nc;
  const int64_t* left;  // bg_result::left / right
  const int64_t* right;
  int64_t* o_lrow;  // the caller's columns; null: skipped
  int64_t* o_rrow;
  int64_t* o_ldist;
  int64_t* o_rdist;
  int64_t* o_srow;
  int64_t* o_sdist;
  bg_dstatus* st;
};

// getDistance(x, ref) of closest-features (ClosestFeature.cpp:244-255), same chromosome: cf_dist
// of bg_format.hip
__device__ __forceinline__ int64_t clx_dist(int64_t xs, int64_t xe, int64_t bs, int64_t be) {
  if (xe <= bs) return -((bs - xe) + 1);
  if (be <= xs) return (xs - be) + 1;
  return 0;
}

// What PrintShortest prints (Printers.hpp:112-200): render_closest's `shortest` branch
// (bg_format.hip), decision by decision, with the element and the distance returned instead of
// printed. A second copy on purpose: the formatter's branch is the hot path of
// `bench.py --workload closest` (--closest), and it stays as it was compiled.
// which: 0 none, 1 the left candidate, 2 the right one.
__device__ __forceinline__ int clx_shortest(bool hasL, int64_t ls, int64_t le, bool hasR, int64_t rs, int64_t re,
                                            int64_t bs, int64_t be, int64_t& dist) {
  dist = BG_DIST_NA;
  if (!hasL && !hasR) return 0;
  int64_t d1 = LLONG_MAX, d2 = LLONG_MAX;
  if (hasL) {
    if (le <= bs) {  // <= as getDistance
      d1 = (bs - le) + 1;
      if (!hasR) { dist = clx_dist(ls, le, bs, be); return 1; }
    } else {  // overlapping left: printed with distance 0
      dist = 0;
      return 1;
    }
  }
  if (hasR) {
    if (!hasL) { dist = clx_dist(rs, re, bs, be); return 2; }
    if (be <= rs) d2 = (rs - be) + 1;
    else { dist = 0; return 2; }
  }
  if (d1 <= d2) { dist = clx_dist(ls, le, bs, be); return 1; }
  dist = clx_dist(rs, re, bs, be);
  return 2;
}

// candidate x of reference row k (start key bs): is it a row (x >= 0, in range)? With `need` its
// keys are gathered and its chromosome compared with the row's. What fails is reported and
// counts as no row.
__device__ __forceinline__ bool clx_cand(const ClxArgs& A, uint64_t k, int64_t bs, int64_t x, bool need, int64_t& xs,
                                         int64_t& xe) {
  xs = xe = 0;
  if (x == -1) return false;
  if (x < -1 || (uint64_t)x >= A.nc) {
    bg_report(A.st, k, ERR_CLOSEST);
    return false;
  }
  if (!need) return true;
  xs = A.cs[x];
  xe = A.ce[x];
  if ((xs >> BG_KEY_SHIFT) != (bs >> BG_KEY_SHIFT)) {
    bg_report(A.st, k, ERR_CLOSEST);
    return false;
  }
  return true;
}

__global__ void __launch_bounds__(BG_NT) k_closest_export(ClxArgs A) {
  const bool shortest = A.o_srow || A.o_sdist;
  const bool needL = A.o_ldist || shortest, needR = A.o_rdist || shortest;
  const uint64_t nchunks = (A.nq + BG_COL_CHUNK - 1) / BG_COL_CHUNK;
  for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const uint64_t i0 = ch * BG_COL_CHUNK + (uint64_t)threadIdx.x * BG_COL_ROWS;
    if (i0 >= A.nq) continue;  // (no barrier in here)
    int64_t bs[BG_COL_ROWS], be[BG_COL_ROWS] = {}, L[BG_COL_ROWS], R[BG_COL_ROWS];
    col_load4(A.left, i0, A.nq, L);
    col_load4(A.right, i0, A.nq, R);
    col_load4(A.qs, i0, A.nq, bs);
    if (needL || needR) col_load4(A.qe, i0, A.nq, be);
    int64_t lrow[BG_COL_ROWS], rrow[BG_COL_ROWS], ldist[BG_COL_ROWS], rdist[BG_COL_ROWS], srow[BG_COL_ROWS],
        sdist[BG_COL_ROWS];
#pragma unroll
    for (int j = 0; j < BG_COL_ROWS; ++j) {
      const bool live = i0 + j < A.nq;  // (past the input's end col_load4 gave zeros: no row 0 is touched for them)
      int64_t ls = 0, le = 0, rs = 0, re = 0;
      const bool hasL = live && clx_cand(A, i0 + j, bs[j], L[j], needL, ls, le);
      const bool hasR = live && clx_cand(A, i0 + j, bs[j], R[j], needR, rs, re);
      lrow[j] = hasL ? L[j] : -1;
      rrow[j] = hasR ? R[j] : -1;
      ldist[j] = hasL && needL ? clx_dist(ls, le, bs[j], be[j]) : BG_DIST_NA;
      rdist[j] = hasR && needR ? clx_dist(rs, re, bs[j], be[j]) : BG_DIST_NA;
      srow[j] = -1;
      sdist[j] = BG_DIST_NA;
      if (shortest) {
        const int w = clx_shortest(hasL, ls, le, hasR, rs, re, bs[j], be[j], sdist[j]);
        srow[j] = w == 1 ? L[j] : (w == 2 ? R[j] : -1);
      }
    }
    if (A.o_lrow) col_store4(A.o_lrow, i0, A.nq, lrow);
    if (A.o_rrow) col_store4(A.o_rrow, i0, A.nq, rrow);
    if (A.o_ldist) col_store4(A.o_ldist, i0, A.nq, ldist);
    if (A.o_rdist) col_store4(A.o_rdist, i0, A.nq, rdist);
    if (A.o_srow) col_store4(A.o_srow, i0, A.nq, srow);
    if (A.o_sdist) col_store4(A.o_sdist, i0, A.nq, sdist);
  }
}

extern "C" int bg_result_export_closest(bg_ctx* c, bg_result* r, int64_t* left_rows, int64_t* right_rows,
                                        int64_t* left_dist, int64_t* right_dist, int64_t* shortest_rows,
                                        int64_t* shortest_dist) {
  if (!c || !r) return BG_E_ARG;
  if (r->kind != RES_CLOSEST) return bg_fail(c, BG_E_ARG, "export: not a closest-features result");
  bool any = false;
  for (const void* p : {(const void*)left_rows, (const void*)right_rows, (const void*)left_dist,
                        (const void*)right_dist, (const void*)shortest_rows, (const void*)shortest_dist}) {
    if ((uintptr_t)p & 15) return bg_fail(c, BG_E_ARG, "export: device columns must be 16-byte aligned");
    any |= p != nullptr;
  }
  if (!any || !r->n) return 0;
  const bg_table* Q = r->set->t[r->tab];
  const bg_table* C = r->set->t[r->tab2];
  ClxArgs A;
  A.qs = Q->ks, A.qe = Q->ke, A.nq = r->n;
  A.cs = C->ks, A.ce = C->ke, A.nc = C->n;
  A.left = r->left, A.right = r->right;
  A.o_lrow = left_rows, A.o_rrow = right_rows;
  A.o_ldist = left_dist, A.o_rdist = right_dist;
  A.o_srow = shortest_rows, A.o_sdist = shortest_dist;
  A.st = c->dstat;
  BG_HIP(c, hipMemsetAsync(&c->dstat->first_bad, 0xff, 8, c->stream));
  const unsigned grid = bg_cols_stride_grid(c, (const void*)k_closest_export, r->n);
  BG_LAUNCH(c, "k_closest_export", k_closest_export, dim3(grid), dim3(BG_NT), A);
  BG_HIP(c, hipGetLastError());
  BG_HIP(c, hipMemcpyAsync(c->hstat, c->dstat, sizeof(bg_dstatus), hipMemcpyDeviceToHost, c->stream));
  BG_HIP(c, hipStreamSynchronize(c->stream));
  if (c->hstat->first_bad != ~0ULL)
    return bg_fail(c, BG_E_INTERNAL, "export: reference row " + std::to_string(c->hstat->first_bad >> 8) +
                                         ": a chosen row outside the query table or on another chromosome");
  bg_mark(c, "closest-export");
  return 0;
}
