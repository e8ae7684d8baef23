// bg_colkern.h — what the column kernels share: bg_columns.hip (k_cols_key) and bg_sortcols.hip
// (k_sc_*) only. Device side: the 4-rows-per-lane access, the rank table in LDS and the
// predecessor carry. Host side: the <true>/<false> launch, the grids, the staging of host arrays
// and the row errors' text (defined in bg_columns.hip). DESIGN.md §3.3.
#pragma once
#include "bg_internal.h"

// consecutive rows per lane: one 16-B access of a 4-byte column, two of an 8-byte column
#define BG_COL_ROWS 4
// rows a workgroup takes per round
#define BG_COL_CHUNK (BG_NT * BG_COL_ROWS)
// rank table entries (caller's chromosome index -> rank) kept in LDS (8 KiB); past that the
// table is read from memory
#define BG_COL_LDS_NAMES 2048

// rows [i0, i0 + 4) of a 16-byte aligned column of n rows (i0 a multiple of 4): 16-byte
// accesses when all four exist; among the input's last rows `out` is 0 past n and nothing is
// stored past n
template <class T>
__device__ __forceinline__ void col_load4(const T* p, uint64_t i0, uint64_t n, T (&out)[BG_COL_ROWS]) {
  constexpr int W = 16 / sizeof(T);
  typedef T V __attribute__((ext_vector_type(W)));
  if (i0 + BG_COL_ROWS <= n) {
#pragma unroll
    for (int j = 0; j < BG_COL_ROWS; j += W) {
      const V v = *reinterpret_cast<const V*>(p + i0 + j);
#pragma unroll
      for (int k = 0; k < W; ++k) out[j + k] = v[k];
    }
  } else {
#pragma unroll
    for (int j = 0; j < BG_COL_ROWS; ++j) out[j] = i0 + j < n ? p[i0 + j] : T(0);
  }
}
template <class T>
__device__ __forceinline__ void col_store4(T* p, uint64_t i0, uint64_t n, const T (&v)[BG_COL_ROWS]) {
  constexpr int W = 16 / sizeof(T);
  typedef T V __attribute__((ext_vector_type(W)));
  if (i0 + BG_COL_ROWS <= n) {
#pragma unroll
    for (int j = 0; j < BG_COL_ROWS; j += W) {
      V o;
#pragma unroll
      for (int k = 0; k < W; ++k) o[k] = v[j + k];
      *reinterpret_cast<V*>(p + i0 + j) = o;
    }
  } else {
#pragma unroll
    for (int j = 0; j < BG_COL_ROWS; ++j)
      if (i0 + j < n) p[i0 + j] = v[j];
  }
}

// the rank table a kernel indexes: LDSMAP copies `table` into smap (BG_COL_LDS_NAMES entries,
// nnames at most that) and every thread of the workgroup passes the barrier in here
template <bool LDSMAP>
__device__ __forceinline__ const uint32_t* col_rank_map(uint32_t* smap, const uint32_t* table, uint32_t nnames) {
  if (!LDSMAP) return table;
  for (uint32_t k = threadIdx.x; k < nnames; k += BG_NT) smap[k] = table[k];
  __syncthreads();
  return smap;
}

// The predecessor carry of a kernel whose workgroup walks consecutive chunks, one per round:
// NV int64 values of the row before a lane's first row. They come from the lane below by
// __shfl_up, from the wave below through LDS, and from the round before through registers of
// thread 0: right after a round's barrier it reads the last wave's values from that round's
// slots and keeps them. The two sets of slots alternate by round, so a slot is next written two
// rounds later, after the barrier in between, which every read of it precedes: one barrier per
// round is enough. (With the cross-round values read from LDS a round late it would not be:
// the last wave could overwrite them first.) Every thread of the workgroup calls step() once
// in every round, also one whose rows are all past the input's end: the barrier is in there.
// What the workgroup has not seen, the row before its span, is the caller's: step() returns
// false to the one thread that needs it, with pred = LLONG_MIN (what row 0 keeps: no row).
template <int NV>
struct ColCarry {
  typedef int64_t Slots[2][BG_NT / 64][NV];  // the kernel's: __shared__ ColCarry<NV>::Slots
  int64_t keep[NV];  // thread 0: the last row of the round before
  uint32_t round = 0;
  __device__ __forceinline__ ColCarry() {
#pragma unroll
    for (int k = 0; k < NV; ++k) keep[k] = LLONG_MIN;
  }
  // last: this lane's last row; pred: the row before this lane's first row
  __device__ __forceinline__ bool step(Slots& slots, const int64_t (&last)[NV], int64_t (&pred)[NV]) {
    const int lane = bg_lane(), w = bg_wave();
    int64_t(&slot)[BG_NT / 64][NV] = slots[round & 1];
    if (lane == 63) {
#pragma unroll
      for (int k = 0; k < NV; ++k) slot[w][k] = last[k];
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) pred[k] = __shfl_up(last[k], 1, 64);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < NV; ++k) pred[k] = w > 0 ? slot[w - 1][k] : keep[k];
      if (w == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) keep[k] = slot[BG_NT / 64 - 1][k];
      }
    }
    return round++ > 0 || threadIdx.x != 0;
  }
};

// ---- host side ----

// Launches k<true> or k<false>, by `flag`, under BG_LAUNCH's `name`, with BG_NT threads. `grid`
// is an expression evaluated with `kern` naming the instantiation that runs (bg_cols_span_grid,
// bg_cols_stride_grid); the kernel's arguments are read after it.
#define BG_COL_LAUNCH(c, name, k, flag, grid, ...)                               \
  do {                                                                           \
    const bool _t = (flag);                                                      \
    const void* kern = _t ? (const void*)k<true> : (const void*)k<false>;        \
    const dim3 _g(grid);                                                         \
    if (_t) BG_LAUNCH(c, name, k<true>, _g, dim3(BG_NT), __VA_ARGS__);           \
    else BG_LAUNCH(c, name, k<false>, _g, dim3(BG_NT), __VA_ARGS__);             \
    BG_HIP(c, hipGetLastError());                                                \
  } while (0)

// workgroups of a persistent kernel that takes n > 0 rows in spans (*per_wg consecutive chunks
// of BG_COL_CHUNK rows each) / grid-strided chunk by chunk
unsigned bg_cols_span_grid(bg_ctx* c, const void* kern, uint64_t n, uint64_t* per_wg);
unsigned bg_cols_stride_grid(bg_ctx* c, const void* kern, uint64_t n);
// I's host arrays (n > 0 rows) copied into device temporaries of `hold`, which take their place
// in I: chrom, start, end, and score where `score`
int bg_cols_stage(bg_ctx* c, BgHold& hold, bg_columns& I, bool score);
// a row error of the column kernels (bg_dstatus.first_bad & 0xff): its text and API code
struct ColRowError {
  const char* what;
  int rc;
};
ColRowError bg_cols_row_error(int code);
