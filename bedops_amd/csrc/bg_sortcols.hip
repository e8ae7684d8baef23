// bg_sortcols.hip — bg_sort_columns: one columnar input (chrom index, start, end[, score]) put
// into the order bg_load_columns accepts, on the GPU (include/bedgpu.h).
//
//   k_sc_key     one pass over chrom / start / end: the row checks, max start, max (end - start)
//                and "is the input in order already"; one host fetch of that status follows and
//                bg_sort_columns_plan (bg_sortplan.h) decides the rest
//   k_sc_pack    packed plan: rank << (bs + bl) | start << bl | len, payload = row index
//                two rounds:  len first, then (k_sc_key2) rank << bs | start gathered through
//                the payload of round 1
//   digit passes bg_sort_u64_bits (bg_sort.hip) with the plan's widths
//   k_sc_gather  payload -> order and the requested columns, in one pass
//
// The kernels follow k_cols_key (bg_columns.hip): BG_NT threads, each lane SC_ROWS consecutive
// rows so that contiguous loads and stores are 16 bytes wide, a persistent grid, no scratch. The
// caller's arrays are touched by kernels only (they may belong to another HIP runtime,
// DESIGN.md §3.3); the caller's output buffers are 16-byte aligned like its input arrays.
#include <stdlib.h>

#include "bg_internal.h"
#include "bg_sortplan.h"

// consecutive rows per lane and rows per workgroup round, as k_cols_key
#define SC_ROWS 4
#define SC_CHUNK (BG_NT * SC_ROWS)
// name -> strcmp rank entries kept in LDS (8 KiB); past that the table is read from memory
#define SC_LDS_NAMES 2048
// a chrom index outside names
enum { ERR_SC_CHROM = 7 };

struct ScStatus {
  unsigned long long first_bad;  // min over bad rows of (row << 8) | code; ~0 if none
  unsigned long long max_start;
  unsigned long long max_len;    // max (end - start)
  unsigned long long unsorted;   // some row's (rank, start, end) is below its predecessor's
};

struct ScCols {
  const int32_t* chrom;
  const int64_t* start;
  const int64_t* end;
  const double* score;   // k_sc_gather only (null: no scores)
  uint64_t n;
  const uint32_t* rank;  // caller's chrom index -> strcmp rank of its name
  uint32_t nnames;
};

__device__ __forceinline__ void sc_report(ScStatus* st, uint64_t row, int code) {
  atomicMin(&st->first_bad, (unsigned long long)((row << 8) | (uint64_t)code));
}

// 4 consecutive rows of one lane: 16-byte loads when all four exist
__device__ __forceinline__ void sc_load(const ScCols& A, uint64_t i0, int32_t* cg, int64_t* s, int64_t* e) {
  if (i0 + SC_ROWS <= A.n) {
    const int4 cv = *reinterpret_cast<const int4*>(A.chrom + i0);
    const longlong2 s0 = *reinterpret_cast<const longlong2*>(A.start + i0);
    const longlong2 s1 = *reinterpret_cast<const longlong2*>(A.start + i0 + 2);
    const longlong2 e0 = *reinterpret_cast<const longlong2*>(A.end + i0);
    const longlong2 e1 = *reinterpret_cast<const longlong2*>(A.end + i0 + 2);
    cg[0] = cv.x, cg[1] = cv.y, cg[2] = cv.z, cg[3] = cv.w;
    s[0] = s0.x, s[1] = s0.y, s[2] = s1.x, s[3] = s1.y;
    e[0] = e0.x, e[1] = e0.y, e[2] = e1.x, e[3] = e1.y;
  } else {  // the input's last rows
#pragma unroll
    for (int j = 0; j < SC_ROWS; ++j) {
      const bool in = i0 + j < A.n;
      cg[j] = in ? A.chrom[i0 + j] : 0;
      s[j] = in ? A.start[i0 + j] : 0;
      e[j] = in ? A.end[i0 + j] : 0;
    }
  }
}

// One pass, 20 B read per row and nothing written but the status. A workgroup takes `per_wg`
// consecutive chunks; the (rank << 40 | start, end) pair before a lane's first row comes from
// the lane below, the wave below through LDS and the round before through registers of thread
// 0, exactly as k_cols_key carries its key (two alternating LDS slots, one barrier per round).
// A row with a bad chrom index never indexes the rank table; a row that fails a check is
// reported and the call ends before any other kernel sees it.
template <bool LDSMAP>
__global__ void __launch_bounds__(BG_NT) k_sc_key(ScCols A, ScStatus* st, uint64_t per_wg) {
  __shared__ uint32_t smap[LDSMAP ? SC_LDS_NAMES : 1];
  __shared__ int64_t wlast[2][BG_NT / 64][2];
  if (LDSMAP) {
    for (uint32_t k = threadIdx.x; k < A.nnames; k += BG_NT) smap[k] = A.rank[k];
    __syncthreads();
  }
  const uint32_t* map = LDSMAP ? smap : A.rank;
  const int lane = bg_lane(), w = bg_wave();
  const uint64_t nchunks = (A.n + SC_CHUNK - 1) / SC_CHUNK;
  const uint64_t c0 = (uint64_t)blockIdx.x * per_wg;
  const uint64_t c1 = min(c0 + per_wg, nchunks);
  int64_t ms = 0, ml = 0;
  bool uns = false;
  uint32_t round = 0;
  int64_t carry_k = LLONG_MIN, carry_e = LLONG_MIN;  // thread 0: the last row of the round before
  for (uint64_t ch = c0; ch < c1; ++ch, ++round) {
    const uint64_t i0 = ch * SC_CHUNK + (uint64_t)threadIdx.x * SC_ROWS;
    int32_t cg[SC_ROWS];
    int64_t s[SC_ROWS], e[SC_ROWS], k[SC_ROWS];
    sc_load(A, i0, cg, s, e);
#pragma unroll
    for (int j = 0; j < SC_ROWS; ++j) {
      const uint64_t i = i0 + j;
      const bool badc = (uint32_t)cg[j] >= A.nnames;
      k[j] = (badc ? 0 : (int64_t)map[cg[j]] << BG_KEY_SHIFT) | (s[j] & BG_COORD_MASK);
      if (i < A.n) {
        if (badc) sc_report(st, i, ERR_SC_CHROM);
        if (s[j] < 0 || e[j] < 0 || (uint64_t)e[j] > BG_KEY_COORD_MAX || s[j] > e[j]) {
          sc_report(st, i, ERR_RANGE);
        } else {
          ms = max(ms, s[j]);
          ml = max(ml, e[j] - s[j]);
        }
      }
    }
    // the row before this lane's first row
    if (lane == 63) wlast[round & 1][w][0] = k[SC_ROWS - 1], wlast[round & 1][w][1] = e[SC_ROWS - 1];
    int64_t pk = __shfl_up(k[SC_ROWS - 1], 1, 64), pe = __shfl_up(e[SC_ROWS - 1], 1, 64);
    __syncthreads();
    if (lane == 0) {
      if (w > 0) {
        pk = wlast[round & 1][w - 1][0], pe = wlast[round & 1][w - 1][1];
      } else if (round > 0) {
        pk = carry_k, pe = carry_e;
      } else if (i0 > 0) {  // the span's first row: its predecessor belongs to another workgroup
        const int32_t pc = A.chrom[i0 - 1];
        pk = ((uint32_t)pc < A.nnames ? (int64_t)map[pc] << BG_KEY_SHIFT : 0) | (A.start[i0 - 1] & BG_COORD_MASK);
        pe = A.end[i0 - 1];
      } else {
        pk = pe = LLONG_MIN;  // row 0 has none
      }
      if (w == 0) carry_k = wlast[round & 1][BG_NT / 64 - 1][0], carry_e = wlast[round & 1][BG_NT / 64 - 1][1];
    }
#pragma unroll
    for (int j = 0; j < SC_ROWS; ++j) {
      if (i0 + j < A.n) uns |= k[j] < pk || (k[j] == pk && e[j] < pe);
      pk = k[j], pe = e[j];
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    ms = max(ms, (int64_t)__shfl_xor(ms, d, 64));
    ml = max(ml, (int64_t)__shfl_xor(ml, d, 64));
  }
  const bool anyuns = __ballot(uns) != 0;
  if (lane == 0) {  // one atomic per wave and value, and only where it raises the value
    if ((unsigned long long)ms > *(volatile unsigned long long*)&st->max_start) atomicMax(&st->max_start, (unsigned long long)ms);
    if ((unsigned long long)ml > *(volatile unsigned long long*)&st->max_len) atomicMax(&st->max_len, (unsigned long long)ml);
    if (anyuns && !*(volatile unsigned long long*)&st->unsorted) atomicOr(&st->unsorted, 1ULL);
  }
}

// Round-0 keys of checked rows (20 B read, 12 B written per row). packed: rank << sh_rank |
// start << sh_start | len; else len alone. sh_rank == 64 only with one name (rank 0: no shift).
template <bool LDSMAP>
__global__ void __launch_bounds__(BG_NT) k_sc_pack(ScCols A, bool packed, int sh_rank, int sh_start,
                                                   uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
  __shared__ uint32_t smap[LDSMAP ? SC_LDS_NAMES : 1];
  if (LDSMAP) {
    for (uint32_t k = threadIdx.x; k < A.nnames; k += BG_NT) smap[k] = A.rank[k];
    __syncthreads();
  }
  const uint32_t* map = LDSMAP ? smap : A.rank;
  const uint64_t nchunks = (A.n + SC_CHUNK - 1) / SC_CHUNK;
  for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const uint64_t i0 = ch * SC_CHUNK + (uint64_t)threadIdx.x * SC_ROWS;
    int32_t cg[SC_ROWS];
    int64_t s[SC_ROWS], e[SC_ROWS];
    uint64_t k[SC_ROWS];
    sc_load(A, i0, cg, s, e);
#pragma unroll
    for (int j = 0; j < SC_ROWS; ++j) {
      k[j] = (uint64_t)(e[j] - s[j]);
      if (packed) {
        const uint64_t r = (uint32_t)cg[j] < A.nnames ? map[cg[j]] : 0;
        k[j] |= ((uint64_t)s[j] << sh_start) | (sh_rank < 64 ? r << sh_rank : 0);
      }
    }
    if (i0 + SC_ROWS <= A.n) {
      *reinterpret_cast<ulonglong2*>(key + i0) = make_ulonglong2(k[0], k[1]);
      *reinterpret_cast<ulonglong2*>(key + i0 + 2) = make_ulonglong2(k[2], k[3]);
      *reinterpret_cast<uint4*>(val + i0) = make_uint4((uint32_t)i0, (uint32_t)i0 + 1, (uint32_t)i0 + 2, (uint32_t)i0 + 3);
    } else {
#pragma unroll
      for (int j = 0; j < SC_ROWS; ++j)
        if (i0 + j < A.n) key[i0 + j] = k[j], val[i0 + j] = (uint32_t)(i0 + j);
    }
  }
}

// Round-1 keys: rank << bs | start of the row that round 0 left at each position
template <bool LDSMAP>
__global__ void __launch_bounds__(BG_NT) k_sc_key2(ScCols A, int bs, const uint32_t* __restrict__ val,
                                                   uint64_t* __restrict__ key) {
  __shared__ uint32_t smap[LDSMAP ? SC_LDS_NAMES : 1];
  if (LDSMAP) {
    for (uint32_t k = threadIdx.x; k < A.nnames; k += BG_NT) smap[k] = A.rank[k];
    __syncthreads();
  }
  const uint32_t* map = LDSMAP ? smap : A.rank;
  const uint64_t nchunks = (A.n + SC_CHUNK - 1) / SC_CHUNK;
  for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const uint64_t i0 = ch * SC_CHUNK + (uint64_t)threadIdx.x * SC_ROWS;
    const bool full = i0 + SC_ROWS <= A.n;
    uint32_t p[SC_ROWS];
    if (full) {
      const uint4 v = *reinterpret_cast<const uint4*>(val + i0);
      p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < SC_ROWS; ++j) p[j] = i0 + j < A.n ? val[i0 + j] : 0;
    }
    uint64_t k[SC_ROWS];
#pragma unroll
    for (int j = 0; j < SC_ROWS; ++j) {
      k[j] = 0;
      if (i0 + j < A.n) {  // (p[j] < n: a row index the pack kernel wrote)
        const int32_t cg = A.chrom[p[j]];
        const uint64_t r = (uint32_t)cg < A.nnames ? map[cg] : 0;
        k[j] = (r << bs) | (uint64_t)A.start[p[j]];
      }
    }
    if (full) {
      *reinterpret_cast<ulonglong2*>(key + i0) = make_ulonglong2(k[0], k[1]);
      *reinterpret_cast<ulonglong2*>(key + i0 + 2) = make_ulonglong2(k[2], k[3]);
    } else {
#pragma unroll
      for (int j = 0; j < SC_ROWS; ++j)
        if (i0 + j < A.n) key[i0 + j] = k[j];
    }
  }
}

struct ScOut {
  int64_t* order;
  int32_t* chrom;
  int64_t* start;
  int64_t* end;
  double* score;
};

// Position k takes input row val[k] (IDENT: row k itself, the input was in order): order and
// the requested columns in one pass; a null output is skipped. Reads through val are gathers,
// the stores (and the IDENT reads) are 16 bytes wide.
template <bool IDENT>
__global__ void __launch_bounds__(BG_NT) k_sc_gather(ScCols A, const uint32_t* __restrict__ val, ScOut O) {
  const uint64_t nchunks = (A.n + SC_CHUNK - 1) / SC_CHUNK;
  for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const uint64_t i0 = ch * SC_CHUNK + (uint64_t)threadIdx.x * SC_ROWS;
    const bool full = i0 + SC_ROWS <= A.n;
    uint64_t p[SC_ROWS];
    int32_t cg[SC_ROWS];
    int64_t s[SC_ROWS], e[SC_ROWS];
    double sc[SC_ROWS];
    if (IDENT) {
#pragma unroll
      for (int j = 0; j < SC_ROWS; ++j) p[j] = i0 + j;
      sc_load(A, i0, cg, s, e);
      if (O.score) {
        if (full) {
          const double2 v0 = *reinterpret_cast<const double2*>(A.score + i0);
          const double2 v1 = *reinterpret_cast<const double2*>(A.score + i0 + 2);
          sc[0] = v0.x, sc[1] = v0.y, sc[2] = v1.x, sc[3] = v1.y;
        } else {
#pragma unroll
          for (int j = 0; j < SC_ROWS; ++j) sc[j] = i0 + j < A.n ? A.score[i0 + j] : 0.0;
        }
      }
    } else {
      if (full) {
        const uint4 v = *reinterpret_cast<const uint4*>(val + i0);
        p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < SC_ROWS; ++j) p[j] = i0 + j < A.n ? val[i0 + j] : 0;
      }
#pragma unroll
      for (int j = 0; j < SC_ROWS; ++j) {
        const bool in = i0 + j < A.n;  // (p[j] < n: a row index the pack kernel wrote)
        cg[j] = (in && O.chrom) ? A.chrom[p[j]] : 0;
        s[j] = (in && O.start) ? A.start[p[j]] : 0;
        e[j] = (in && O.end) ? A.end[p[j]] : 0;
        sc[j] = (in && O.score) ? A.score[p[j]] : 0.0;
      }
    }
    if (full) {
      if (O.order) {
        *reinterpret_cast<longlong2*>(O.order + i0) = make_longlong2((int64_t)p[0], (int64_t)p[1]);
        *reinterpret_cast<longlong2*>(O.order + i0 + 2) = make_longlong2((int64_t)p[2], (int64_t)p[3]);
      }
      if (O.chrom) *reinterpret_cast<int4*>(O.chrom + i0) = make_int4(cg[0], cg[1], cg[2], cg[3]);
      if (O.start) {
        *reinterpret_cast<longlong2*>(O.start + i0) = make_longlong2(s[0], s[1]);
        *reinterpret_cast<longlong2*>(O.start + i0 + 2) = make_longlong2(s[2], s[3]);
      }
      if (O.end) {
        *reinterpret_cast<longlong2*>(O.end + i0) = make_longlong2(e[0], e[1]);
        *reinterpret_cast<longlong2*>(O.end + i0 + 2) = make_longlong2(e[2], e[3]);
      }
      if (O.score) {
        *reinterpret_cast<double2*>(O.score + i0) = make_double2(sc[0], sc[1]);
        *reinterpret_cast<double2*>(O.score + i0 + 2) = make_double2(sc[2], sc[3]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < SC_ROWS; ++j)
        if (i0 + j < A.n) {
          if (O.order) O.order[i0 + j] = (int64_t)p[j];
          if (O.chrom) O.chrom[i0 + j] = cg[j];
          if (O.start) O.start[i0 + j] = s[j];
          if (O.end) O.end[i0 + j] = e[j];
          if (O.score) O.score[i0 + j] = sc[j];
        }
    }
  }
}

// caller's chrom index -> rank of its name among the input's names in strcmp order (the names
// were checked: none empty, no duplicates)
static void sc_rank_table(const char* const* names, uint32_t nnames, uint32_t* rank) {
  std::vector<uint32_t> idx(nnames);
  for (uint32_t k = 0; k < nnames; ++k) idx[k] = k;
  std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return strcmp(names[a], names[b]) < 0; });
  for (uint32_t r = 0; r < nnames; ++r) rank[idx[r]] = r;
}

static unsigned sc_grid(bg_ctx* c, const void* kern, uint64_t nchunks) {
  return (unsigned)std::min<uint64_t>(nchunks, bg_cols_grid(c, kern));
}

static int sc_sort(bg_ctx* c, const bg_columns& I, const ScOut& O) {
  const uint64_t n = I.n;
  const uint32_t m1 = I.nnames ? I.nnames : 1;
  BgHold hold(c);
  bg_pin_reset(c);
  ScCols A;
  A.chrom = I.chrom, A.start = I.start, A.end = I.end, A.score = O.score ? I.score : nullptr;
  A.n = n, A.nnames = I.nnames;
  uint32_t* drank = hold.alloc<uint32_t>(m1);
  ScStatus* dst = hold.alloc<ScStatus>(1);
  uint32_t* hrank = (uint32_t*)bg_pin_take(c, 4ull * m1);
  ScStatus* hst = (ScStatus*)bg_pin_take(c, sizeof(ScStatus));
  if (!hold.ok() || !hrank || !hst) return BG_E_NOMEM;
  if (!I.on_device) {  // host arrays: staged in device temporaries
    int32_t* dc = hold.alloc<int32_t>(n);
    int64_t* ds = hold.alloc<int64_t>(n);
    int64_t* de = hold.alloc<int64_t>(n);
    double* dv = A.score ? hold.alloc<double>(n) : nullptr;
    if (!hold.ok()) return BG_E_NOMEM;
    BG_HIP(c, hipMemcpyAsync(dc, I.chrom, 4 * n, hipMemcpyHostToDevice, c->stream));
    BG_HIP(c, hipMemcpyAsync(ds, I.start, 8 * n, hipMemcpyHostToDevice, c->stream));
    BG_HIP(c, hipMemcpyAsync(de, I.end, 8 * n, hipMemcpyHostToDevice, c->stream));
    if (dv) BG_HIP(c, hipMemcpyAsync(dv, I.score, 8 * n, hipMemcpyHostToDevice, c->stream));
    A.chrom = dc, A.start = ds, A.end = de, A.score = dv;
  }
  hrank[0] = 0;
  sc_rank_table(I.names, I.nnames, hrank);
  A.rank = drank;
  hst->first_bad = ~0ULL;
  hst->max_start = hst->max_len = hst->unsorted = 0;
  BG_HIP(c, hipMemcpyAsync(drank, hrank, 4ull * m1, hipMemcpyHostToDevice, c->stream));
  BG_HIP(c, hipMemcpyAsync(dst, hst, sizeof(ScStatus), hipMemcpyHostToDevice, c->stream));
  const bool lds = I.nnames <= SC_LDS_NAMES;
  const uint64_t nchunks = (n + SC_CHUNK - 1) / SC_CHUNK;
  const dim3 block(BG_NT);
  {
    const void* kern = lds ? (const void*)k_sc_key<true> : (const void*)k_sc_key<false>;
    const uint64_t g = bg_cols_grid(c, kern), per_wg = (nchunks + g - 1) / g;
    const dim3 grid((unsigned)((nchunks + per_wg - 1) / per_wg));
    if (lds) BG_LAUNCH(c, "k_sc_key", k_sc_key<true>, grid, block, A, dst, per_wg);
    else BG_LAUNCH(c, "k_sc_key", k_sc_key<false>, grid, block, A, dst, per_wg);
    BG_HIP(c, hipGetLastError());
  }
  // the call's one host round trip (the device read the status image above first: stream order)
  BG_HIP(c, hipMemcpyAsync(hst, dst, sizeof(ScStatus), hipMemcpyDeviceToHost, c->stream));
  BG_HIP(c, hipStreamSynchronize(c->stream));
  if (hst->first_bad != ~0ULL) {
    const bool chrom = (int)(hst->first_bad & 0xff) == ERR_SC_CHROM;
    char msg[192];
    snprintf(msg, sizeof(msg), "sort_columns: row %llu: %s", (unsigned long long)(hst->first_bad >> 8),
             chrom ? "chrom index outside names" : "coordinate out of range (negative, end < start or >= 2^40)");
    return bg_fail(c, chrom ? BG_E_ARG : BG_E_RANGE, msg);
  }
  uint32_t* val = nullptr;
  if (n >= 2 && hst->unsorted) {
    const bg_sort_plan P = bg_sort_columns_plan(n, I.nnames, hst->max_start, hst->max_len);
    uint64_t* key = hold.alloc<uint64_t>(n);
    val = hold.alloc<uint32_t>(n);
    if (!hold.ok()) return BG_E_NOMEM;
    {
      const void* kern = lds ? (const void*)k_sc_pack<true> : (const void*)k_sc_pack<false>;
      const dim3 grid(sc_grid(c, kern, nchunks));
      if (lds) BG_LAUNCH(c, "k_sc_pack", k_sc_pack<true>, grid, block, A, P.packed, P.bs + P.bl, P.bl, key, val);
      else BG_LAUNCH(c, "k_sc_pack", k_sc_pack<false>, grid, block, A, P.packed, P.bs + P.bl, P.bl, key, val);
      BG_HIP(c, hipGetLastError());
    }
    int rc = bg_sort_u64_bits(c, key, val, n, P.bits[0]);
    if (rc) return rc;
    if (!P.packed) {
      const void* kern = lds ? (const void*)k_sc_key2<true> : (const void*)k_sc_key2<false>;
      const dim3 grid(sc_grid(c, kern, nchunks));
      if (lds) BG_LAUNCH(c, "k_sc_key2", k_sc_key2<true>, grid, block, A, P.bs, (const uint32_t*)val, key);
      else BG_LAUNCH(c, "k_sc_key2", k_sc_key2<false>, grid, block, A, P.bs, (const uint32_t*)val, key);
      BG_HIP(c, hipGetLastError());
      if ((rc = bg_sort_u64_bits(c, key, val, n, P.bits[1]))) return rc;
    }
    hold.drop(key);
  }
  if (O.order || O.chrom || O.start || O.end || O.score) {
    const void* kern = val ? (const void*)k_sc_gather<false> : (const void*)k_sc_gather<true>;
    const dim3 grid(sc_grid(c, kern, nchunks));
    if (val) BG_LAUNCH(c, "k_sc_gather", k_sc_gather<false>, grid, block, A, (const uint32_t*)val, O);
    else BG_LAUNCH(c, "k_sc_gather", k_sc_gather<true>, grid, block, A, (const uint32_t*)val, O);
    BG_HIP(c, hipGetLastError());
  }
  bg_mark(c, "sort_columns");
  return 0;
}

extern "C" int bg_sort_columns(bg_ctx* c, const bg_columns* in, int64_t* order, int32_t* chrom, int64_t* start,
                               int64_t* end, double* score) {
  if (!c || !in) return BG_E_ARG;
  int rc = bg_cols_check_args(c, 1, in, false);  // (reads no row)
  if (rc) return rc;
  if (in->n > 0xffffffffULL) return bg_fail(c, BG_E_UNSUPPORTED, "sort_columns: more than 2^32 - 1 rows");
  if (score && !in->score) return bg_fail(c, BG_E_ARG, "sort_columns: a score output needs a BG_BED5 input");
  for (const void* p : {(const void*)order, (const void*)chrom, (const void*)start, (const void*)end, (const void*)score})
    if ((uintptr_t)p & 15) return bg_fail(c, BG_E_ARG, "sort_columns: output buffers must be 16-byte aligned");
  if (!in->n) return 0;
  ScOut O;
  O.order = order, O.chrom = chrom, O.start = start, O.end = end, O.score = score;
  rc = sc_sort(c, *in, O);
  if (rc) (void)hipStreamSynchronize(c->stream);  // queued copies may still read the caller's arrays
  return rc;
}
