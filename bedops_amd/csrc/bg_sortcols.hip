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
// The kernels are built from the pieces k_cols_key (bg_columns.hip) is built from, bg_colkern.h:
// BG_NT threads, each lane BG_COL_ROWS consecutive rows so that contiguous loads and stores are
// 16 bytes wide, the rank table in LDS, a persistent grid, no scratch. The caller's arrays are
// touched by kernels only (they may belong to another HIP runtime); the
// caller's output buffers are 16-byte aligned like its input arrays.
#include <stdlib.h>

#include "bg_colkern.h"
#include "bg_sortplan.h"

// the names tests/test_gpu_sort_columns.py reads its shapes by: the shared values, nothing else
#define SC_ROWS 4
#define SC_LDS_NAMES 2048
static_assert(SC_ROWS == BG_COL_ROWS && SC_LDS_NAMES == BG_COL_LDS_NAMES, "bg_colkern.h holds the values");

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

// One pass, 20 B read per row and nothing written but the status. A workgroup takes `per_wg`
// consecutive chunks; the (rank << 40 | start, end) pair before a lane's first row: ColCarry.
// A row with a bad chrom index never indexes the rank table; a row that fails a check is
// reported and the call ends before any other kernel sees it.
template <bool LDSMAP>
__global__ void __launch_bounds__(BG_NT) k_sc_key(ScCols A, ScStatus* st, uint64_t per_wg) {
  __shared__ uint32_t smap[LDSMAP ? BG_COL_LDS_NAMES : 1];
  __shared__ ColCarry<2>::Slots wlast;
  const uint32_t* map = col_rank_map<LDSMAP>(smap, A.rank, A.nnames);
  const int lane = bg_lane();
  const uint64_t nchunks = (A.n + BG_COL_CHUNK - 1) / BG_COL_CHUNK;
  const uint64_t c0 = (uint64_t)blockIdx.x * per_wg;
  const uint64_t c1 = min(c0 + per_wg, nchunks);
  int64_t ms = 0, ml = 0;
  bool uns = false;
  ColCarry<2> carry;
  for (uint64_t ch = c0; ch < c1; ++ch) {
    const uint64_t i0 = ch * BG_COL_CHUNK + (uint64_t)threadIdx.x * BG_COL_ROWS;
    int32_t cg[BG_COL_ROWS];
    int64_t s[BG_COL_ROWS], e[BG_COL_ROWS], k[BG_COL_ROWS];
    col_load4(A.chrom, i0, A.n, cg);
    col_load4(A.start, i0, A.n, s);
    col_load4(A.end, i0, A.n, e);
#pragma unroll
    for (int j = 0; j < BG_COL_ROWS; ++j) {
      const uint64_t i = i0 + j;
      const bool badc = (uint32_t)cg[j] >= A.nnames;
      k[j] = (badc ? 0 : (int64_t)map[cg[j]] << BG_KEY_SHIFT) | (s[j] & BG_COORD_MASK);
      if (i < A.n) {
        if (badc) bg_report(&st->first_bad, i, ERR_COLS_CHROM);
        if (s[j] < 0 || e[j] < 0 || (uint64_t)e[j] > BG_KEY_COORD_MAX || s[j] > e[j]) {
          bg_report(&st->first_bad, i, ERR_RANGE);
        } else {
          ms = max(ms, s[j]);
          ml = max(ml, e[j] - s[j]);
        }
      }
    }
    // the row before this lane's first row (ColCarry; LLONG_MIN twice for row 0, which has none)
    int64_t p[2];
    if (!carry.step(wlast, {k[BG_COL_ROWS - 1], e[BG_COL_ROWS - 1]}, p) && i0 > 0) {
      // the span's first row: its predecessor belongs to another workgroup
      const int32_t pc = A.chrom[i0 - 1];
      p[0] = ((uint32_t)pc < A.nnames ? (int64_t)map[pc] << BG_KEY_SHIFT : 0) | (A.start[i0 - 1] & BG_COORD_MASK);
      p[1] = A.end[i0 - 1];
    }
#pragma unroll
    for (int j = 0; j < BG_COL_ROWS; ++j) {
      if (i0 + j < A.n) uns |= k[j] < p[0] || (k[j] == p[0] && e[j] < p[1]);
      p[0] = k[j], p[1] = e[j];
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
  __shared__ uint32_t smap[LDSMAP ? BG_COL_LDS_NAMES : 1];
  const uint32_t* map = col_rank_map<LDSMAP>(smap, A.rank, A.nnames);
  const uint64_t nchunks = (A.n + BG_COL_CHUNK - 1) / BG_COL_CHUNK;
  for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const uint64_t i0 = ch * BG_COL_CHUNK + (uint64_t)threadIdx.x * BG_COL_ROWS;
    int32_t cg[BG_COL_ROWS];
    int64_t s[BG_COL_ROWS], e[BG_COL_ROWS];
    uint64_t k[BG_COL_ROWS];
    uint32_t row[BG_COL_ROWS];
    col_load4(A.chrom, i0, A.n, cg);
    col_load4(A.start, i0, A.n, s);
    col_load4(A.end, i0, A.n, e);
#pragma unroll
    for (int j = 0; j < BG_COL_ROWS; ++j) {
      row[j] = (uint32_t)i0 + j;
      k[j] = (uint64_t)(e[j] - s[j]);
      if (packed) {
        const uint64_t r = (uint32_t)cg[j] < A.nnames ? map[cg[j]] : 0;
        k[j] |= ((uint64_t)s[j] << sh_start) | (sh_rank < 64 ? r << sh_rank : 0);
      }
    }
    col_store4(key, i0, A.n, k);
    col_store4(val, i0, A.n, row);
  }
}

// Round-1 keys: rank << bs | start of the row that round 0 left at each position
template <bool LDSMAP>
__global__ void __launch_bounds__(BG_NT) k_sc_key2(ScCols A, int bs, const uint32_t* __restrict__ val,
                                                   uint64_t* __restrict__ key) {
  __shared__ uint32_t smap[LDSMAP ? BG_COL_LDS_NAMES : 1];
  const uint32_t* map = col_rank_map<LDSMAP>(smap, A.rank, A.nnames);
  const uint64_t nchunks = (A.n + BG_COL_CHUNK - 1) / BG_COL_CHUNK;
  for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const uint64_t i0 = ch * BG_COL_CHUNK + (uint64_t)threadIdx.x * BG_COL_ROWS;
    uint32_t p[BG_COL_ROWS];
    uint64_t k[BG_COL_ROWS];
    col_load4(val, i0, A.n, p);
#pragma unroll
    for (int j = 0; j < BG_COL_ROWS; ++j) {
      k[j] = 0;
      if (i0 + j < A.n) {  // (p[j] < n: a row index the pack kernel wrote)
        const int32_t cg = A.chrom[p[j]];
        const uint64_t r = (uint32_t)cg < A.nnames ? map[cg] : 0;
        k[j] = (r << bs) | (uint64_t)A.start[p[j]];
      }
    }
    col_store4(key, i0, A.n, k);
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
  const uint64_t nchunks = (A.n + BG_COL_CHUNK - 1) / BG_COL_CHUNK;
  for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const uint64_t i0 = ch * BG_COL_CHUNK + (uint64_t)threadIdx.x * BG_COL_ROWS;
    int64_t p[BG_COL_ROWS];
    int32_t cg[BG_COL_ROWS];
    int64_t s[BG_COL_ROWS], e[BG_COL_ROWS];
    double sc[BG_COL_ROWS];
    if (IDENT) {
#pragma unroll
      for (int j = 0; j < BG_COL_ROWS; ++j) p[j] = (int64_t)(i0 + j);
      col_load4(A.chrom, i0, A.n, cg);
      col_load4(A.start, i0, A.n, s);
      col_load4(A.end, i0, A.n, e);
      if (O.score) col_load4(A.score, i0, A.n, sc);
    } else {
      uint32_t v[BG_COL_ROWS];
      col_load4(val, i0, A.n, v);
#pragma unroll
      for (int j = 0; j < BG_COL_ROWS; ++j) {
        const bool in = i0 + j < A.n;  // (v[j] < n: a row index the pack kernel wrote)
        p[j] = v[j];
        cg[j] = (in && O.chrom) ? A.chrom[v[j]] : 0;
        s[j] = (in && O.start) ? A.start[v[j]] : 0;
        e[j] = (in && O.end) ? A.end[v[j]] : 0;
        sc[j] = (in && O.score) ? A.score[v[j]] : 0.0;
      }
    }
    if (O.order) col_store4(O.order, i0, A.n, p);
    if (O.chrom) col_store4(O.chrom, i0, A.n, cg);
    if (O.start) col_store4(O.start, i0, A.n, s);
    if (O.end) col_store4(O.end, i0, A.n, e);
    if (O.score) col_store4(O.score, i0, A.n, sc);
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

static int sc_sort(bg_ctx* c, bg_columns I, const ScOut& O) {
  const uint64_t n = I.n;
  const uint32_t m1 = I.nnames ? I.nnames : 1;
  BgHold hold(c);
  bg_pin_reset(c);
  uint32_t* drank = hold.alloc<uint32_t>(m1);
  ScStatus* dst = hold.alloc<ScStatus>(1);
  uint32_t* hrank = (uint32_t*)bg_pin_take(c, 4ull * m1);
  ScStatus* hst = (ScStatus*)bg_pin_take(c, sizeof(ScStatus));
  if (!hold.ok() || !hrank || !hst) return BG_E_NOMEM;
  if (!O.score) I.score = nullptr;
  if (!I.on_device) {  // host arrays: staged in device temporaries
    const int rc = bg_cols_stage(c, hold, I, I.score != nullptr);
    if (rc) return rc;
  }
  ScCols A;
  A.chrom = I.chrom, A.start = I.start, A.end = I.end, A.score = I.score;
  A.n = n, A.nnames = I.nnames;
  hrank[0] = 0;
  sc_rank_table(I.names, I.nnames, hrank);
  A.rank = drank;
  hst->first_bad = ~0ULL;
  hst->max_start = hst->max_len = hst->unsorted = 0;
  BG_HIP(c, hipMemcpyAsync(drank, hrank, 4ull * m1, hipMemcpyHostToDevice, c->stream));
  BG_HIP(c, hipMemcpyAsync(dst, hst, sizeof(ScStatus), hipMemcpyHostToDevice, c->stream));
  const bool lds = I.nnames <= BG_COL_LDS_NAMES;
  uint64_t per_wg = 0;
  BG_COL_LAUNCH(c, "k_sc_key", k_sc_key, lds, bg_cols_span_grid(c, kern, n, &per_wg), A, dst, per_wg);
  // the call's one host round trip (the device read the status image above first: stream order)
  BG_HIP(c, hipMemcpyAsync(hst, dst, sizeof(ScStatus), hipMemcpyDeviceToHost, c->stream));
  BG_HIP(c, hipStreamSynchronize(c->stream));
  if (hst->first_bad != ~0ULL) {
    const ColRowError err = bg_cols_row_error((int)(hst->first_bad & 0xff));
    char msg[192];
    snprintf(msg, sizeof(msg), "sort_columns: row %llu: %s", (unsigned long long)(hst->first_bad >> 8), err.what);
    return bg_fail(c, err.rc, msg);
  }
  uint32_t* val = nullptr;
  if (n >= 2 && hst->unsorted) {
    const bg_sort_plan P = bg_sort_columns_plan(n, I.nnames, hst->max_start, hst->max_len);
    uint64_t* key = hold.alloc<uint64_t>(n);
    val = hold.alloc<uint32_t>(n);
    if (!hold.ok()) return BG_E_NOMEM;
    BG_COL_LAUNCH(c, "k_sc_pack", k_sc_pack, lds, bg_cols_stride_grid(c, kern, n), A, P.packed, P.bs + P.bl, P.bl,
                  key, val);
    int rc = bg_sort_u64_bits(c, key, val, n, P.bits[0]);
    if (rc) return rc;
    if (!P.packed) {
      BG_COL_LAUNCH(c, "k_sc_key2", k_sc_key2, lds, bg_cols_stride_grid(c, kern, n), A, P.bs, (const uint32_t*)val,
                    key);
      if ((rc = bg_sort_u64_bits(c, key, val, n, P.bits[1]))) return rc;
    }
    hold.drop(key);
  }
  if (O.order || O.chrom || O.start || O.end || O.score)
    BG_COL_LAUNCH(c, "k_sc_gather", k_sc_gather, !val, bg_cols_stride_grid(c, kern, n), A, (const uint32_t*)val, O);
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
