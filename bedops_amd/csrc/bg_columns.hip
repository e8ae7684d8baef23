// bg_columns.hip — the columnar seam of libbedgpu: intervals in and results out as numeric
// device columns instead of BED text (include/bedgpu.h, "columnar interface").
//
// In:  bg_load_columns keys (chrom index, start, end) rows into the same ks / ke columns the
//      text loaders produce (bg_internal.h), in one pass that also applies their row checks
//      (emit_row and the sort checks of bg_load.hip): k_cols_key, built from the pieces it
//      shares with bg_sort_columns' kernels (bg_colkern.h, whose host helpers are defined here).
// Out: bg_set_export_rows / bg_result_export_* unkey tables and results into caller-owned
//      device columns.
// A column-loaded table has no text and no remainders (bg_table::cols): whatever prints or
// compares row text refuses it on the host (bg_no_text).
#include <math.h>
#include <stdlib.h>

#include "bg_colkern.h"

// the names tests/test_gpu_columns.py reads its shapes by: the shared values, nothing else
#define CK_ROWS 4
#define CK_LDS_NAMES 2048
static_assert(CK_ROWS == BG_COL_ROWS && CK_LDS_NAMES == BG_COL_LDS_NAMES, "bg_colkern.h holds the values");

struct ColsArgs {
  const int32_t* chrom;
  const int64_t* start;
  const int64_t* end;
  const double* score;  // null: no scores
  double* score_out;    // the table's own score column
  uint64_t n;
  const uint32_t* remap;  // local chromosome index -> rank in the set's dictionary
  uint32_t nnames;
  int64_t* ks;
  int64_t* ke;
  unsigned long long* runrow;  // local chromosome -> first row of its run (~0: no row)
  bg_dstatus* st;
  uint64_t per_wg;  // consecutive chunks of BG_COL_CHUNK rows per workgroup
};

// One pass over the columns: 20 B read and 16 B written per row (28 and 24 with scores, which
// are checked and copied to the table's column here: the caller's arrays may belong to another
// HIP runtime in the process, whose pointers only kernels may touch). A workgroup keys `per_wg`
// consecutive chunks, each lane BG_COL_ROWS consecutive rows (col_load4 / col_store4). The key
// before a lane's first row: ColCarry; only the first row of a workgroup's span reloads its
// predecessor from memory.
template <bool LDSMAP>
__global__ void __launch_bounds__(BG_NT) k_cols_key(ColsArgs A) {
  __shared__ uint32_t smap[LDSMAP ? BG_COL_LDS_NAMES : 1];
  __shared__ ColCarry<1>::Slots wlast;
  const uint32_t* map = col_rank_map<LDSMAP>(smap, A.remap, A.nnames);
  const int lane = bg_lane();
  const uint64_t nchunks = (A.n + BG_COL_CHUNK - 1) / BG_COL_CHUNK;
  const uint64_t c0 = (uint64_t)blockIdx.x * A.per_wg;
  const uint64_t c1 = min(c0 + A.per_wg, nchunks);
  int64_t mlen = 0;
  bool zero = false, nonint = false;
  ColCarry<1> carry;
  for (uint64_t ch = c0; ch < c1; ++ch) {
    const uint64_t i0 = ch * BG_COL_CHUNK + (uint64_t)threadIdx.x * BG_COL_ROWS;
    int32_t cg[BG_COL_ROWS];
    int64_t s[BG_COL_ROWS], e[BG_COL_ROWS];
    double sc[BG_COL_ROWS];
    col_load4(A.chrom, i0, A.n, cg);
    col_load4(A.start, i0, A.n, s);
    col_load4(A.end, i0, A.n, e);
    if (A.score) col_load4(A.score, i0, A.n, sc);
    int64_t ks[BG_COL_ROWS], ke[BG_COL_ROWS];
#pragma unroll
    for (int j = 0; j < BG_COL_ROWS; ++j) {
      const uint64_t i = i0 + j;
      const bool badc = (uint32_t)cg[j] >= A.nnames;
      const int64_t g = badc ? 0 : (int64_t)map[cg[j]] << BG_KEY_SHIFT;
      ks[j] = g | (s[j] & BG_COORD_MASK);
      ke[j] = g | (e[j] & BG_COORD_MASK);
      if (i < A.n) {
        if (badc) bg_report(A.st, i, ERR_COLS_CHROM);
        if (s[j] < 0 || e[j] < 0 || (uint64_t)e[j] > BG_KEY_COORD_MAX || s[j] > e[j]) {
          bg_report(A.st, i, ERR_RANGE);
        } else {
          zero |= s[j] == e[j];
          mlen = max(mlen, e[j] - s[j]);
        }
        if (A.score) {
          if (!isfinite(sc[j])) bg_report(A.st, i, ERR_SCORE);
          nonint |= sc[j] != trunc(sc[j]) || fabs(sc[j]) >= 9007199254740992.0;
        }
      }
    }
    // the key before this lane's first row (ColCarry; LLONG_MIN for row 0, whose rank then
    // differs from every row's)
    int64_t pk[1];
    if (!carry.step(wlast, {ks[BG_COL_ROWS - 1]}, pk) && i0 > 0) {
      // the span's first row: its predecessor was keyed by another workgroup
      const int32_t pc = A.chrom[i0 - 1];
      pk[0] = (uint32_t)pc < A.nnames ? ((int64_t)map[pc] << BG_KEY_SHIFT) | (A.start[i0 - 1] & BG_COORD_MASK) : 0;
    }
    int64_t pred = pk[0];
#pragma unroll
    for (int j = 0; j < BG_COL_ROWS; ++j) {
      const uint64_t i = i0 + j;
      if (i < A.n) {
        // (a row with a bad chrom index has no rank: it is reported as that, not as unsorted)
        if ((uint32_t)cg[j] < A.nnames) {
          if (ks[j] < pred) bg_report(A.st, i, ERR_UNSORTED);
          if ((ks[j] >> BG_KEY_SHIFT) != (pred >> BG_KEY_SHIFT)) atomicMin(&A.runrow[cg[j]], (unsigned long long)i);
        }
      }
      pred = ks[j];
    }
    col_store4(A.ks, i0, A.n, ks);
    col_store4(A.ke, i0, A.n, ke);
    if (A.score) col_store4(A.score_out, i0, A.n, sc);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mlen = max(mlen, (int64_t)__shfl_xor(mlen, d, 64));
  const bool anyzero = __ballot(zero) != 0, anynonint = __ballot(nonint) != 0;
  if (lane == 0) {
    if (mlen > *(volatile long long*)&A.st->maxlen) atomicMax(&A.st->maxlen, (long long)mlen);
    const unsigned long long f = (anynonint ? 1ULL : 0ULL) | (anyzero ? 2ULL : 0ULL);
    if (f) atomicOr(&A.st->flags, f);
  }
}

// (kernels, not hipMemcpy, write the caller's buffers: see k_cols_key)
__global__ void __launch_bounds__(BG_NT) k_cols_copy_u64(const uint64_t* __restrict__ in, uint64_t n,
                                                         int64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * BG_NT + threadIdx.x;
  if (i < n) out[i] = (int64_t)in[i];
}
// keys -> (dictionary rank, coordinate) columns (+ scores); a null output skips that column
__global__ void __launch_bounds__(BG_NT) k_cols_unkey(const int64_t* __restrict__ S, const int64_t* __restrict__ E,
                                                      uint64_t n, int32_t* __restrict__ chrom,
                                                      int64_t* __restrict__ start, int64_t* __restrict__ end,
                                                      const double* __restrict__ SC, double* __restrict__ score) {
  const uint64_t i = (uint64_t)blockIdx.x * BG_NT + threadIdx.x;
  if (i >= n) return;
  if (score) score[i] = SC[i];
  const int64_t s = S[i];
  if (chrom) chrom[i] = (int32_t)(s >> BG_KEY_SHIFT);
  if (start) start[i] = s & BG_COORD_MASK;
  if (end) end[i] = E[i] & BG_COORD_MASK;
}

// the double render() of bg_format.hip prints for one of the plain numeric operations
__global__ void __launch_bounds__(BG_NT) k_map_export(int op, const int32_t* __restrict__ cnt,
                                                      const int64_t* __restrict__ isum,
                                                      const double* __restrict__ dsum,
                                                      const double* __restrict__ vmin,
                                                      const double* __restrict__ vmax, uint64_t n,
                                                      double* __restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * BG_NT + threadIdx.x;
  if (k >= n) return;
  const int32_t c = cnt[k];
  double v;
  if (op == BG_MAP_COUNT) v = (double)c;
  else if (op == BG_MAP_INDICATOR) v = c > 0 ? 1.0 : 0.0;
  else if (c <= 0) v = __builtin_nan("");
  else if (op == BG_MAP_MEAN) v = (dsum ? dsum[k] : (double)isum[k]) / (double)c;
  else if (op == BG_MAP_SUM) v = dsum ? dsum[k] : (double)isum[k];
  else v = (op == BG_MAP_MIN) ? vmin[k] : vmax[k];
  out[k] = v;
}

int bg_no_text(bg_ctx* c, const bg_set* set, int file, const char* what) {
  if (!set->t[file]->cols) return 0;
  return bg_fail(c, BG_E_ARG, std::string(what) + ": input " + std::to_string(file + 1) +
                                  " was loaded from columns and has no text");
}

// rows of one start whose ends do not strictly increase: two rows equal in (start, end), or
// ends out of order (the loader orders rows by start only, so equal rows need not be neighbours)
__global__ void __launch_bounds__(BG_NT) k_cols_end_order(const int64_t* __restrict__ S, const int64_t* __restrict__ E,
                                                          uint64_t n, unsigned int* __restrict__ any) {
  const uint64_t m = (uint64_t)blockIdx.x * BG_NT + threadIdx.x + 1;
  if (m < n && S[m] == S[m - 1] && E[m] <= E[m - 1]) atomicOr(any, 1u);
}

int bg_cols_end_ties(bg_ctx* c, const bg_table* M, bool* any) {
  *any = false;
  if (M->n < 2) return 0;
  BgHold hold(c);
  unsigned int* d = hold.alloc<unsigned int>(1);
  unsigned int* h = (unsigned int*)c->hstat;  // pinned; bg_map refills it after its kernels
  if (!hold.ok()) return BG_E_NOMEM;
  BG_HIP(c, hipMemsetAsync(d, 0, 4, c->stream));
  BG_LAUNCH(c, "k_cols_end_order", k_cols_end_order, dim3(bg_blocks(M->n - 1, BG_NT)), dim3(BG_NT), M->ks, M->ke,
            M->n, d);
  BG_HIP(c, hipGetLastError());
  BG_HIP(c, hipMemcpyAsync(h, d, 4, hipMemcpyDeviceToHost, c->stream));
  BG_HIP(c, hipStreamSynchronize(c->stream));
  *any = *h != 0;
  return 0;
}

static bool name_less(const std::string& a, const std::string& b) { return strcmp(a.c_str(), b.c_str()) < 0; }

// everything the host can see before any launch (`rows`: host arrays are walked too; the sort
// finds a bad chrom index in its key pass on either kind of array, bg_sortcols.hip)
int bg_cols_check_args(bg_ctx* c, int n, const bg_columns* in, bool rows) {
  for (int i = 0; i < n; ++i) {
    const bg_columns& I = in[i];
    const std::string who = "input " + std::to_string(i + 1) + ": ";
    if (I.kind == BG_BED3_REST || I.kind == BG_BED5_REST)
      return bg_fail(c, BG_E_ARG, who + "columns carry no remainder (BG_BED3, BG_BED3_SET or BG_BED5)");
    if (I.kind != BG_BED3 && I.kind != BG_BED3_SET && I.kind != BG_BED5)
      return bg_fail(c, BG_E_ARG, who + "unknown kind");
    if ((I.kind == BG_BED5) != (I.score != nullptr))
      return bg_fail(c, BG_E_ARG, who + "a score column goes with BG_BED5, and only with it");
    if (I.n && (!I.chrom || !I.start || !I.end)) return bg_fail(c, BG_E_ARG, who + "null column");
    if (I.nnames && !I.names) return bg_fail(c, BG_E_ARG, who + "null names");
    if (I.n >= (1ULL << BG_KEY_SHIFT)) return bg_fail(c, BG_E_UNSUPPORTED, who + "too many rows");
    std::vector<std::string> nm;
    for (uint32_t k = 0; k < I.nnames; ++k) {
      const char* p = I.names[k];
      if (!p || !*p) return bg_fail(c, BG_E_ARG, who + "empty chromosome name");
      const size_t len = strlen(p);
      if (strpbrk(p, " \t\n\v\f\r")) return bg_fail(c, BG_E_ARG, who + "whitespace in a chromosome name");
      if (len > BG_CHR_MAX) return bg_fail(c, BG_E_CHROM, who + "chromosome name longer than 127 characters");
      nm.emplace_back(p, len);
    }
    std::sort(nm.begin(), nm.end(), name_less);
    if (std::adjacent_find(nm.begin(), nm.end()) != nm.end())
      return bg_fail(c, BG_E_ARG, who + "duplicate chromosome name");
    if (I.on_device) {
      for (const void* p : {(const void*)I.chrom, (const void*)I.start, (const void*)I.end, (const void*)I.score})
        if (I.n && ((uintptr_t)p & 15)) return bg_fail(c, BG_E_ARG, who + "device columns must be 16-byte aligned");
      continue;
    }
    for (uint64_t r = 0; rows && r < I.n; ++r) {
      if ((uint32_t)I.chrom[r] >= I.nnames)
        return bg_fail(c, BG_E_ARG, who + "row " + std::to_string(r) + ": chrom index outside names");
      if (I.score && !isfinite(I.score[r]))
        return bg_fail(c, BG_E_UNSUPPORTED, who + "row " + std::to_string(r) + ": score is not finite");
    }
  }
  return 0;
}

ColRowError bg_cols_row_error(int code) {
  switch (code) {
    case ERR_RANGE: return {"coordinate out of range (negative, end < start or >= 2^40)", BG_E_RANGE};
    case ERR_UNSORTED: return {"rows are not sorted (chromosome names in strcmp order, then start)", BG_E_UNSORTED};
    case ERR_SCORE: return {"score is not finite", BG_E_UNSUPPORTED};
    case ERR_COLS_CHROM: return {"chrom index outside names", BG_E_ARG};
  }
  return {"", BG_E_INTERNAL};
}

static int cols_report(bg_ctx* c, int file, const bg_dstatus& h) {
  if (h.first_bad == ~0ULL) return 0;
  const ColRowError err = bg_cols_row_error((int)(h.first_bad & 0xff));
  char msg[256];
  snprintf(msg, sizeof(msg), "input %d, row %llu: %s", file + 1, (unsigned long long)(h.first_bad >> 8), err.what);
  return bg_fail(c, err.rc, msg);
}

// workgroups of k_cols_key: the resident grid, or fewer. BEDGPU_COLS_BLOCKS is a test hook
// (bedgpu.h): it caps the grid so that a workgroup runs several rounds on an
// input of a few thousand rows; read at every load so a test can set it between calls
uint64_t bg_cols_grid(bg_ctx* c, const void* kern) {
  uint64_t g = bg_resident_blocks(c, kern);
  const char* s = getenv("BEDGPU_COLS_BLOCKS");
  const long v = s ? atol(s) : 0;
  if (v > 0 && (uint64_t)v < g) g = (uint64_t)v;
  return g;
}

unsigned bg_cols_span_grid(bg_ctx* c, const void* kern, uint64_t n, uint64_t* per_wg) {
  const uint64_t nchunks = (n + BG_COL_CHUNK - 1) / BG_COL_CHUNK, g = bg_cols_grid(c, kern);
  *per_wg = (nchunks + g - 1) / g;
  return (unsigned)((nchunks + *per_wg - 1) / *per_wg);
}

unsigned bg_cols_stride_grid(bg_ctx* c, const void* kern, uint64_t n) {
  return (unsigned)std::min<uint64_t>((n + BG_COL_CHUNK - 1) / BG_COL_CHUNK, bg_cols_grid(c, kern));
}

int bg_cols_stage(bg_ctx* c, BgHold& hold, bg_columns& I, bool score) {
  int32_t* dc = hold.alloc<int32_t>(I.n);
  int64_t* ds = hold.alloc<int64_t>(I.n);
  int64_t* de = hold.alloc<int64_t>(I.n);
  double* dv = score ? hold.alloc<double>(I.n) : nullptr;
  if (!hold.ok()) return BG_E_NOMEM;
  BG_HIP(c, hipMemcpyAsync(dc, I.chrom, 4 * I.n, hipMemcpyHostToDevice, c->stream));
  BG_HIP(c, hipMemcpyAsync(ds, I.start, 8 * I.n, hipMemcpyHostToDevice, c->stream));
  BG_HIP(c, hipMemcpyAsync(de, I.end, 8 * I.n, hipMemcpyHostToDevice, c->stream));
  if (dv) BG_HIP(c, hipMemcpyAsync(dv, I.score, 8 * I.n, hipMemcpyHostToDevice, c->stream));
  I.chrom = dc, I.start = ds, I.end = de;
  if (dv) I.score = dv;
  return 0;
}

static int cols_load(bg_ctx* c, int n, const bg_columns* in, bg_set** out) {
  std::vector<Ivl> comps((size_t)n);  // BG_BED3_SET inputs' components until their tables take them
  bg_set* s = new bg_set();
  s->ctx = c;
  BgHold hold(c);
  hold.own(s, comps);
  // the dictionary: strcmp-sorted union of every input's names
  std::vector<std::string> all;
  for (int i = 0; i < n; ++i)
    for (uint32_t k = 0; k < in[i].nnames; ++k) all.emplace_back(in[i].names[k]);
  std::sort(all.begin(), all.end(), name_less);
  all.erase(std::unique(all.begin(), all.end()), all.end());
  if (all.size() >= (1u << 22)) return bg_fail(c, BG_E_UNSUPPORTED, "too many chromosomes");
  s->names = all;
  bg_pin_reset(c);
  {  // one device block: names (16-B padded) | offsets | lengths (as build_dictionary, bg_load.hip)
    std::string packed;
    std::vector<uint32_t> off(all.size() + 1, 0), len(all.size() + 1, 0);
    for (size_t k = 0; k < all.size(); ++k) {
      off[k] = (uint32_t)packed.size();
      len[k] = (uint32_t)all[k].size();
      s->max_name_len = std::max<uint32_t>(s->max_name_len, len[k]);
      packed += all[k];
    }
    const size_t nbn = (packed.size() + 16) & ~(size_t)15, nbo = 4 * off.size(), blk = nbn + 2 * nbo;
    s->d_names = hold.raw<char>(blk);
    char* h = (char*)bg_pin_take(c, blk);
    if (!hold.ok() || !h) return BG_E_NOMEM;
    s->d_name_off = (uint32_t*)(s->d_names + nbn);
    s->d_name_len = (uint32_t*)(s->d_names + nbn + nbo);
    memset(h, 0, blk);
    memcpy(h, packed.data(), packed.size());
    memcpy(h + nbn, off.data(), nbo);
    memcpy(h + nbn + nbo, len.data(), nbo);
    BG_HIP(c, hipMemcpyAsync(s->d_names, h, blk, hipMemcpyHostToDevice, c->stream));
  }
  bg_dstatus* dst = hold.alloc<bg_dstatus>((size_t)n);
  bg_dstatus* hst = (bg_dstatus*)bg_pin_take(c, sizeof(bg_dstatus) * n);
  if (!hold.ok() || !hst) return BG_E_NOMEM;
  for (int i = 0; i < n; ++i) {
    memset(&hst[i], 0, sizeof(bg_dstatus));
    hst[i].first_bad = ~0ULL;
  }
  BG_HIP(c, hipMemcpyAsync(dst, hst, sizeof(bg_dstatus) * n, hipMemcpyHostToDevice, c->stream));
  // (the device reads that image before a later copy back overwrites it: stream order)
  std::vector<unsigned long long*> drun((size_t)n, nullptr), hrun((size_t)n, nullptr);
  std::vector<int64_t*> sks((size_t)n, nullptr), ske((size_t)n, nullptr);  // set inputs' keyed rows
  for (int i = 0; i < n; ++i) {
    bg_columns I = in[i];
    bg_table* T = new bg_table();
    s->t.push_back(T);
    T->kind = I.kind;
    T->cols = true;
    T->n = I.n;
    T->is_set = I.kind == BG_BED3_SET;
    const uint64_t n1 = I.n ? I.n : 1, m1 = I.nnames ? I.nnames : 1;
    ColsArgs A;
    if (I.score) T->score = hold.raw<double>(n1);
    if (!I.on_device && I.n) {  // host arrays: staged in device temporaries (the scores in the table's column)
      const int rc = bg_cols_stage(c, hold, I, false);
      if (rc) return rc;
    }
    if (!hold.ok()) return BG_E_NOMEM;
    A.chrom = I.chrom, A.start = I.start, A.end = I.end, A.score = I.score;
    A.score_out = T->score;
    if (I.score && I.n && !I.on_device) {  // (in place: the kernel's copy onto itself changes nothing)
      BG_HIP(c, hipMemcpyAsync(T->score, I.score, 8 * I.n, hipMemcpyHostToDevice, c->stream));
      A.score = T->score;
    }
    // the keyed rows: the table's columns, or temporaries of a set input
    int64_t* ks = T->is_set ? hold.alloc<int64_t>(n1) : (T->ks = hold.raw<int64_t>(n1));
    int64_t* ke = T->is_set ? hold.alloc<int64_t>(n1) : (T->ke = hold.raw<int64_t>(n1));
    uint32_t* dmap = hold.alloc<uint32_t>(m1);
    drun[i] = hold.alloc<unsigned long long>(m1);
    uint32_t* hmap = (uint32_t*)bg_pin_take(c, 4 * m1);
    hrun[i] = (unsigned long long*)bg_pin_take(c, 8 * m1);
    if (!hold.ok() || !hmap || !hrun[i]) return BG_E_NOMEM;
    for (uint32_t k = 0; k < I.nnames; ++k)
      hmap[k] = (uint32_t)(std::lower_bound(all.begin(), all.end(), std::string(I.names[k]), name_less) - all.begin());
    BG_HIP(c, hipMemcpyAsync(dmap, hmap, 4 * m1, hipMemcpyHostToDevice, c->stream));
    BG_HIP(c, hipMemsetAsync(drun[i], 0xff, 8 * m1, c->stream));
    if (I.n) {
      A.n = I.n;
      A.remap = dmap;
      A.nnames = I.nnames;
      A.ks = ks, A.ke = ke;
      A.runrow = drun[i];
      A.st = dst + i;
      BG_COL_LAUNCH(c, "k_cols_key", k_cols_key, I.nnames <= BG_COL_LDS_NAMES,
                    bg_cols_span_grid(c, kern, I.n, &A.per_wg), A);
    }
    if (T->is_set) sks[i] = ks, ske[i] = ke;
  }
  // one round trip for every input's status and runs; only checked rows are merged below
  for (int i = 0; i < n; ++i)
    BG_HIP(c, hipMemcpyAsync(hrun[i], drun[i], 8ull * (in[i].nnames ? in[i].nnames : 1), hipMemcpyDeviceToHost,
                             c->stream));
  BG_HIP(c, hipMemcpyAsync(hst, dst, sizeof(bg_dstatus) * n, hipMemcpyDeviceToHost, c->stream));
  BG_HIP(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; ++i) {
    const int rc = cols_report(c, i, hst[i]);
    if (rc) return rc;
  }
  // BG_BED3_SET: the keyed rows merged by bg_components, then released
  for (int i = 0; i < n; ++i) {
    bg_table* T = s->t[i];
    if (!T->is_set) continue;
    Ivl rows;
    rows.s = sks[i], rows.e = ske[i], rows.n = T->n;
    const int rc = bg_components(c, rows, comps[i]);
    if (rc) return rc;
    T->cs = comps[i].s;
    T->ce = comps[i].e;
    T->nc = comps[i].n;
    comps[i] = Ivl();
    hold.drop(sks[i], ske[i]);
  }
  for (int i = 0; i < n; ++i) {
    bg_table* T = s->t[i];
    const bg_dstatus& h = hst[i];
    T->has_zero_len = (h.flags & 2ULL) != 0;
    if (T->score) T->score_int = (h.flags & 1ULL) == 0;
    // chromosome runs in row order (a checked input has one run per chromosome it uses)
    std::vector<std::pair<uint64_t, uint32_t>> runs;
    for (uint32_t k = 0; k < in[i].nnames; ++k)
      if (hrun[i][k] != ~0ULL) runs.push_back({(uint64_t)hrun[i][k], k});
    std::sort(runs.begin(), runs.end());
    for (auto& r : runs) T->run_name.emplace_back(in[i].names[r.second]);
    if (T->is_set) {  // as a text-loaded set table: one span over the rows that were read
      T->run_row0.assign({0, T->n});
      continue;
    }
    T->maxlen = h.maxlen;
    for (auto& r : runs) T->run_row0.push_back(r.first);
    T->run_row0.push_back(T->n);
    if (T->n == 0) T->run_row0.assign(1, 0);
  }
  bg_mark(c, "columns");
  *out = s;
  s = nullptr;  // the caller's from here
  return 0;
}

extern "C" int bg_load_columns(bg_ctx* c, int n, const bg_columns* in, bg_set** out) {
  if (!c || n <= 0 || !in || !out) return BG_E_ARG;
  *out = nullptr;
  int rc = bg_cols_check_args(c, n, in, true);
  if (rc) return rc;
  rc = cols_load(c, n, in, out);
  if (rc) (void)hipStreamSynchronize(c->stream);  // queued copies may still read the caller's arrays
  return rc;
}

static int cols_unkey(bg_ctx* c, const int64_t* S, const int64_t* E, uint64_t n, int32_t* chrom, int64_t* start,
                      int64_t* end, const double* SC = nullptr, double* score = nullptr) {
  if (!n || (!chrom && !start && !end && !score)) return 0;
  BG_LAUNCH(c, "k_cols_unkey", k_cols_unkey, dim3(bg_blocks(n, BG_NT)), dim3(BG_NT), S, E, n, chrom, start, end, SC,
            score);
  BG_HIP(c, hipGetLastError());
  return 0;
}

extern "C" int bg_set_export_rows(bg_ctx* c, const bg_set* set, int file, int32_t* chrom, int64_t* start,
                                  int64_t* end, double* score) {
  if (!c || !set || file < 0 || file >= (int)set->t.size()) return BG_E_ARG;
  const bg_table* T = set->t[file];
  if (T->is_set)
    return bg_fail(c, BG_E_ARG, "export: input " + std::to_string(file + 1) + " was loaded as BG_BED3_SET (no rows kept)");
  if (score && !T->score) return bg_fail(c, BG_E_ARG, "export: input " + std::to_string(file + 1) + " has no scores");
  return cols_unkey(c, T->ks, T->ke, T->n, chrom, start, end, T->score, score);
}

extern "C" int bg_result_kind(const bg_result* r, int* kind, int* table) {
  if (!r || !kind) return BG_E_ARG;
  int t = -1;
  switch (r->kind) {
    case RES_IVL: *kind = BG_RESKIND_INTERVALS; break;
    case RES_ROWS: *kind = BG_RESKIND_ROWS; t = r->tab; break;
    case RES_MAP: *kind = BG_RESKIND_MAP; t = r->tab; break;
    case RES_CLOSEST:  // (bg_closest's own results stay "text only", as before bg_closest_rows)
      if (r->crows) { *kind = BG_RESKIND_CLOSEST; t = r->tab; }
      else *kind = BG_RESKIND_OTHER;
      break;
    default: *kind = BG_RESKIND_OTHER; break;
  }
  if (table) *table = t;
  return 0;
}

extern "C" int bg_result_export_intervals(bg_ctx* c, bg_result* r, int32_t* chrom, int64_t* start, int64_t* end) {
  if (!c || !r) return BG_E_ARG;
  if (r->kind != RES_IVL) return bg_fail(c, BG_E_ARG, "export: not an interval result");
  // a segmented result: its count fetched and its pieces made contiguous (text it already
  // has stays; the formatter reads either layout)
  int rc = bg_result_compact(c, r);
  if (rc) return rc;
  return cols_unkey(c, r->s, r->e, r->n, chrom, start, end);
}

extern "C" int bg_result_export_rows(bg_ctx* c, bg_result* r, int64_t* rows) {
  if (!c || !r) return BG_E_ARG;
  if (r->kind != RES_ROWS) return bg_fail(c, BG_E_ARG, "export: not a row result (element-of / not-element-of)");
  if (!rows || !r->n) return 0;
  BG_LAUNCH(c, "k_cols_copy_u64", k_cols_copy_u64, dim3(bg_blocks(r->n, BG_NT)), dim3(BG_NT),
            (const uint64_t*)r->rows, r->n, rows);
  BG_HIP(c, hipGetLastError());
  return 0;
}

extern "C" int bg_result_export_map(bg_ctx* c, bg_result* r, int op_index, double* values) {
  if (!c || !r || !values) return BG_E_ARG;
  if (r->kind != RES_MAP) return bg_fail(c, BG_E_ARG, "export: not a bedmap result");
  if (op_index < 0 || op_index >= r->mopts.n_ops) return bg_fail(c, BG_E_ARG, "export: no such operation in the result");
  if (r->mopts.skip_unmapped)
    return bg_fail(c, BG_E_ARG, "export: the result was built with --skip-unmapped (filter by the count instead)");
  const int op = r->mopts.ops[op_index];
  switch (op) {
    case BG_MAP_COUNT: case BG_MAP_INDICATOR: case BG_MAP_SUM: case BG_MAP_MEAN: case BG_MAP_MIN: case BG_MAP_MAX: break;
    default: return bg_fail(c, BG_E_UNSUPPORTED, "export: count, indicator, sum, mean, min and max only");
  }
  if (!r->n) return 0;
  BG_LAUNCH(c, "k_map_export", k_map_export, dim3(bg_blocks(r->n, BG_NT)), dim3(BG_NT), op, (const int32_t*)r->cnt,
            (const int64_t*)r->isum, (const double*)r->dsum, (const double*)r->vmin, (const double*)r->vmax, r->n,
            values);
  BG_HIP(c, hipGetLastError());
  return 0;
}
