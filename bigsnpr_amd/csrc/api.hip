// api.hip — the operator over a sub-view, the code counts and their caches, and the one-shot .Call replacements declared
// in include/bigsnpr_hip.h.  The process-level plumbing is runtime.hip, the handle as an object handle.hip.
#include <cxxabi.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>

#include "bsn_internal.hpp"

namespace bsn {

// a NULL index list means the first `len` rows / columns, everywhere in this ABI
static std::vector<int32_t> to_i32(const int64_t *ind, int64_t len, int64_t limit, const char *what) {
  std::vector<int32_t> v((size_t)len);
  if (!ind) {
    if (len > limit)
      fail("Tested %lld < %lld. Subscript out of bounds (%s).", (long long)(len - 1), (long long)limit, what);
    for (int64_t i = 0; i < len; i++) v[(size_t)i] = (int32_t)i;
    return v;
  }
  for (int64_t i = 0; i < len; i++) {
    if (ind[i] < 0 || ind[i] >= limit)
      // bigstatsr vec_int_to_size(): "Tested %s < %s. Subscript out of bounds."
      fail("Tested %lld < %lld. Subscript out of bounds (%s).", (long long)ind[i], (long long)limit,
           what);
    v[(size_t)i] = (int32_t)ind[i];
  }
  return v;
}
// a checked list on the device, uploaded through the handle `on` (its staging buffers, its stream)
static void upload_list(bsn_bed *on, DevBuf<int32_t> &d, const std::vector<int32_t> &v) {
  copy_h2d(on, d.ensure(v.size()), v.data(), v.size() * 4);
}

__global__ void k_fill_f64(double *p, int64_t n, double v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

void fill_op(bsn_op *op, bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
             int64_t m, const double *center, const double *scale, bool defer_scale, bool allow_streamed) {
  if (n <= 0 || m <= 0) fail("'ind.row' and 'ind.col' can't be empty.");
  if (bed->n >= (int64_t)1 << 31 || bed->m >= (int64_t)1 << 31) fail("dimension too large");
  if (!allow_streamed) require_resident(bed, "this function");
  BSN_HIP(hipSetDevice(bed->device));
  op->bed = bed;
  op->n = n;
  op->m = m;
  // rows (NULL: the first n)
  if (!ind_row && n > bed->n)
    fail("Tested %lld < %lld. Subscript out of bounds (ind.row).", (long long)(n - 1), (long long)bed->n);
  bool ident = (n == bed->n);
  if (ind_row) {
    for (int64_t i = 0; ident && i < n; i++) ident = (ind_row[i] == i);
  }
  op->rows_identity = ident;
  if (!ident) upload_list(bed, op->d_rows, to_i32(ind_row, n, bed->n, "ind.row"));
  // cols
  bool contig = true;
  int64_t c0 = ind_col ? ind_col[0] : 0;
  if (ind_col)
    for (int64_t j = 0; contig && j < m; j++) contig = (ind_col[j] == c0 + j);
  if (c0 < 0 || c0 >= bed->m || (contig && c0 + m > bed->m))
    fail("Tested %lld < %lld. Subscript out of bounds (ind.col).", (long long)(c0 + m - 1),
         (long long)bed->m);
  op->cols_contig = contig;
  op->col0 = contig ? c0 : 0;
  if (!contig) {
    auto c = to_i32(ind_col, m, bed->m, "ind.col");
    c.resize((size_t)bsn::round_up(m, 64), c[0]);
    upload_list(bed, op->d_cols, c);
  }
  // missing-value knowledge (BSN_FORCE_NA_PLANE=1 keeps the general kernels, for A/B tests)
  op->no_na = false;
  if ((int64_t)bed->na_cnt.size() == bed->m && !getenv("BSN_FORCE_NA_PLANE")) {
    bool all0 = true;
    for (int64_t j = 0; all0 && j < m; j++) all0 = bed->na_cnt[(size_t)(ind_col ? ind_col[j] : j)] == 0;
    op->no_na = all0;
  }
  if (defer_scale) {  // written on the device by the first crossproduct pass (matvec.hip)
    op->d_center.ensure((size_t)m);
    op->d_scale.ensure((size_t)m);
    return;
  }
  // centre / scale (defaults 0 / 1, R/bed-mult-vec.R:23-24)
  op->d_center.ensure((size_t)m);
  op->d_scale.ensure((size_t)m);
  if (center) copy_h2d(bed, op->d_center.p, center, (size_t)m * 8);
  else BSN_HIP(hipMemsetAsync(op->d_center.p, 0, (size_t)m * 8, bed->stream));
  if (scale) {
    copy_h2d(bed, op->d_scale.p, scale, (size_t)m * 8);
  } else {
    hipLaunchKernelGGL(k_fill_f64, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, bed->stream, op->d_scale.p, m, 1.0);
    BSN_HIP(hipGetLastError());
  }
}

// counts of the codes 0, 1, 2, missing of every selected variant over the selected rows, 4 x m int32 on
// the device
void counts_device(bsn_op *op, const int64_t *ind_row, int64_t n, int32_t *d_counts) {
  bsn_bed *bed = op->bed;
  if (op->rows_identity) {
    counts_all_rows(bed, op->cols(), op->col0, op->m, d_counts);
  } else {
    std::vector<double> w((size_t)bed->n, 0.0);
    for (int64_t i = 0; i < n; i++) w[(size_t)(ind_row ? ind_row[i] : i)] += 1.0;
    DevBuf<double> d_w;
    copy_h2d(bed, d_w.ensure((size_t)bed->n), w.data(), (size_t)bed->n * 8);
    counts_weighted(op, d_w.p, n, d_counts);
    BSN_HIP(hipStreamSynchronize(bed->stream));  // d_w is released on return
  }
}

// the same into a host 4 x m int32 array, from a resident image
static void counts_resident(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                            int64_t m, int32_t *res) {
  // the counts as an earlier call left them (BSN_NO_COUNTS_CACHE=1: always count).  All samples in file order: the
  // handle's device-resident counts, which the solves feed and read too (bsn_bed::stats_cache); any other row
  // selection: the host copy of the last one
  auto &cc = bed->counts_cache;
  const bool use_cache = n > 0 && m > 0 && !getenv("BSN_NO_COUNTS_CACHE");
  bool rows_all = n == bed->n;
  for (int64_t i = 0; rows_all && ind_row && i < n; i++) rows_all = ind_row[i] == i;
  std::vector<int64_t> lead;         // (a NULL list with n < the handle's samples: the leading n)
  const int64_t *rows = ind_row;
  if (use_cache && !rows_all && !ind_row) {
    lead.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) lead[(size_t)i] = i;
    rows = lead.data();
  }
  const bool same_rows = use_cache && !rows_all && (int64_t)cc.cnt.size() == 4 * bed->m && (int64_t)cc.rows.size() == n &&
                         std::memcmp(cc.rows.data(), rows, (size_t)n * 8) == 0;
  if (same_rows) {
    bool known = true;
    for (int64_t j = 0; known && j < m; j++) {
      const int64_t c = ind_col ? ind_col[j] : j;
      known = c >= 0 && c < bed->m && cc.cnt[(size_t)4 * c] >= 0;
    }
    if (known) {
      for (int64_t j = 0; j < m; j++) std::memcpy(res + 4 * j, &cc.cnt[(size_t)4 * (ind_col ? ind_col[j] : j)], 16);
      return;
    }
  }
  bsn_op op;
  fill_op(&op, bed, ind_row, n, ind_col, m, nullptr, nullptr, true);
  DevBuf<int32_t> d_counts;
  d_counts.ensure((size_t)4 * m);
  const bool device_cache = op.rows_identity && stats_cache_enabled(bed);
  const StatsCols sel{op.cols_contig ? nullptr : ind_col, op.cols(), op.col0, m};
  if (device_cache && use_cache && stats_cache_known(bed, sel)) {
    stats_cache_load(bed, sel, d_counts.p, bed->stream);
    copy_d2h(bed, res, d_counts.p, (size_t)4 * m * 4);
    return;
  }
  counts_device(&op, ind_row, n, d_counts.p);
  if (device_cache) stats_cache_store(bed, sel, d_counts.p, bed->stream);   // (the download below synchronises)
  copy_d2h(bed, res, d_counts.p, (size_t)4 * m * 4);
  if (op.rows_identity) {  // remember which variants are complete
    if ((int64_t)bed->na_cnt.size() != bed->m) bed->na_cnt.assign((size_t)bed->m, -1);
    for (int64_t j = 0; j < m; j++) bed->na_cnt[(size_t)(ind_col ? ind_col[j] : j)] = res[4 * j + 3];
  }
  if (use_cache && !rows_all) {
    if (!same_rows) {
      cc.clear();
      cc.rows.assign(rows, rows + n);
      cc.cnt.assign((size_t)4 * bed->m, -1);
    }
    for (int64_t j = 0; j < m; j++) std::memcpy(&cc.cnt[(size_t)4 * (ind_col ? ind_col[j] : j)], res + 4 * j, 16);
  }
}

// ... resident, or slab by slab of an out-of-core handle
void counts_host(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                 int64_t m, int32_t *res) {
  if (!bed->streamed()) return counts_resident(bed, ind_row, n, ind_col, m, res);
  std::vector<int32_t> part;
  slab_walk(bed, ind_col, m, [&](const SlabPart &s) {
    part.resize((size_t)4 * s.P.size());
    counts_resident(s.img, ind_row, n, s.local.data(), s.count(), part.data());
    s.place(res, part.data(), 16);
  });
}

// ---- counts of the codes per group of rows (bsn_bed_group_counts; the table stays on the device for popstat.hip) ----------
// d_table: 4 x G x m int32, table[4 * (G * j + g) + c].  Reads and writes neither counts_cache nor stats_cache: the
// cached selections of the single-group calls stay as they are.
void group_counts_device(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int32_t *group, int32_t G,
                         const int64_t *ind_col, int64_t m, DevBuf<int32_t> &d_table, double ms_out[3]) {
  require_gpu();
  if (!bed) fail("bed_counts_by_group: no genotype handle");
  if (G < 1) fail("bed_counts_by_group: the number of groups should be at least 1 (got %d).", (int)G);
  if (n <= 0 || m <= 0) fail("'ind.row' and 'ind.col' can't be empty.");
  if (!group) fail("bed_counts_by_group: no group labels");
  require_bits(bed, 2, "bed_counts_by_group");
  refuse_generic(bed, "bed_counts_by_group");
  if ((double)G * (double)m * 4.0 >= 9.0e15) fail("bed_counts_by_group: the table of %d groups x %lld variants is too large", (int)G, (long long)m);
  BSN_HIP(hipSetDevice(bed->device));
  // ---- the labels: range, group sizes, and whether one digit holds every multiplicity ----
  const std::vector<int32_t> rows = to_i32(ind_row, n, bed->n, "ind.row");
  std::vector<int64_t> size64((size_t)G, 0);
  for (int64_t i = 0; i < n; i++) {
    const int32_t g = group[i];
    if (g < -1 || g >= G)
      fail("bed_counts_by_group: label %d of row %lld is outside -1 .. %d (-1: in no group).", (int)g, (long long)i, (int)(G - 1));
    if (g >= 0) size64[(size_t)g]++;
  }
  std::vector<int32_t> gsize((size_t)G);
  for (int32_t g = 0; g < G; g++) {
    if (size64[(size_t)g] > (int64_t)INT32_MAX)
      fail("bed_counts_by_group: group %d holds %lld rows, more than a 32-bit count.", (int)g, (long long)size64[(size_t)g]);
    gsize[(size_t)g] = (int32_t)size64[(size_t)g];
  }
  // (how often a file row was selected at all bounds its multiplicity under any one group: the pairs are only sorted
  // when that bound exceeds a digit)
  int64_t max_mult = 1;
  if (ind_row) {
    std::vector<int32_t> per_row((size_t)bed->n, 0);
    int32_t top = 0;
    for (int64_t i = 0; i < n; i++)
      if (group[i] >= 0) top = std::max(top, ++per_row[(size_t)rows[(size_t)i]]);
    max_mult = top;
    if (top > 127) {
      std::vector<int64_t> key;
      key.reserve((size_t)n);
      for (int64_t i = 0; i < n; i++)
        if (group[i] >= 0) key.push_back((int64_t)rows[(size_t)i] * G + group[i]);
      std::sort(key.begin(), key.end());
      max_mult = 0;
      for (size_t a = 0; a < key.size();) {
        size_t e = a;
        while (e < key.size() && key[e] == key[a]) e++;
        max_mult = std::max<int64_t>(max_mult, (int64_t)(e - a));
        a = e;
      }
    }
  }
  // (the four signed base-256 digits hold up to 0x7F7F7F7F)
  if (max_mult > 0x7F7F7F7FLL) fail("bed_counts_by_group: one row is selected %lld times under one group.", (long long)max_mult);
  const bool one_digit = max_mult <= 127;

  DevBuf<int32_t> d_rows, d_group, d_gsize;
  d_table.ensure((size_t)4 * G * m);
  auto upload = [&](bsn_bed *on) {
    if (ind_row) upload_list(on, d_rows, rows);
    copy_h2d(on, d_group.ensure((size_t)n), group, (size_t)n * 4);
    copy_h2d(on, d_gsize.ensure((size_t)G), gsize.data(), (size_t)G * 4);
  };
  if (bed->streamed()) {
    // slab by slab, exactly as counts_host walks: a slab's table comes back to the host, the whole one goes up once
    std::vector<int32_t> table((size_t)4 * G * m), part;
    DevBuf<int32_t> d_part;
    bsn_bed *img = slab_image(bed);
    upload(img);
    slab_walk(bed, ind_col, m, [&](const SlabPart &s) {
      const int64_t m_slab = s.count();
      bsn_op op;
      fill_op(&op, s.img, nullptr, s.img->n, s.local.data(), m_slab, nullptr, nullptr, true);
      counts_grouped(&op, ind_row ? d_rows.p : nullptr, d_group.p, n, G, d_gsize.p, one_digit, d_part.ensure((size_t)4 * G * m_slab),
                     ms_out);
      part.resize((size_t)4 * G * m_slab);
      copy_d2h(s.img, part.data(), d_part.p, part.size() * 4);
      s.place(table.data(), part.data(), (size_t)16 * G);
    });
    copy_h2d(img, d_table.p, table.data(), table.size() * 4);
    BSN_HIP(hipStreamSynchronize(img->stream));
    return;
  }
  upload(bed);
  bsn_op op;
  fill_op(&op, bed, nullptr, bed->n, ind_col, m, nullptr, nullptr, true);
  counts_grouped(&op, ind_row ? d_rows.p : nullptr, d_group.p, n, G, d_gsize.p, one_digit, d_table.p, ms_out);
}

// ---- the handle's device-resident code counts over all samples (bsn_bed::stats_cache) ---------------------------------
// to_cache: cache[variant of j] = counts[j]; else counts[j] = cache[variant of j].  One int4 per variant.
__global__ void k_stats_cache_copy(int32_t *cache, int32_t *counts, const int32_t *cols, int64_t col0, int64_t m, int to_cache) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int64_t c = cols ? (int64_t)cols[j] : col0 + j;
  if (to_cache) *(int4 *)(cache + 4 * c) = *(const int4 *)(counts + 4 * j);
  else *(int4 *)(counts + 4 * j) = *(const int4 *)(cache + 4 * c);
}

bool stats_cache_enabled(const bsn_bed *b) {
  return b->bits == 2 && !b->generic && b->d_img != nullptr && !getenv("BSN_NO_STATS_CACHE");
}

static void stats_cols_check(const bsn_bed *b, const StatsCols &c) {
  if (c.m <= 0 || (c.ind_col ? c.d_cols == nullptr : (c.col0 < 0 || c.col0 + c.m > b->m)))
    fail("internal: selection of variants for the handle's code counts");
}

bool stats_cache_known(const bsn_bed *b, const StatsCols &c) {
  const auto &sc = b->stats_cache;
  stats_cols_check(b, c);
  if ((int64_t)sc.known.size() != b->m) return false;
  if (sc.n_known == b->m) return true;
  for (int64_t j = 0; j < c.m; j++)
    if (!sc.known[(size_t)(c.ind_col ? c.ind_col[j] : c.col0 + j)]) return false;
  return true;
}

void stats_cache_store(bsn_bed *b, const StatsCols &c, const int32_t *d_counts, hipStream_t st) {
  auto &sc = b->stats_cache;
  stats_cols_check(b, c);
  hipLaunchKernelGGL(k_stats_cache_copy, dim3((unsigned)((c.m + 255) / 256)), dim3(256), 0, st,
                     sc.d_cnt.ensure((size_t)4 * b->m), const_cast<int32_t *>(d_counts), c.d_cols, c.col0, c.m, 1);
  BSN_HIP(hipGetLastError());
  if ((int64_t)sc.known.size() != b->m) {
    sc.known.assign((size_t)b->m, 0);
    sc.n_known = 0;
  }
  for (int64_t j = 0; j < c.m; j++) {
    uint8_t &k = sc.known[(size_t)(c.ind_col ? c.ind_col[j] : c.col0 + j)];
    sc.n_known += k == 0;
    k = 1;
  }
}

void stats_cache_load(bsn_bed *b, const StatsCols &c, int32_t *d_counts, hipStream_t st) {
  stats_cols_check(b, c);
  if (!stats_cache_known(b, c)) fail("internal: code counts asked of the handle's cache before they were written");
  hipLaunchKernelGGL(k_stats_cache_copy, dim3((unsigned)((c.m + 255) / 256)), dim3(256), 0, st, b->stats_cache.d_cnt.p,
                     d_counts, c.d_cols, c.col0, c.m, 0);
  BSN_HIP(hipGetLastError());
}

// ---- multLinReg on the device ----------------------------------------------------------------
// X = [U, U^2] (n x 2K) and the column totals sum_i y, sum_i y^2 (one workgroup per column, fixed order)
__global__ __launch_bounds__(1024) void k_mlr_prepare(const double *U, int64_t n, int K, double *X, double *tot) {
  const int k = blockIdx.x;
  double s1 = 0, s2 = 0;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const double y = U[i + (int64_t)k * n], yy = y * y;
    X[i + (int64_t)k * n] = y;
    X[i + (int64_t)(K + k) * n] = yy;
    s1 += y;
    s2 += yy;
  }
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_down(s1, off);
    s2 += __shfl_down(s2, off);
  }
  __shared__ double sm[2][16];
  if ((threadIdx.x & 63) == 0) sm[0][threadIdx.x >> 6] = s1, sm[1][threadIdx.x >> 6] = s2;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; w++) s1 += sm[0][w], s2 += sm[1][w];
    tot[k] = s1;
    tot[K + k] = s2;
  }
}

// src/multLinReg.cpp:36-57 per (variant, column) from the plane sums: P = sum g y over the non-missing,
// Q = sum of y (columns < K) / y^2 (columns >= K) over the MISSING samples, counts = code counts
#pragma clang fp contract(off)
__global__ void k_mlr_final(const double *P, const double *Q, int64_t ld, const int32_t *counts, const double *tot,
                            int64_t m, int K, int64_t n, bool has_q, double *res) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y;
  if (j >= m) return;
  const int4 c = *(const int4 *)(counts + 4 * j);
  const int nona = (int)(n - c.w);
  const double xSum = (double)c.y + 2.0 * c.z, xxSum = (double)c.y + 4.0 * c.z;
  const double deno_x = xxSum - xSum * xSum / nona;
  const double xySum = P[j + (int64_t)k * ld];
  const double ySum = tot[k] - (has_q ? Q[j + (int64_t)k * ld] : 0.0);
  const double yySum = tot[K + k] - (has_q ? Q[j + (int64_t)(K + k) * ld] : 0.0);
  const double num = xySum - xSum * ySum / nona;
  const double deno_y = yySum - ySum * ySum / nona;
  const double deno = deno_x * deno_y - num * num;
  res[j + (int64_t)k * m] = (deno == 0 || nona < 2) ? __longlong_as_double(0x7ff8000000000000LL)
                                                    : num * sqrt((nona - 2) / deno);
}
#pragma clang fp contract(on)

}  // namespace bsn

using namespace bsn;

extern "C" {

int bsn_selftest(void) {
  return guarded([&] {
    require_gpu();
    selftest();
  });
}

// Name (as bsn_bed_streaming_kernels gives it) of the streaming kernel the last bsn_op_prod on this operator launched.
int bsn_op_last_kernel(bsn_op *op, char *buf, int64_t len) {
  return guarded([&] {
    if (!buf || len < 1) fail("bsn_op_last_kernel: no buffer");
    buf[0] = 0;
    if (!op->last_kernel) return;
    const char *mangled = hipKernelNameRefByPtr(op->last_kernel, op->bed->stream);
    if (!mangled) return;
    int status = 1;
    char *dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
    std::string name = (status == 0 && dem) ? dem : mangled;
    free(dem);
    const size_t par = name.find('(');
    if (par != std::string::npos) name.resize(par);
    snprintf(buf, (size_t)len, "%s", name.c_str());
  });
}

// The grid (prod_plan.hpp: CprodGrid) the first k_cprod launch of bsn_op_cprod over nvec vectors would take now; nothing runs.
// out9: blocks of variants, those of the whole rounds, slabs and chunks per slab of the blocks beyond them, chunks, variants of
// those blocks; then what the plan was made from: variants per workgroup, CUs (BSN_PLAN_CUS), workgroups of the kernel a CU
// holds — three zeros for a launch that keeps one workgroup per block.  A hook of tests/test_gpu_cprod_whole.py, which binds
// it itself: not part of the header's ABI, so that the Python side still loads an older build through BSN_LIB_PATH.
int bsn_op_cprod_grid(bsn_op *op, int nvec, int64_t *out9) {
  return guarded([&] {
    if (!out9) fail("bsn_op_cprod_grid: no buffer");
    op_cprod_grid(op, nvec, out9);
  });
}

// ---- operator -------------------------------------------------------------------
int bsn_op_create(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                  int64_t m, const double *center, const double *scale, bsn_op **out) {
  return guarded([&] {
    std::unique_ptr<bsn_op> op(new bsn_op());
    fill_op(op.get(), bed, ind_row, n, ind_col, m, center, scale);
    *out = op.release();
  });
}

int bsn_op_destroy(bsn_op *op) {
  return guarded([&] {
    if (op) {
      (void)hipSetDevice(op->bed->device);
      delete op;
    }
  });
}

int bsn_op_set_slices(bsn_op *op, int slices) {
  return guarded([&] {
    if (slices < 1 || slices > 7) fail("slices must be in 1..7");
    op->slices = slices;
  });
}

int bsn_op_prod(bsn_op *op, const double *d_X, int64_t ldx, int nvec, double *d_Y, int64_t ldy) {
  return guarded([&] {
    BSN_HIP(hipSetDevice(op->bed->device));
    op_prod(op, d_X, ldx, nvec, d_Y, ldy);
  });
}

int bsn_op_cprod(bsn_op *op, const double *d_X, int64_t ldx, int nvec, double *d_Z, int64_t ldz) {
  return guarded([&] {
    BSN_HIP(hipSetDevice(op->bed->device));
    op_cprod(op, d_X, ldx, nvec, d_Z, ldz);
  });
}

int bsn_op_sync(bsn_op *op) {
  return guarded([&] { BSN_HIP(hipStreamSynchronize(op->bed->stream)); });
}

// ---- .Call replacements ------------------------------------------------------------
static void matvec_resident(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                            int64_t m, const double *center, const double *scale, const double *x,
                            double *out, bool transpose, bsn_comm *comm = nullptr) {
  bsn_op op;
  // A~' x needs centre / scale only in its finalize kernel: their upload is queued on the second stream and runs
  // beside the streaming kernel (2-bit image; the byte and look-up kernels read them earlier)
  const bool late = transpose && bed->bits == 2 && !bed->generic && (center || scale);
  fill_op(&op, bed, ind_row, n, ind_col, m, center, scale, late);
  if (late) {   // (fill_op has only allocated centre / scale; a default is written here, on the main stream)
    op.late_center = center;
    op.late_scale = scale;
    if (!center) BSN_HIP(hipMemsetAsync(op.d_center.p, 0, (size_t)m * 8, bed->stream));
    if (!scale) {
      hipLaunchKernelGGL(k_fill_f64, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, bed->stream, op.d_scale.p, m, 1.0);
      BSN_HIP(hipGetLastError());
    }
  }
  op.slices = 7;  // 56-bit fixed point: fp64-grade for a single vector, still one MFMA column block
  int64_t nin = transpose ? n : m, nout = transpose ? m : n;
  DevBuf<double> d_in, d_out;
  copy_h2d(bed, d_in.ensure((size_t)nin), x, (size_t)nin * 8);
  d_out.ensure((size_t)nout);
  if (bed->generic) {   // arbitrary decode table: fp64 look-up kernels
    const int32_t *rows = op.rows(), *cols = op.cols();
    if (comm) fail("sharded products are not available for a generic decode table");
    if (transpose)
      lut_cprod(bed, rows, n, cols, op.col0, m, center ? op.d_center.p : nullptr, scale ? op.d_scale.p : nullptr,
                d_in.p, d_out.p);
    else
      lut_prod(bed, rows, n, cols, op.col0, m, center ? op.d_center.p : nullptr, scale ? op.d_scale.p : nullptr,
               d_in.p, d_out.p);
    copy_d2h(bed, out, d_out.p, (size_t)nout * 8);
    return;
  }
  if (transpose)
    op_cprod(&op, d_in.p, nin, 1, d_out.p, nout);
  else
    op_prod(&op, d_in.p, nin, 1, d_out.p, nout);
  if (comm) {  // column shards: sum of the partial products over the ranks, on the device
    if (transpose) fail("internal: the crossproduct of a column shard needs no exchange");
    if (comm->device != bed->device) fail("the communicator was created on another device");
    comm_allreduce_sum(comm, d_out.p, nout, bed->stream);
  }
  copy_d2h(bed, out, d_out.p, (size_t)nout * 8);
}

static void matvec_host(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                        int64_t m, const double *center, const double *scale, const double *x,
                        double *out, bool transpose, bsn_comm *comm = nullptr) {
  if (!bed->streamed()) return matvec_resident(bed, ind_row, n, ind_col, m, center, scale, x, out, transpose, comm);
  // out of core: A~' x slab by slab is the result slab by slab; A~ x is the sum of the slabs' products (added on the
  // host in ascending slab order: deterministic)
  if (comm) fail("sharded products are not available for an out-of-core handle");
  std::vector<double> ce, sc, xs, part;
  if (!transpose) std::fill(out, out + n, 0.0);
  slab_walk(bed, ind_col, m, [&](const SlabPart &s) {
    part.resize((size_t)(transpose ? s.count() : n));
    matvec_resident(s.img, ind_row, n, s.local.data(), s.count(), s.gather(center, ce), s.gather(scale, sc),
                    transpose ? x : s.gather(x, xs), part.data(), transpose);
    BSN_HIP(hipStreamSynchronize(s.img->stream));
    if (transpose) s.place(out, part.data(), 8);
    else
      for (int64_t i = 0; i < n; i++) out[i] += part[(size_t)i];
  });
}

int bsn_bed_prodvec(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                    int64_t m, const double *center, const double *scale, const double *x,
                    double *y) {
  return guarded([&] { matvec_host(bed, ind_row, n, ind_col, m, center, scale, x, y, false); });
}

int bsn_bed_prodvec_sharded(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                            int64_t m, const double *center, const double *scale, const double *x,
                            bsn_comm *comm, double *y) {
  return guarded([&] { matvec_host(bed, ind_row, n, ind_col, m, center, scale, x, y, false, comm); });
}

int bsn_bed_cprodvec(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                     int64_t m, const double *center, const double *scale, const double *x,
                     double *z) {
  return guarded([&] { matvec_host(bed, ind_row, n, ind_col, m, center, scale, x, z, true); });
}

int bsn_bed_col_counts(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                       int64_t m, int32_t *res) {
  return guarded([&] { counts_host(bed, ind_row, n, ind_col, m, res); });
}

int bsn_bed_row_counts(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m,
                       int32_t *res) {
  return guarded([&] {
    bsn_op op;
    fill_op(&op, bed, ind_row, n, ind_col, m, nullptr, nullptr);
    DevBuf<double> d_c;
    d_c.ensure((size_t)3 * n);
    op_row_counts(&op, d_c.p);
    std::vector<double> c((size_t)3 * n);
    copy_d2h(bed, c.data(), d_c.p, (size_t)3 * n * 8);
    for (int64_t i = 0; i < n; i++) {
      const int64_t n2 = (int64_t)c[(size_t)i], n1 = (int64_t)c[(size_t)(n + i)], na = (int64_t)c[(size_t)(2 * n + i)];
      res[4 * i + 0] = (int32_t)(m - n1 - n2 - na);
      res[4 * i + 1] = (int32_t)n1;
      res[4 * i + 2] = (int32_t)n2;
      res[4 * i + 3] = (int32_t)na;
    }
  });
}

int bsn_bed_colstats(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                     int64_t m, double *sumX, double *denoX, int32_t *nb_nona_col,
                     int32_t *n_bad) {
  return guarded([&] {
    // integer-exact restatement of src/bed-fun.cpp:22-38 from the code counts:
    // xSum = n1 + 2 n2, xxSum = n1 + 4 n2 (both exact in fp64), c = n - nNA
    std::vector<int32_t> cnt((size_t)4 * m);
    counts_host(bed, ind_row, n, ind_col, m, cnt.data());
    int32_t bad = 0;
    for (int64_t j = 0; j < m; j++) {
      const int32_t *c = &cnt[(size_t)4 * j];
      double xSum = (double)c[1] + 2.0 * c[2], xxSum = (double)c[1] + 4.0 * c[2];
      int32_t nona = (int32_t)(n - c[3]);
      sumX[j] = xSum;
      denoX[j] = xxSum - xSum * xSum / nona;
      nb_nona_col[j] = nona;
      if (2 * (int64_t)nona < n) bad++;
    }
    if (n_bad) *n_bad = bad;
  });
}

int bsn_snp_colstats(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                     int64_t m, double *sumX, double *denoX) {
  return guarded([&] {
    // src/colstats.cpp:22-32: no NA handling, denominator n.  The accessor decodes a missing code to
    // NA_real (code256 is passed as is, :14), which poisons the sums of its column: NaN here.
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    if (bed->generic) {   // arbitrary decode table: sum v and sum v^2 by look-up, src/colstats.cpp:22-32 in fp64
      bsn_op op;
      fill_op(&op, bed, ind_row, n, ind_col, m, nullptr, nullptr);
      DevBuf<double> d_st;
      lut_colstats(bed, op.rows(), n, op.cols(), op.col0, m, d_st.ensure((size_t)2 * m));
      std::vector<double> st((size_t)2 * m);
      copy_d2h(bed, st.data(), d_st.p, st.size() * 8);
      for (int64_t j = 0; j < m; j++) {
        sumX[j] = st[(size_t)(2 * j)];
        denoX[j] = st[(size_t)(2 * j + 1)] - st[(size_t)(2 * j)] * st[(size_t)(2 * j)] / n;
      }
      return;
    }
    if (bed->bits == 8) {
      bsn_op op;
      fill_op(&op, bed, ind_row, n, ind_col, m, nullptr, nullptr);
      DevBuf<long long> d_st;
      stats8(bed, op.rows(), n, op.cols(), op.col0, m, d_st.ensure((size_t)3 * m));
      std::vector<long long> st((size_t)3 * m);
      copy_d2h(bed, st.data(), d_st.p, st.size() * 8);
      const double a = bed->v_off, h = bed->v_step;
      for (int64_t j = 0; j < m; j++) {
        const double s1 = (double)st[(size_t)(3 * j)], s2 = (double)st[(size_t)(3 * j + 1)];
        // sum v = n a + h S1;  sum v^2 = n a^2 + 2 a h S1 + h^2 S2   (v = a + h k, exact integer S1, S2)
        const double xSum = (double)n * a + h * s1;
        const double xxSum = (double)n * a * a + 2.0 * a * h * s1 + h * h * s2;
        const bool na = st[(size_t)(3 * j + 2)] > 0;
        sumX[j] = na ? qnan : xSum;
        denoX[j] = na ? qnan : xxSum - xSum * xSum / n;
      }
      return;
    }
    std::vector<int32_t> cnt((size_t)4 * m);
    counts_host(bed, ind_row, n, ind_col, m, cnt.data());
    for (int64_t j = 0; j < m; j++) {
      const int32_t *c = &cnt[(size_t)4 * j];
      double xSum = (double)c[1] + 2.0 * c[2];
      double xxSum = (double)c[1] + 4.0 * c[2];
      sumX[j] = c[3] > 0 ? qnan : xSum;
      denoX[j] = c[3] > 0 ? qnan : xxSum - xSum * xSum / n;
    }
  });
}

static void read_resident(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                          int64_t m, const double *center, const double *scale, int32_t na_val,
                          int32_t *out_i, double *out_d) {
  DevBuf<int32_t> d_r, d_c, d_oi;
  DevBuf<double> d_ce, d_sc, d_od;
  upload_list(bed, d_r, to_i32(ind_row, n, bed->n, "ind.row"));
  upload_list(bed, d_c, to_i32(ind_col, m, bed->m, "ind.col"));
  if (out_d) {
    copy_h2d(bed, d_ce.ensure((size_t)m), center, (size_t)m * 8);
    copy_h2d(bed, d_sc.ensure((size_t)m), scale, (size_t)m * 8);
    d_od.ensure((size_t)n * m);
  } else {
    d_oi.ensure((size_t)n * m);
  }
  read_dense(bed, d_r.p, n, d_c.p, m, d_ce.p, d_sc.p, na_val, d_oi.p, d_od.p);
  BSN_HIP(hipStreamSynchronize(bed->stream));
  if (out_d)
    copy_d2h(bed, out_d, d_od.p, (size_t)n * m * 8);
  else
    copy_d2h(bed, out_i, d_oi.p, (size_t)n * m * 4);
}

static void read_host(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                      int64_t m, const double *center, const double *scale, int32_t na_val,
                      int32_t *out_i, double *out_d) {
  if (n <= 0 || m <= 0) fail("'ind.row' and 'ind.col' can't be empty.");
  BSN_HIP(hipSetDevice(bed->device));
  if (!bed->streamed()) return read_resident(bed, ind_row, n, ind_col, m, center, scale, na_val, out_i, out_d);
  // out of core: the columns of every slab, placed where ind.col has them
  std::vector<uint8_t> part;
  std::vector<double> ce, sc;
  const size_t col_bytes = (size_t)n * (out_d ? 8 : 4);
  slab_walk(bed, ind_col, m, [&](const SlabPart &s) {
    part.resize(col_bytes * (size_t)s.count());
    read_resident(s.img, ind_row, n, s.local.data(), s.count(), s.gather(center, ce), s.gather(scale, sc), na_val,
                  out_d ? nullptr : (int32_t *)part.data(), out_d ? (double *)part.data() : nullptr);
    BSN_HIP(hipStreamSynchronize(s.img->stream));
    s.place(out_d ? (void *)out_d : (void *)out_i, part.data(), col_bytes);
  });
}

int bsn_bed_read(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                 int64_t m, int32_t na_val, int32_t *out) {
  return guarded([&] { read_host(bed, ind_row, n, ind_col, m, nullptr, nullptr, na_val, out, nullptr); });
}

int bsn_bed_read_scaled(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                        int64_t m, const double *center, const double *scale, double *out) {
  return guarded([&] { read_host(bed, ind_row, n, ind_col, m, center, scale, 0, nullptr, out); });
}

// plane sums behind multLinReg (src/multLinReg.cpp:25-44)
int bsn_bed_cprod_planes(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                         int64_t m, const double *X, int64_t K, double *P, double *Q) {
  return guarded([&] {
    if (K <= 0) fail("'U' must have at least one column.");
    bsn_op op;
    fill_op(&op, bed, ind_row, n, ind_col, m, nullptr, nullptr);
    op.slices = 7;
    DevBuf<double> d_X, d_P, d_Q;
    copy_h2d(bed, d_X.ensure((size_t)n * K), X, (size_t)n * K * 8);
    d_P.ensure((size_t)m * K);
    d_Q.ensure((size_t)m * K);
    op_cprod_raw(&op, d_X.p, n, (int)K, d_P.p, d_Q.p, m);
    copy_d2h(bed, P, d_P.p, (size_t)m * K * 8);
    copy_d2h(bed, Q, d_Q.p, (size_t)m * K * 8);
    BSN_HIP(hipStreamSynchronize(bed->stream));
  });
}

// _bigsnpr_prod_and_rowSumsSq (6 args) src/bed-fun.cpp:103-133
int bsn_bed_prod_and_rowsumssq(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                               int64_t m, const double *center, const double *scale, const double *V,
                               int64_t K, double *XV, double *rowSumsSq) {
  return guarded([&] {
    if (K <= 0) fail("'V' must have at least one column.");
    bsn_op op;
    fill_op(&op, bed, ind_row, n, ind_col, m, center, scale);
    op.slices = 7;
    DevBuf<double> d_V, d_XV, d_r;
    copy_h2d(bed, d_V.ensure((size_t)m * K), V, (size_t)m * K * 8);
    d_XV.ensure((size_t)n * K);
    d_r.ensure((size_t)n);
    op_prod(&op, d_V.p, m, (int)K, d_XV.p, n);
    op_row_sums_sq(&op, d_r.p);
    copy_d2h(bed, XV, d_XV.p, (size_t)n * K * 8);
    copy_d2h(bed, rowSumsSq, d_r.p, (size_t)n * 8);
    BSN_HIP(hipStreamSynchronize(bed->stream));
  });
}

// _bigsnpr_multLinReg (5 args) src/multLinReg.cpp:8-86: K t-scores per variant.  The sums over the
// samples are plane sums of the crossproduct kernel on the panels (U, U^2) at 56 bits plus the exact
// genotype counts; the rest is the reference's expressions per (variant, column).  NA_REAL -> NaN.
int bsn_mult_lin_reg(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m,
                     const double *U, int64_t K, double *res) {
  return guarded([&] {
    if (K <= 0) fail("'U' must have at least one column.");
    if (K > 1024) fail("'U' has too many columns.");
    bsn_op op;
    fill_op(&op, bed, ind_row, n, ind_col, m, nullptr, nullptr, true);
    op.slices = 7;
    DevBuf<double> d_U, d_X, d_P, d_Q, d_tot, d_res;
    DevBuf<int32_t> d_counts;
    copy_h2d(bed, d_U.ensure((size_t)n * K), U, (size_t)n * K * 8);
    d_X.ensure((size_t)n * 2 * K);
    d_tot.ensure((size_t)2 * K);
    hipLaunchKernelGGL(k_mlr_prepare, dim3((unsigned)K), dim3(1024), 0, bed->stream, d_U.p, n, (int)K, d_X.p, d_tot.p);
    BSN_HIP(hipGetLastError());
    counts_device(&op, ind_row, n, d_counts.ensure((size_t)4 * m));
    // complete data (known from an earlier counting pass): the sums over the missing samples are zero and the
    // squared columns are not needed at all
    const bool has_q = !op.no_na;
    const int nvec = (int)(has_q ? 2 * K : K);
    d_P.ensure((size_t)m * nvec);
    d_Q.ensure((size_t)m * nvec);
    op_cprod_raw(&op, d_X.p, n, nvec, d_P.p, d_Q.p, m);
    d_res.ensure((size_t)m * K);
    hipLaunchKernelGGL(k_mlr_final, dim3((unsigned)((m + 255) / 256), (unsigned)K), dim3(256), 0, bed->stream, d_P.p,
                       d_Q.p, m, d_counts.p, d_tot.p, m, (int)K, n, has_q, d_res.p);
    BSN_HIP(hipGetLastError());
    copy_d2h(bed, res, d_res.p, (size_t)m * K * 8);
  });
}

// _bigsnpr_prod_and_rowSumsSq2 (6 args) src/project-utils.cpp:12-43, the FBM.code256 twin: the FBM
// accessor has no missing-value handling, so a missing code is NA_real and poisons its whole row of XV
// and its rowSumsSq entry (:33-38) — reproduced with NaN from the per-sample missing counts.
int bsn_snp_prod_and_rowsumssq2(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                                int64_t m, const double *center, const double *scale, const double *V,
                                int64_t K, double *XV, double *rowSumsSq) {
  int rc = bsn_bed_prod_and_rowsumssq(bed, ind_row, n, ind_col, m, center, scale, V, K, XV, rowSumsSq);
  if (rc != 0) return rc;
  return guarded([&] {
    std::vector<int32_t> rcnt((size_t)4 * n);
    if (bsn_bed_row_counts(bed, ind_row, n, ind_col, m, rcnt.data()) != 0) throw Error(bsn_last_error());
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t i = 0; i < n; i++)
      if (rcnt[(size_t)(4 * i + 3)] > 0) {
        for (int64_t k = 0; k < K; k++) XV[i + k * n] = qnan;
        rowSumsSq[i] = qnan;
      }
  });
}

// running sums of snp_grid_PRS: last[:, c] += Y[:, c]; out[:, c * T + t] = last[:, c]
__global__ void k_prs_accum(const double *__restrict__ Y, int64_t n, int64_t C, double *__restrict__ last,
                            double *__restrict__ out, int64_t T, int64_t t) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * C) return;
  const int64_t i = idx % n, c = idx / n;
  const double v = last[idx] + (Y ? Y[idx] : 0.0);
  last[idx] = v;
  out[(c * T + t) * n + i] = v;
}

int bsn_snp_grid_prs(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m,
                     const double *betas, const int32_t *bin, const uint8_t *member, int64_t C, int64_t T,
                     int slices, double *out) {
  return guarded([&] {
    if (n <= 0) fail("'ind.row' can't be empty.");
    if (C <= 0 || T <= 0) fail("the grid is empty");
    require_gpu();
    BSN_HIP(hipSetDevice(bed->device));
    // columns by bin, highest first (R/PRS.R:66-73 accumulates from the highest threshold down)
    std::vector<std::vector<int64_t>> by_bin((size_t)T + 1);
    for (int64_t j = 0; j < m; j++) {
      if (bin[j] < 0 || bin[j] > T) fail("'bin' out of range");
      bool any = false;
      for (int64_t c = 0; c < C && !any; c++) any = member[c * m + j] != 0;
      if (any && bin[j] > 0) by_bin[(size_t)bin[j]].push_back(j);
    }
    DevBuf<double> d_last, d_out, d_V, d_Y;
    BSN_HIP(hipMemsetAsync(d_last.ensure((size_t)n * C), 0, (size_t)n * C * 8, bed->stream));
    d_out.ensure((size_t)n * C * T);
    d_Y.ensure((size_t)n * C);
    std::vector<double> V;
    std::vector<int64_t> cols;
    const unsigned nblk = (unsigned)((n * C + 255) / 256);
    for (int64_t b = T; b >= 1; b--) {
      const std::vector<int64_t> &jj = by_bin[(size_t)b];
      const int64_t mb = (int64_t)jj.size();
      if (mb > 0) {
        cols.resize((size_t)mb);
        V.assign((size_t)mb * C, 0.0);
        for (int64_t k = 0; k < mb; k++) {
          cols[(size_t)k] = ind_col ? ind_col[jj[(size_t)k]] : jj[(size_t)k];
          for (int64_t c = 0; c < C; c++)
            if (member[c * m + jj[(size_t)k]]) V[(size_t)(c * mb + k)] = betas[jj[(size_t)k]];
        }
        bsn_op op;
        fill_op(&op, bed, ind_row, n, cols.data(), mb, nullptr, nullptr);
        op.slices = slices > 0 ? slices : 7;
        copy_h2d(bed, d_V.ensure((size_t)mb * C), V.data(), (size_t)mb * C * 8);
        op_prod(&op, d_V.p, mb, (int)C, d_Y.p, n);
        hipLaunchKernelGGL(k_prs_accum, dim3(nblk), dim3(256), 0, bed->stream, d_Y.p, n, C, d_last.p, d_out.p,
                           T, b - 1);
        BSN_HIP(hipGetLastError());
        BSN_HIP(hipStreamSynchronize(bed->stream));  // `op` and V are reused by the next bin
      } else {
        hipLaunchKernelGGL(k_prs_accum, dim3(nblk), dim3(256), 0, bed->stream, (const double *)nullptr, n, C,
                           d_last.p, d_out.p, T, b - 1);
        BSN_HIP(hipGetLastError());
      }
    }
    copy_d2h(bed, out, d_out.p, (size_t)n * C * T * 8);
    BSN_HIP(hipStreamSynchronize(bed->stream));
  });
}

static void convert_resident(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                             int64_t m, uint8_t *out, bool packed) {
  DevBuf<int32_t> d_r, d_c;
  DevBuf<uint8_t> d_o;
  upload_list(bed, d_r, to_i32(ind_row, n, bed->n, "ind.row"));
  upload_list(bed, d_c, to_i32(ind_col, m, bed->m, "ind.col"));
  const size_t bytes = packed ? (size_t)((n + 3) / 4) * m : (size_t)n * m;
  d_o.ensure(bytes);
  if (packed)
    subset_pack(bed, d_r.p, n, d_c.p, m, d_o.p);
  else
    to_bytes(bed, d_r.p, n, d_c.p, m, d_o.p);
  copy_d2h(bed, out, d_o.p, bytes);
  BSN_HIP(hipStreamSynchronize(bed->stream));
}

static void convert_host(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                         int64_t m, uint8_t *out, bool packed) {
  if (n <= 0 || m <= 0) fail("'ind.row' and 'ind.col' can't be empty.");
  BSN_HIP(hipSetDevice(bed->device));
  if (!bed->streamed()) return convert_resident(bed, ind_row, n, ind_col, m, out, packed);
  // (round 6) out of core: a column of the result depends on ONE variant, so the selected variants are served slab by
  // slab of the file (the reference maps the file and walks it: src/read-plink.cpp:61-80, src/write-plink.cpp:13-52);
  // every slab's columns go to their places in the caller's array — byte-identical to the resident conversion.  The row
  // list goes up once and every transfer runs through the HANDLE's staging buffers, so the slabs do not call the
  // resident body
  const size_t col_bytes = packed ? (size_t)((n + 3) / 4) : (size_t)n;
  DevBuf<int32_t> d_r, d_c;
  DevBuf<uint8_t> d_o;
  std::vector<uint8_t> h_o;
  upload_list(bed, d_r, to_i32(ind_row, n, bed->n, "ind.row"));
  slab_walk(bed, ind_col, m, [&](const SlabPart &s) {
    const int64_t ml = s.count();
    upload_list(bed, d_c, to_i32(s.local.data(), ml, s.img->m, "ind.col"));
    d_o.ensure(col_bytes * (size_t)ml);
    if (packed) subset_pack(s.img, d_r.p, n, d_c.p, ml, d_o.p);
    else to_bytes(s.img, d_r.p, n, d_c.p, ml, d_o.p);
    h_o.resize(col_bytes * (size_t)ml);
    copy_d2h(bed, h_o.data(), d_o.p, h_o.size());
    BSN_HIP(hipStreamSynchronize(bed->stream));
    s.place(out, h_o.data(), col_bytes);
  });
}

int bsn_bed_to_fbm(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m,
                   uint8_t *out) {
  return guarded([&] { convert_host(bed, ind_row, n, ind_col, m, out, false); });
}

int bsn_bed_readbina(bsn_bed *bed, const uint8_t *tab, uint8_t *out) {
  return guarded([&] {
    if (!tab || !out) fail("readbina: 'tab' and the output must not be NULL");
    BSN_HIP(hipSetDevice(bed->device));
    DevBuf<uint8_t> d_tab, d_o;
    copy_h2d(bed, d_tab.ensure(1024), tab, 1024);
    if (bed->streamed()) {   // (round 6) out of core: slab by slab of the file, each slab's n x cnt bytes to its place
      slab_walk(bed, nullptr, bed->m, [&](const SlabPart &s) {   // (every variant: a slab's positions are one run)
        const size_t bytes = (size_t)bed->n * (size_t)s.count();
        readbina_bytes(s.img, d_tab.p, d_o.ensure(bytes));
        copy_d2h(bed, out + (size_t)s.P[0] * (size_t)bed->n, d_o.p, bytes);
        BSN_HIP(hipStreamSynchronize(bed->stream));
      });
      return;
    }
    const size_t bytes = (size_t)bed->n * (size_t)bed->m;
    readbina_bytes(bed, d_tab.p, d_o.ensure(bytes));
    copy_d2h(bed, out, d_o.p, bytes);
    BSN_HIP(hipStreamSynchronize(bed->stream));
  });
}

int bsn_bed_subset_payload(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                           int64_t m, uint8_t *payload_out) {
  return guarded([&] { convert_host(bed, ind_row, n, ind_col, m, payload_out, true); });
}

}  // extern "C"
