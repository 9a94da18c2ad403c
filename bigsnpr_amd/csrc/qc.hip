// qc.hip — the exact Hardy–Weinberg test per variant (bsn_hwe, bsn_bed_hwe) and the filters of plink --mind --geno --maf
// --hwe in one call (bsn_bed_qc).
//
// Replaces the PLINK run of snp_plinkQC (R/external-software.R:247-290 of the reference).  The per-sample counts are the
// pass of bsn_bed_row_counts, the per-variant counts over the three classes of samples the grouped counting pass
// (counts_grouped in matvec.hip); their results stay on the device, where one kernel makes the labels of the second pass
// from the first, one runs the test and one forms the masks.  The test and every comparison live in hwe_step.hpp, shared
// with the CPU statement.  DESIGN.md 3.5o.
#include <cstring>
#include <vector>

#include "bsn_internal.hpp"
#include "hwe_step.hpp"

namespace bsn {
namespace {

// device milliseconds of the last call of this process (bsn_qc_last_ms): the per-sample counts, the per-class counting
// pass, the test kernel, the masks
double g_last_ms[4] = {0.0, 0.0, 0.0, 0.0};

// The test kernel has no LDS and no barrier, and the trip counts of neighbouring variants differ by orders of magnitude (a
// rare variant ends in tens of steps, a common one among 200 000 samples takes thousands).  A workgroup is one wave: the
// smallest unit the dispatcher can hand to a free SIMD, so a wave held by one long variant holds nothing else.  The loop
// body is a correctly rounded fp64 division of two products of counts, which does not wait for the running term, and a
// multiply and two or three additions that do; it needs few registers, so the waves per SIMD are bounded by the grid, not
// by the kernel.
constexpr int kHweBlock = 64;
// The form bsn_hwe and the handle entries take.  Measured against each other on the counts of 50 000 samples x 200 000
// variants (tools/probe_qc.py, profiles/qc_c2.json; 3 021 terms per variant on average, 547 to 4 213): one lane per
// variant 1.41 ms, two lanes 2.11 ms.  Both stay built: they return the same bits, and the tests hold them to it.
constexpr int kHweLanes = 1;

// p[j] from the counts t[stride * j + 0 .. 2] = hom1, het, hom2.
// LANES == 1: thread j walks down, then up.  LANES == 2: lanes 2 j and 2 j + 1 of a wave take one walk each and lane 2 j
// combines them — the same two accumulations in the same order, hence the same bits.
template <int LANES>
__global__ __launch_bounds__(kHweBlock) void k_hwe_exact(const int32_t *__restrict__ t, int64_t stride, int64_t m, int midp,
                                                         double *__restrict__ p) {
  const int64_t gid = (int64_t)blockIdx.x * kHweBlock + threadIdx.x;
  const int64_t j = LANES == 2 ? gid >> 1 : gid;
  const bool valid = j < m;
  hwe::Start s = hwe::start(0, 0, 0);
  if (valid) s = hwe::start(t[stride * j], t[stride * j + 1], t[stride * j + 2]);
  const bool mp = midp != 0;
  if constexpr (LANES == 1) {
    if (!valid) return;
    if (!s.ok) {
      p[j] = s.fixed;
      return;
    }
    const hwe::Walk down = hwe::walk_down(s.het, s.homr, s.homc, mp);
    const hwe::Walk up = hwe::walk_up(s.het, s.homr, s.homc, s.rare, mp);
    p[j] = hwe::combine(down, up, mp);
  } else {
    // (no early return: every lane of the wave takes part in the exchange below)
    const bool is_up = (gid & 1) != 0;
    hwe::Walk mine = {0.0, 0.0, 0};
    if (s.ok) mine = is_up ? hwe::walk_up(s.het, s.homr, s.homc, s.rare, mp) : hwe::walk_down(s.het, s.homr, s.homc, mp);
    hwe::Walk other;
    other.total = __shfl_xor(mine.total, 1);
    other.tail = __shfl_xor(mine.tail, 1);
    other.steps = 0;
    if (valid && !is_up) p[j] = s.ok ? hwe::combine(mine, other, mp) : s.fixed;
  }
}

// queues the test on `st`; lanes: 1, 2 or 0 = kHweLanes
void launch_hwe(const int32_t *d_t, int64_t stride, int64_t m, int midp, int lanes, double *d_p, hipStream_t st) {
  if (lanes == 0) lanes = kHweLanes;
  if (lanes != 1 && lanes != 2) fail("hwe: 'lanes' should be 0, 1 or 2 (got %d).", lanes);
  const int64_t threads = m * lanes, blocks = (threads + kHweBlock - 1) / kHweBlock;
  if (blocks > (int64_t)INT32_MAX) fail("hwe: %lld variants are too many for one launch.", (long long)m);
  if (lanes == 1) hipLaunchKernelGGL(k_hwe_exact<1>, dim3((unsigned)blocks), dim3(kHweBlock), 0, st, d_t, stride, m, midp, d_p);
  else hipLaunchKernelGGL(k_hwe_exact<2>, dim3((unsigned)blocks), dim3(kHweBlock), 0, st, d_t, stride, m, midp, d_p);
  BSN_HIP(hipGetLastError());
}

void hwe_host(const int32_t *counts, int64_t m, int midp, int lanes, double *p_out, double *ms_out) {
  require_gpu();
  if (m <= 0) fail("hwe: no variant");
  if (!counts || !p_out) fail("hwe: no counts or no result buffer");
  for (int64_t j = 0; j < m; j++) {
    const int32_t *c = counts + 3 * j;
    if (c[0] < 0 || c[1] < 0 || c[2] < 0)
      fail("hwe: variant %lld has a negative count (%d, %d, %d).", (long long)j, (int)c[0], (int)c[1], (int)c[2]);
    if ((int64_t)c[0] + c[1] + c[2] > (int64_t)INT32_MAX)
      fail("hwe: variant %lld has %lld genotypes, more than a 32-bit count.", (long long)j, (long long)c[0] + c[1] + c[2]);
  }
  DevBuf<int32_t> d_t;
  DevBuf<double> d_p;
  BSN_HIP(hipMemcpy(d_t.ensure((size_t)3 * m), counts, (size_t)3 * m * 4, hipMemcpyHostToDevice));
  d_p.ensure((size_t)m);
  EventMarks<2> ev;
  ev.mark(0, nullptr);
  launch_hwe(d_t.p, 3, m, midp, lanes, d_p.p, nullptr);
  ev.mark(1, nullptr);
  BSN_HIP(hipStreamSynchronize(nullptr));
  BSN_HIP(hipMemcpy(p_out, d_p.p, (size_t)m * 8, hipMemcpyDeviceToHost));
  for (double &v : g_last_ms) v = 0.0;
  g_last_ms[2] = ev.ms(0, 1);
  if (ms_out) *ms_out = g_last_ms[2];
}

void check_rows(const bsn_bed *bed, int64_t n, const char *what) {
  if (!bed) fail("%s: no genotype handle", what);
  if (n > (int64_t)INT32_MAX) fail("%s: %lld samples are more than a 32-bit count.", what, (long long)n);
}

void bed_hwe(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, int midp, double *p_out,
             int32_t *counts_out) {
  check_rows(bed, n, "bed_hwe");
  if (!p_out) fail("bed_hwe: no result buffer");
  require_bits(bed, 2, "bed_hwe");
  refuse_generic(bed, "bed_hwe");
  for (double &v : g_last_ms) v = 0.0;
  if (n <= 0 || m <= 0) fail("'ind.row' and 'ind.col' can't be empty.");
  const std::vector<int32_t> group((size_t)n, 0);
  DevBuf<int32_t> d_table;
  double ms3[3] = {0.0, 0.0, 0.0};
  group_counts_device(bed, ind_row, n, group.data(), 1, ind_col, m, d_table, ms3);
  g_last_ms[1] = ms3[0] + ms3[1] + ms3[2];
  bsn_bed *on = bed->streamed() ? slab_image(bed) : bed;
  hipStream_t st = on->stream;
  DevBuf<double> d_p;
  d_p.ensure((size_t)m);
  EventMarks<2> ev;
  ev.mark(0, st);
  launch_hwe(d_table.p, 4, m, midp, 0, d_p.p, st);
  ev.mark(1, st);
  copy_d2h(on, p_out, d_p.p, (size_t)m * 8);
  if (counts_out) copy_d2h(on, counts_out, d_table.p, (size_t)4 * m * 4);
  BSN_HIP(hipStreamSynchronize(st));
  g_last_ms[2] = ev.ms(0, 1);
}

// ---- bsn_bed_qc --------------------------------------------------------------------------------------------------------
// From the per-sample counts (rc: 3 x n doubles, the missing calls at 2 n + i): keep_row, row_miss (may be NULL), the label
// of the second pass (cls[i], or -1 for a removed sample) and the class sizes of S1 (integer atomics: exact).
__global__ void k_qc_rows(const double *__restrict__ rc, const int32_t *__restrict__ cls, int64_t n, int64_t m, double mind,
                          uint8_t *keep_row, double *row_miss, int32_t *label, int32_t *gsize) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t na = (int64_t)rc[2 * n + i];
  const bool out = hwe::too_many_missing(na, m, mind);
  keep_row[i] = out ? 0 : 1;
  if (row_miss) row_miss[i] = hwe::missing_rate(na, m);
  const int32_t c = cls[i];
  label[i] = out ? -1 : c;
  if (!out) atomicAdd(&gsize[c], 1);
}

// the count table of classes 0, 1, 2 (table[4 * (3 j + g) + c]) and p -> keep_col and col_stats (may be NULL)
__global__ void k_qc_cols(const int32_t *__restrict__ table, const int32_t *__restrict__ gsize, const double *__restrict__ p,
                          int64_t m, double maf, double geno, double hwe_thr, uint8_t *keep_col, double *col_stats) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int4 a = *(const int4 *)(table + 12 * j), b = *(const int4 *)(table + 12 * j + 4), c = *(const int4 *)(table + 12 * j + 8);
  const int64_t s1 = (int64_t)gsize[0] + gsize[1] + gsize[2];
  const int64_t na = (int64_t)a.w + b.w + c.w;
  const double maf_j = hwe::maf_from_counts((int64_t)a.x + b.x, (int64_t)a.y + b.y, (int64_t)a.z + b.z);
  const double pj = p ? p[j] : 1.0;
  const bool out = hwe::too_many_missing(na, s1, geno) || hwe::hwe_rejected(pj, hwe_thr) || hwe::maf_too_low(maf_j, maf);
  keep_col[j] = out ? 0 : 1;
  if (col_stats) {
    col_stats[3 * j] = hwe::missing_rate(na, s1);
    col_stats[3 * j + 1] = maf_j;
    col_stats[3 * j + 2] = pj;
  }
}

void check_rate(double v, const char *name) {
  if (!(v >= 0.0 && v <= 1.0)) fail("bed_plinkQC: '%s' should be in range [0, 1] (got %g).", name, v);
}

void bed_qc(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const int32_t *cls, double maf,
            double geno, double mind, double hwe_thr, int midp, uint8_t *keep_row, uint8_t *keep_col, double *row_miss,
            double *col_stats) {
  require_gpu();
  check_rows(bed, n, "bed_plinkQC");
  check_rate(maf, "maf");
  check_rate(geno, "geno");
  check_rate(mind, "mind");
  check_rate(hwe_thr, "hwe");
  if (n <= 0 || m <= 0) fail("'ind.row' and 'ind.col' can't be empty.");
  if (!cls) fail("bed_plinkQC: no sample classes");
  if (!keep_row || !keep_col) fail("bed_plinkQC: no result buffers");
  require_bits(bed, 2, "bed_plinkQC");
  refuse_generic(bed, "bed_plinkQC");
  require_resident(bed, "bed_plinkQC");
  for (int64_t i = 0; i < n; i++)
    if (cls[i] < 0 || cls[i] > 2)
      fail("bed_plinkQC: class %d of row %lld is outside 0 .. 2 (founder counted for the test, founder, non-founder).",
           (int)cls[i], (long long)i);
  // the file rows of the selection, checked, and how often one of them is selected: one int8 digit of the counting pass
  // holds a multiplicity up to 127
  std::vector<int32_t> rows;
  bool one_digit = true;
  if (ind_row) {
    rows.resize((size_t)n);
    std::vector<int32_t> per_row((size_t)bed->n, 0);
    for (int64_t i = 0; i < n; i++) {
      if (ind_row[i] < 0 || ind_row[i] >= bed->n)
        fail("Tested %lld < %lld. Subscript out of bounds (ind.row).", (long long)ind_row[i], (long long)bed->n);
      rows[(size_t)i] = (int32_t)ind_row[i];
      if (++per_row[(size_t)ind_row[i]] > 127) one_digit = false;
    }
  } else if (n > bed->n) {
    fail("Tested %lld < %lld. Subscript out of bounds (ind.row).", (long long)(n - 1), (long long)bed->n);
  }
  BSN_HIP(hipSetDevice(bed->device));
  hipStream_t st = bed->stream;
  for (double &v : g_last_ms) v = 0.0;
  EventMarks<6> ev;

  DevBuf<int32_t> d_cls, d_label, d_gsize, d_rows, d_table;
  DevBuf<uint8_t> d_keep_row, d_keep_col;
  DevBuf<double> d_row_miss, d_p, d_stats;
  copy_h2d(bed, d_cls.ensure((size_t)n), cls, (size_t)n * 4);
  if (ind_row) copy_h2d(bed, d_rows.ensure((size_t)n), rows.data(), (size_t)n * 4);
  d_label.ensure((size_t)n);
  d_keep_row.ensure((size_t)n);
  d_keep_col.ensure((size_t)m);
  if (row_miss) d_row_miss.ensure((size_t)n);
  if (col_stats) d_stats.ensure((size_t)3 * m);

  // 1. the per-sample counts over the selected variants
  DevBuf<double> d_rc;
  d_rc.ensure((size_t)3 * n);
  {
    bsn_op op;
    fill_op(&op, bed, ind_row, n, ind_col, m, nullptr, nullptr);
    ev.mark(0, st);
    op_row_counts(&op, d_rc.p);
    ev.mark(1, st);
  }
  // ... -> keep_row, the labels and class sizes of S1
  BSN_HIP(hipMemsetAsync(d_gsize.ensure(4), 0, 16, st));
  hipLaunchKernelGGL(k_qc_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_rc.p, d_cls.p, n, m, mind, d_keep_row.p,
                     row_miss ? d_row_miss.p : nullptr, d_label.p, d_gsize.p);
  BSN_HIP(hipGetLastError());
  ev.mark(2, st);

  // 2. the counts of every variant over the classes of S1, the test over class 0, the masks
  d_table.ensure((size_t)12 * m);
  double ms3[3] = {0.0, 0.0, 0.0};
  {
    bsn_op op;
    fill_op(&op, bed, nullptr, bed->n, ind_col, m, nullptr, nullptr, true);
    counts_grouped(&op, ind_row ? d_rows.p : nullptr, d_label.p, n, 3, d_gsize.p, one_digit, d_table.p, ms3);
  }
  const bool test = hwe_thr > 0.0 || col_stats;
  ev.mark(3, st);
  if (test) launch_hwe(d_table.p, 12, m, midp, 0, d_p.ensure((size_t)m), st);
  ev.mark(4, st);
  hipLaunchKernelGGL(k_qc_cols, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, d_table.p, d_gsize.p, test ? d_p.p : nullptr, m,
                     maf, geno, hwe_thr, d_keep_col.p, col_stats ? d_stats.p : nullptr);
  BSN_HIP(hipGetLastError());
  ev.mark(5, st);

  int32_t gsize[4];
  copy_d2h(bed, gsize, d_gsize.p, 16);
  copy_d2h(bed, keep_row, d_keep_row.p, (size_t)n);
  copy_d2h(bed, keep_col, d_keep_col.p, (size_t)m);
  if (row_miss) copy_d2h(bed, row_miss, d_row_miss.p, (size_t)n * 8);
  if (col_stats) copy_d2h(bed, col_stats, d_stats.p, (size_t)3 * m * 8);
  BSN_HIP(hipStreamSynchronize(st));
  g_last_ms[0] = ev.ms(0, 1);
  g_last_ms[1] = ms3[0] + ms3[1] + ms3[2];
  g_last_ms[2] = ev.ms(3, 4);
  g_last_ms[3] = ev.ms(1, 2) + ev.ms(4, 5);
  if (gsize[0] + gsize[1] + gsize[2] == 0)
    fail("bed_plinkQC: every sample has more than mind = %g of its genotypes missing; none is left.", mind);
  if (hwe_thr > 0.0 && gsize[0] == 0)
    fail("bed_plinkQC: no remaining sample is counted for the Hardy-Weinberg test (hwe = %g); set hwe = 0 to skip it.", hwe_thr);
  if (maf > 0.0 && gsize[0] + gsize[1] == 0) fail("bed_plinkQC: no remaining sample is a founder (maf = %g); set maf = 0 to skip it.", maf);
}

}  // namespace
}  // namespace bsn

extern "C" {

int bsn_hwe(const int32_t *counts, int64_t m, int midp, double *p_out) {
  return bsn::guarded([&] { bsn::hwe_host(counts, m, midp, 0, p_out, nullptr); });
}

int bsn_hwe_lanes(const int32_t *counts, int64_t m, int midp, int lanes, double *p_out, double *ms_out) {
  return bsn::guarded([&] { bsn::hwe_host(counts, m, midp, lanes, p_out, ms_out); });
}

int bsn_bed_hwe(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, int midp, double *p_out,
                int32_t *counts_out) {
  return bsn::guarded([&] { bsn::bed_hwe(bed, ind_row, n, ind_col, m, midp, p_out, counts_out); });
}

int bsn_bed_qc(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const int32_t *cls, double maf,
               double geno, double mind, double hwe, int midp, uint8_t *keep_row, uint8_t *keep_col, double *row_miss,
               double *col_stats) {
  return bsn::guarded(
      [&] { bsn::bed_qc(bed, ind_row, n, ind_col, m, cls, maf, geno, mind, hwe, midp, keep_row, keep_col, row_miss, col_stats); });
}

int bsn_qc_last_ms(double *ms_out) {
  return bsn::guarded([&] {
    for (int k = 0; k < 4; k++) ms_out[k] = bsn::g_last_ms[k];
  });
}

}  // extern "C"
