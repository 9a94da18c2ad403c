// popstat.hip — snp_fst and snp_MAX3 on the device (bsn_fst, bsn_bed_fst, bsn_snp_max3) and the C entry point of the grouped
// counting pass they read (bsn_bed_group_counts; the pass itself: counts_grouped in matvec.hip, its driver in api.hip).
//
// Replaces R/Fst.R:47-85 and R/MAX3.R:81-107 of the reference, which call big_counts / bed_MAF once per population — one
// pass over the genotype matrix each — and evaluate the statistics in R.  Here one pass counts every population, the
// 4 x G x m table stays on the device and only the m results (or the three numbers of `overall`) come back.  The
// formulas live in popstat_step.hpp, shared with the CPU statement.  DESIGN.md 3.5k.
#include <algorithm>
#include <vector>

#include "bsn_internal.hpp"
#include "popstat_step.hpp"

namespace bsn {
namespace {

// device milliseconds of the last call of this process (bsn_popstat_last_ms): the multiplicity and digit panels, the
// streaming launches, the finalising kernels, the statistic
double g_last_ms[4] = {0.0, 0.0, 0.0, 0.0};

// (no contraction in the sums below either: they are the header's order, spelled out for 256 threads)
#pragma clang fp contract(off)

// af, N (G x m, group g's vector at g * m) from the count table: what bed_MAF makes of each group's counts
__global__ void k_group_maf(const int32_t *__restrict__ table, int64_t m, int G, double *af, double *N) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m * G) return;
  const int64_t j = idx / G;
  const int g = (int)(idx - j * G);
  const int4 c = *(const int4 *)(table + 4 * idx);
  const int64_t nn = (int64_t)c.x + c.y + c.z;
  af[(int64_t)g * m + j] = popstat::af_from_counts(c.y, c.z, nn);
  N[(int64_t)g * m + j] = (double)nn;
}

// One variant per thread, popstat::kBlock variants per workgroup: fst[j] (may be NULL), and the workgroup's sums of a and
// of a + b + c over its kept variants in the order of popstat::tree_sum -> part[2 * block], part[2 * block + 1] (may be
// NULL).
__global__ __launch_bounds__(popstat::kBlock) void k_fst(const double *__restrict__ af, const double *__restrict__ N, int64_t r,
                                                         int64_t m, double min_maf, double *fst, double *part) {
  __shared__ double sa[popstat::kBlock], sb[popstat::kBlock];
  const int tid = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * popstat::kBlock + tid;
  double ta = 0.0, tb = 0.0;
  if (j < m) {
    const popstat::FstTerms t = popstat::fst_terms(af + j, N + j, r, m, min_maf);
    if (fst) fst[j] = t.keep ? t.a / t.abc : __longlong_as_double(0x7FF8000000000000LL);
    if (t.keep) ta = t.a, tb = t.abc;
  }
  if (!part) return;   // (uniform: a kernel argument)
  sa[tid] = ta;
  sb[tid] = tb;
  __syncthreads();
  for (int s = popstat::kBlock / 2; s > 0; s >>= 1) {
    if (tid < s) {
      sa[tid] = sa[tid] + sa[tid + s];
      sb[tid] = sb[tid] + sb[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[2 * (int64_t)blockIdx.x] = sa[0];
    part[2 * (int64_t)blockIdx.x + 1] = sb[0];
  }
}

// the block sums in index order: out = (ratio, numerator, denominator).  One thread: the order is the definition.
__global__ void k_fst_overall(const double *__restrict__ part, int64_t nblk, double *out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double num = 0.0, den = 0.0;
  for (int64_t b = 0; b < nblk; b++) {
    num = num + part[2 * b];
    den = den + part[2 * b + 1];
  }
  out[0] = num / den;
  out[1] = num;
  out[2] = den;
}

// table of two groups: 0 = controls, 1 = cases
__global__ void k_max3(const int32_t *__restrict__ table, int64_t m, const double *__restrict__ val, int L, double *score) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int4 s = *(const int4 *)(table + 8 * j), r = *(const int4 *)(table + 8 * j + 4);
  score[j] = popstat::max3_score(r.x, r.y, r.z, s.x, s.y, s.z, val, L);
}

#pragma clang fp contract(on)

void check_fst_args(int64_t r, double min_maf) {
  if (r < 2) fail("You should provide frequencies for at least 2 populations.");
  if (!(min_maf >= 0.0 && min_maf <= 0.45)) fail("Parameter 'min_maf' should be in range [0, 0.45].");
}

// d_af, d_N: r x m on the device -> the host results.  Queued on `st` behind `first` (a kernel that fills d_af and d_N, or
// nothing); returns the device ms of the kernels.
template <class F>
double fst_from_device(F first, const double *d_af, const double *d_N, int64_t r, int64_t m, double min_maf, double *fst,
                       double *overall, hipStream_t st) {
  const int64_t nblk = (m + popstat::kBlock - 1) / popstat::kBlock;
  DevBuf<double> d_fst, d_part, d_out;
  if (fst) d_fst.ensure((size_t)m);
  if (overall) d_part.ensure((size_t)2 * nblk), d_out.ensure(3);
  EventMarks<2> ev;
  ev.mark(0, st);
  first();
  hipLaunchKernelGGL(k_fst, dim3((unsigned)nblk), dim3(popstat::kBlock), 0, st, d_af, d_N, r, m, min_maf, fst ? d_fst.p : nullptr,
                     overall ? d_part.p : nullptr);
  BSN_HIP(hipGetLastError());
  if (overall) {
    hipLaunchKernelGGL(k_fst_overall, dim3(1), dim3(64), 0, st, d_part.p, nblk, d_out.p);
    BSN_HIP(hipGetLastError());
  }
  ev.mark(1, st);
  BSN_HIP(hipStreamSynchronize(st));
  if (fst) BSN_HIP(hipMemcpy(fst, d_fst.p, (size_t)m * 8, hipMemcpyDeviceToHost));
  if (overall) BSN_HIP(hipMemcpy(overall, d_out.p, 24, hipMemcpyDeviceToHost));
  return ev.ms(0, 1);
}

void fst_host(const double *af, const double *N, int64_t r, int64_t m, double min_maf, double *fst, double *overall) {
  require_gpu();
  check_fst_args(r, min_maf);
  if (m <= 0) fail("snp_fst: no variant");
  if (!af || !N) fail("snp_fst: no frequencies");
  if (!fst && !overall) return;
  DevBuf<double> d_af, d_N;
  BSN_HIP(hipMemcpy(d_af.ensure((size_t)r * m), af, (size_t)r * m * 8, hipMemcpyHostToDevice));
  BSN_HIP(hipMemcpy(d_N.ensure((size_t)r * m), N, (size_t)r * m * 8, hipMemcpyHostToDevice));
  for (double &v : g_last_ms) v = 0.0;
  g_last_ms[3] = fst_from_device([] {}, d_af.p, d_N.p, r, m, min_maf, fst, overall, nullptr);
}

void bed_fst(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int32_t *group, int32_t G, const int64_t *ind_col, int64_t m,
             double min_maf, double *fst, double *overall) {
  check_fst_args(G, min_maf);
  for (double &v : g_last_ms) v = 0.0;
  DevBuf<int32_t> d_table;
  group_counts_device(bed, ind_row, n, group, G, ind_col, m, d_table, g_last_ms);
  if (!fst && !overall) return;
  hipStream_t st = bed->stream;
  DevBuf<double> d_af, d_N;
  d_af.ensure((size_t)G * m);
  d_N.ensure((size_t)G * m);
  g_last_ms[3] = fst_from_device(
      [&] {
        hipLaunchKernelGGL(k_group_maf, dim3((unsigned)((m * G + 255) / 256)), dim3(256), 0, st, d_table.p, m, (int)G, d_af.p,
                           d_N.p);
        BSN_HIP(hipGetLastError());
      },
      d_af.p, d_N.p, G, m, min_maf, fst, overall, st);
}

void snp_max3(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int32_t *y01, const int64_t *ind_col, int64_t m,
              const double *val, int32_t L, double *score) {
  if (L < 1 || !val) fail("snp_MAX3: 'val' should hold at least one value.");
  if (!y01) fail("snp_MAX3: no phenotype");
  if (!score) fail("snp_MAX3: no result buffer");
  for (int64_t i = 0; i < n; i++)
    if (y01[i] != 0 && y01[i] != 1)
      fail("snp_MAX3: 'y01.train' should hold 0 (control) or 1 (case) only; row %lld holds %d.", (long long)i, (int)y01[i]);
  for (double &v : g_last_ms) v = 0.0;
  DevBuf<int32_t> d_table;
  group_counts_device(bed, ind_row, n, y01, 2, ind_col, m, d_table, g_last_ms);
  hipStream_t st = bed->stream;
  DevBuf<double> d_val, d_score;
  copy_h2d(bed, d_val.ensure((size_t)L), val, (size_t)L * 8);
  d_score.ensure((size_t)m);
  EventMarks<2> ev;
  ev.mark(0, st);
  hipLaunchKernelGGL(k_max3, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, d_table.p, m, d_val.p, (int)L, d_score.p);
  BSN_HIP(hipGetLastError());
  ev.mark(1, st);
  copy_d2h(bed, score, d_score.p, (size_t)m * 8);
  BSN_HIP(hipStreamSynchronize(st));
  g_last_ms[3] = ev.ms(0, 1);
}

}  // namespace
}  // namespace bsn

extern "C" {

int bsn_bed_group_counts(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int32_t *group, int32_t G, const int64_t *ind_col,
                         int64_t m, int32_t *res) {
  return bsn::guarded([&] {
    for (double &v : bsn::g_last_ms) v = 0.0;
    bsn::DevBuf<int32_t> d_table;
    bsn::group_counts_device(bed, ind_row, n, group, G, ind_col, m, d_table, bsn::g_last_ms);
    bsn::copy_d2h(bed, res, d_table.p, (size_t)4 * G * m * 4);
  });
}

int bsn_fst(const double *af, const double *N, int64_t r, int64_t m, double min_maf, double *fst, double *overall) {
  return bsn::guarded([&] { bsn::fst_host(af, N, r, m, min_maf, fst, overall); });
}

int bsn_bed_fst(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int32_t *group, int32_t G, const int64_t *ind_col,
                int64_t m, double min_maf, double *fst, double *overall) {
  return bsn::guarded([&] { bsn::bed_fst(bed, ind_row, n, group, G, ind_col, m, min_maf, fst, overall); });
}

int bsn_snp_max3(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int32_t *y01, const int64_t *ind_col, int64_t m,
                 const double *val, int32_t L, double *score) {
  return bsn::guarded([&] { bsn::snp_max3(bed, ind_row, n, y01, ind_col, m, val, L, score); });
}

int bsn_popstat_last_ms(double *ms_out) {
  return bsn::guarded([&] {
    for (int k = 0; k < 4; k++) ms_out[k] = bsn::g_last_ms[k];
  });
}

}  // extern "C"
