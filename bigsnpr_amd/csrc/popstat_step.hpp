// popstat_step.hpp — the two population statistics that are evaluated from per-group genotype counts: the Weir–Cockerham
// Fst of snp_fst (R/Fst.R:57-84 of the reference) and the MAX3 / MAXL / Armitage trend statistic of snp_MAX3
// (R/MAX3.R:3-28,95-103).  Shared by the kernels (popstat.hip) and the CPU statement (tests/native/popstat_ref.cpp): the
// two cannot drift apart.  DESIGN.md 3.5k.
//
// Bit equality of host and device.  Everything below is + - * / sqrt on doubles, each correctly rounded on both sides and
// never contracted into a fused multiply-add (the pragma below on the device, -ffp-contract=off on the host), in the order
// written here.  The sums over populations run in list order, the sums over variants of `overall` in the order of
// kBlock / tree_sum / the block index: no atomics, no launch geometry enters a result.
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#define BSN_POPSTAT_HD __host__ __device__ __forceinline__
#else
#define BSN_POPSTAT_HD inline
#endif

namespace bsn {
namespace popstat {

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// bed_MAF (R/binom-scaling.R:203-222): ac / (2 * nb_nona) with ac = n1 + 2 n2; N = group size - missing.  N == 0: NaN.
BSN_POPSTAT_HD double af_from_counts(int64_t c1, int64_t c2, int64_t N) { return (double)(c1 + 2 * c2) / (2.0 * (double)N); }

// ---- Fst of one variant ---------------------------------------------------------------------------------------------------
// af[p * stride], N[p * stride] for the populations p = 0 .. r - 1.  a: the numerator term, abc: a + b + c, keep: p_bar
// lies strictly inside (min_maf, 1 - min_maf) — false for a NaN p_bar (an empty population, a variant without any call).
struct FstTerms {
  double a, abc;
  bool keep;
};

BSN_POPSTAT_HD FstTerms fst_terms(const double *af, const double *N, int64_t r, int64_t stride, double min_maf) {
  const double rr = (double)r;
  double n_sum = N[0];
  for (int64_t p = 1; p < r; p++) n_sum = n_sum + N[p * stride];
  const double n_bar = n_sum / rr;
  double n_sqsum = N[0] * N[0];
  for (int64_t p = 1; p < r; p++) n_sqsum = n_sqsum + N[p * stride] * N[p * stride];
  const double n_c = (n_sum - n_sqsum / n_sum) / (rr - 1.0);

  double af_n_sum = af[0] * N[0];
  for (int64_t p = 1; p < r; p++) af_n_sum = af_n_sum + af[p * stride] * N[p * stride];
  const double p_bar = af_n_sum / n_sum;

  double diff_af_n_sum = 0.0;
  for (int64_t p = 0; p < r; p++) {
    const double d = af[p * stride] - p_bar;
    const double t = (d * d) * N[p * stride];
    diff_af_n_sum = p == 0 ? t : diff_af_n_sum + t;
  }
  const double s2 = diff_af_n_sum / n_bar / (rr - 1.0);

  double h_n_sum = 0.0;
  for (int64_t p = 0; p < r; p++) {
    const double f = af[p * stride];
    const double t = ((2.0 * f) * (1.0 - f)) * N[p * stride];
    h_n_sum = p == 0 ? t : h_n_sum + t;
  }
  const double h_bar = h_n_sum / n_sum;

  const double pq = p_bar * (1.0 - p_bar);
  const double rs2 = ((rr - 1.0) / rr) * s2;
  const double a = (n_bar / n_c) * (s2 - (1.0 / (n_bar - 1.0)) * ((pq - rs2) - h_bar / 4.0));
  const double b = (n_bar / (n_bar - 1.0)) * ((pq - rs2) - ((2.0 * n_bar - 1.0) / (4.0 * n_bar)) * h_bar);
  const double c = h_bar / 2.0;

  FstTerms t;
  t.a = a;
  t.abc = (a + b) + c;
  t.keep = p_bar > min_maf && p_bar < (1.0 - min_maf);
  return t;
}

// ---- the sums of `overall = TRUE` ---------------------------------------------------------------------------------------
// The variants are cut into blocks of kBlock; a block's terms (0 for a variant that is not kept or past the end) are summed
// by tree_sum, and the block sums are added in index order from 0.0.  tree_sum is what 256 threads do in log2(256) steps:
// at distance s = 128, 64, ... 1, element i < s receives element i + s.
constexpr int kBlock = 256;

inline double tree_sum(double *t /* kBlock values, overwritten */) {
  for (int s = kBlock / 2; s > 0; s >>= 1)
    for (int i = 0; i < s; i++) t[i] = t[i] + t[i + s];
  return t[0];
}

// ---- MAX3 of one variant ------------------------------------------------------------------------------------------------
// r0, r1, r2: the cases with 0, 1, 2 alleles; s0, s1, s2: the controls.  For every x of val the trend statistic with
// scores (0, x, 1); a NaN statistic counts as 0 (R/MAX3.R:96); the result is the largest square.
BSN_POPSTAT_HD double max3_score(int64_t r0, int64_t r1, int64_t r2, int64_t s0, int64_t s1, int64_t s2, const double *val,
                                 int64_t L) {
  const double rj[3] = {(double)r0, (double)r1, (double)r2}, sj[3] = {(double)s0, (double)s1, (double)s2};
  const double r = (rj[0] + rj[1]) + rj[2], s = (sj[0] + sj[1]) + sj[2];
  const double n = r + s;
  const double phi = r / n;
  double num[3], pj[3];
  for (int j = 0; j < 3; j++) {
    num[j] = rj[j] * (1.0 - phi) - sj[j] * phi;
    pj[j] = (rj[j] + sj[j]) / n;
  }
  const double coef = (n * phi) * (1.0 - phi);
  double best = 0.0;
  for (int64_t l = 0; l < L; l++) {
    const double x2[3] = {0.0, val[l], 1.0};
    const double num2 = (x2[0] * num[0] + x2[1] * num[1]) + x2[2] * num[2];
    const double m2 = ((x2[0] * x2[0]) * pj[0] + (x2[1] * x2[1]) * pj[1]) + (x2[2] * x2[2]) * pj[2];
    const double m1 = (x2[0] * pj[0] + x2[1] * pj[1]) + x2[2] * pj[2];
    const double deno = m2 - m1 * m1;
    const double deno2 = sqrt(coef * deno);
    double z = num2 / deno2;
    if (z != z) z = 0.0;
    const double z2 = z * z;
    if (z2 > best) best = z2;
  }
  return best;
}

#if defined(__clang__)
#pragma clang fp contract(on)
#endif

}  // namespace popstat
}  // namespace bsn
