// ibd_step.hpp — the method-of-moments IBD estimate of PLINK 1.9's --genome (bed_ibd / bed_ibdQC): the allele-frequency
// moments of one variant, the order in which they are summed, the estimate of one pair of samples from its IBS counts
// and the filter.  Shared by the kernels (ibd.hip) and the CPU statement (tests/native/ibd_ref.cpp): the two cannot drift
// apart.  DESIGN.md 3.5p holds the statement in full.
//
// Everything is plain IEEE double in the order written here, never contracted; no guard beyond those written here.  A
// pair without a variant where both samples are called (S = 0) is NaN in every column, by IEEE, and passes no filter.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BSN_IBD_HD __host__ __device__ __forceinline__
#else
#define BSN_IBD_HD inline
#endif

namespace bsn {
namespace ibd {

// Variants per leaf of the moment sums.  Within a leaf the terms are added one after the other, ascending; the leaves are
// then added one after the other, ascending.  Part of the statement: independent of grid size and CU count.
constexpr int kLeaf = 256;

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// the five means E00, E01, E02, E11, E12 of the terms below over the used variants: P(IBS = i | IBD = z)
struct Moments {
  double e00, e01, e02, e11, e12;
};

// The terms a00, a01, a02, a11, a12 of one variant from the counts n0, n1, n2 of its called genotypes among the frequency
// samples.  Returns whether the variant is used (more than 3 called alleles, both alleles seen); a[] is 0 otherwise.
BSN_IBD_HD bool terms(int64_t n0, int64_t n1, int64_t n2, double a[5]) {
  const double Na = (double)(2 * (n0 + n1 + n2));
  const double p = (double)(n1 + 2 * n2) / Na;
  const double q = 1.0 - p;
  if (!(Na > 3.0 && p > 0.0 && q > 0.0)) {
    for (int k = 0; k < 5; k++) a[k] = 0.0;
    return false;
  }
  const double f2 = Na * Na / ((Na - 1.0) * (Na - 2.0));
  const double f3 = f2 * Na / (Na - 3.0);
  const double x = p * Na, y = q * Na;
  const double x1 = (x - 1.0) / x, x2 = x1 * (x - 2.0) / x;
  const double y1 = (y - 1.0) / y, y2 = y1 * (y - 2.0) / y;
  const double p2 = p * p, q2 = q * q;
  a[0] = 2.0 * p2 * q2 * x1 * y1 * f3;
  a[1] = 4.0 * p * q * f3 * (p2 * x2 + q2 * y2);
  a[2] = f3 * (q2 * q2 * y2 * (y - 3.0) / y + p2 * p2 * x2 * (x - 3.0) / x + 4.0 * p2 * q2 * x1 * y1);
  a[3] = 2.0 * p * q * f2 * (p * x1 + q * y1);
  a[4] = f2 * (p2 * p * x2 + q2 * q * y2 + p2 * q * x1 + p * q2 * y1);
  return true;
}

// the mean of a sum over n_used variants
BSN_IBD_HD Moments means(const double sum[5], int64_t n_used) {
  const double d = (double)n_used;
  Moments E;
  E.e00 = sum[0] / d;
  E.e01 = sum[1] / d;
  E.e02 = sum[2] / d;
  E.e11 = sum[3] / d;
  E.e12 = sum[4] / d;
  return E;
}

struct Estimate {
  double z0, z1, z2, pi_hat, dst;
};

// which branch of the estimate fired (the CPU statement counts them; the kernels pass no pointer)
enum Branch { kZ0Gt1 = 0, kZ1Gt1, kZ2Gt1, kZ0Lt0, kZ1Lt0, kZ2Lt0, kBounded, kBranches };

BSN_IBD_HD Estimate estimate(int64_t ibs0, int64_t ibs1, int64_t ibs2, const Moments &E, int64_t *fired = nullptr) {
  const double S = (double)(ibs0 + ibs1 + ibs2);
  const double r = 1.0 / S;
  double z0 = (double)ibs0 * r / E.e00;
  double z1 = ((double)ibs1 * r - z0 * E.e01) / E.e11;
  double z2 = (double)ibs2 * r - z0 * E.e02 - z1 * E.e12;
  if (z0 > 1.0) {
    z0 = 1.0; z1 = 0.0; z2 = 0.0;
    if (fired) fired[kZ0Gt1]++;
  }
  if (z1 > 1.0) {
    z0 = 0.0; z1 = 1.0; z2 = 0.0;
    if (fired) fired[kZ1Gt1]++;
  }
  if (z2 > 1.0) {
    z0 = 0.0; z1 = 0.0; z2 = 1.0;
    if (fired) fired[kZ2Gt1]++;
  }
  if (z0 < 0.0) {
    const double s = z1 + z2;
    z1 /= s; z2 /= s; z0 = 0.0;
    if (fired) fired[kZ0Lt0]++;
  }
  if (z1 < 0.0) {
    const double s = z0 + z2;
    z0 /= s; z2 /= s; z1 = 0.0;
    if (fired) fired[kZ1Lt0]++;
  }
  if (z2 < 0.0) {
    const double s = z0 + z1;
    z0 /= s; z1 /= s; z2 = 0.0;
    if (fired) fired[kZ2Lt0]++;
  }
  const double pi = z1 * 0.5 + z2;
  if (pi * pi <= z2) {   // PLINK's default ("bounded"): the nearest point on the curve of outbred pairs
    z0 = (1.0 - pi) * (1.0 - pi);
    z1 = 2.0 * pi * (1.0 - pi);
    z2 = pi * pi;
    if (fired) fired[kBounded]++;
  }
  Estimate e;
  e.z0 = z0;
  e.z1 = z1;
  e.z2 = z2;
  e.pi_hat = pi;
  e.dst = ((double)ibs2 + 0.5 * (double)ibs1) * r;
  return e;
}

// a row of the filtered table: NaN fails every threshold
BSN_IBD_HD bool passes(double pi_hat, double min_pi_hat) { return pi_hat >= min_pi_hat; }

#if defined(__clang__)
#pragma clang fp contract(on)
#endif

}  // namespace ibd
}  // namespace bsn
