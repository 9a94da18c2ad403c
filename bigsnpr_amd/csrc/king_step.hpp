// king_step.hpp — one pair of samples of the KING-robust kinship table (bed_king / bed_kingQC): the five counts of PLINK 2's
// --make-king-table from the pairwise-complete plane sums the kernel holds, the between-family estimator of Manichaikul
// et al. 2010 and the filter.  Shared by the kernels (king.hip) and the CPU statement (tests/native/king_ref.cpp): the two
// cannot drift apart.  DESIGN.md 3.5n.
//
// x in {0, 1, 2} is a called genotype, P "called", H = 2 x - x^2 "heterozygous"; every sum runs over the selected variants
// where BOTH samples are called.  (x_i - x_j)^2 is 4 for opposite homozygotes, 1 for het against hom and 0 otherwise, so
//   sum (x_i - x_j)^2 = sum x_i^2 P_j + sum P_i x_j^2 - 2 sum x_i x_j = 4 IBS0 + HET1HOM2 + HET2HOM1
//   sum H_i P_j       = 2 sum x_i P_j - sum x_i^2 P_j                 = HETHET + HET1HOM2.
// All of it is integer arithmetic; the kinship is ONE division and ONE subtraction in IEEE double, never contracted.  A
// zero denominator stays what IEEE makes of it (NaN for 0 / 0, -inf otherwise) and passes no filter.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BSN_KING_HD __host__ __device__ __forceinline__
#else
#define BSN_KING_HD inline
#endif

namespace bsn {
namespace king {

// int32 accumulation of the plane products is exact while 4 m < 2^31
constexpr int64_t kMaxVariants = ((int64_t)1 << 29) - 1;

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// the plane sums of the pair (i, j): xx = sum x_i x_j, hh = sum H_i H_j, xP / x2P = sum x_i P_j / sum x_i^2 P_j (sample i's
// values over sample j's calls), Px / Px2 the same with the roles swapped, PP = variants where both are called
struct Sums {
  int64_t xx, hh, xP, x2P, Px, Px2, PP;
};

struct Pair {
  int32_t nsnp, hethet, ibs0, het1hom2, het2hom1;
  double kinship;
};

BSN_KING_HD double kinship(int64_t hethet, int64_t ibs0, int64_t het1hom2, int64_t het2hom1) {
  const int64_t lo = het1hom2 < het2hom1 ? het1hom2 : het2hom1;
  return 0.5 - (double)(4 * ibs0 + het1hom2 + het2hom1) / (4.0 * (double)(hethet + lo));
}

BSN_KING_HD Pair pair_from_sums(const Sums &s) {
  const int64_t het1 = 2 * s.xP - s.x2P, het2 = 2 * s.Px - s.Px2;   // heterozygous calls of i / of j among the shared variants
  const int64_t h1 = het1 - s.hh, h2 = het2 - s.hh;
  const int64_t d2 = s.x2P + s.Px2 - 2 * s.xx;
  const int64_t ibs0 = (d2 - h1 - h2) / 4;
  Pair p;
  p.nsnp = (int32_t)s.PP;
  p.hethet = (int32_t)s.hh;
  p.ibs0 = (int32_t)ibs0;
  p.het1hom2 = (int32_t)h1;
  p.het2hom1 = (int32_t)h2;
  p.kinship = kinship(s.hh, ibs0, h1, h2);
  return p;
}

// a row of the filtered table: NaN and -inf fail every threshold
BSN_KING_HD bool passes(double kin, double thr) { return kin >= thr; }

#if defined(__clang__)
#pragma clang fp contract(on)
#endif

}  // namespace king
}  // namespace bsn
