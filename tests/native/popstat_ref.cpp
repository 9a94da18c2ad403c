// popstat_ref.cpp — the CPU statement of snp_fst and snp_MAX3 over bigsnpr_amd/csrc/popstat_step.hpp: the per-variant
// terms of the header the kernels compile from, and the reduction of `overall = TRUE` in the order the header defines
// (blocks of kBlock variants summed by tree_sum, block sums added in index order).  Built by popstat_ref.py with
// -ffp-contract=off.
#include <stdint.h>

#include <cmath>
#include <limits>

#include "popstat_step.hpp"

using namespace bsn::popstat;

extern "C" {

double popstat_af(int64_t c1, int64_t c2, int64_t N) { return af_from_counts(c1, c2, N); }

// af, N: r x m, population p's vector at p * m.  a, abc, keep (m each, may be NULL): the terms.  fst (m, may be NULL): NaN
// where not kept.  overall (3, may be NULL): ratio, numerator, denominator.
void popstat_fst(const double *af, const double *N, int64_t r, int64_t m, double min_maf, double *a, double *abc,
                 int32_t *keep, double *fst, double *overall) {
  double num = 0.0, den = 0.0;
  for (int64_t j0 = 0; j0 < m; j0 += kBlock) {
    double ta[kBlock], tb[kBlock];
    for (int64_t k = 0; k < kBlock; k++) {
      const int64_t j = j0 + k;
      ta[k] = tb[k] = 0.0;
      if (j >= m) continue;
      const FstTerms t = fst_terms(af + j, N + j, r, m, min_maf);
      if (a) a[j] = t.a;
      if (abc) abc[j] = t.abc;
      if (keep) keep[j] = t.keep ? 1 : 0;
      if (fst) fst[j] = t.keep ? t.a / t.abc : std::numeric_limits<double>::quiet_NaN();
      if (t.keep) ta[k] = t.a, tb[k] = t.abc;
    }
    num = num + tree_sum(ta);
    den = den + tree_sum(tb);
  }
  if (overall) overall[0] = num / den, overall[1] = num, overall[2] = den;
}

// the reduction alone: the sum of m terms in the header's order
double popstat_block_sum(const double *x, int64_t m) {
  double s = 0.0;
  for (int64_t j0 = 0; j0 < m; j0 += kBlock) {
    double t[kBlock];
    for (int64_t k = 0; k < kBlock; k++) t[k] = j0 + k < m ? x[j0 + k] : 0.0;
    s = s + tree_sum(t);
  }
  return s;
}

// cases, controls: 3 x m (counts of 0, 1, 2 of variant j at 3 j)
void popstat_max3(const int64_t *cases, const int64_t *controls, int64_t m, const double *val, int64_t L, double *score) {
  for (int64_t j = 0; j < m; j++)
    score[j] = max3_score(cases[3 * j], cases[3 * j + 1], cases[3 * j + 2], controls[3 * j], controls[3 * j + 1],
                          controls[3 * j + 2], val, L);
}

}  // extern "C"
