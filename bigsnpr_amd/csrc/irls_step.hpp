// irls_step.hpp — what one iteration of big_univLogReg's per-variant fit computes apart from the sums over the samples:
// the per-sample map eta -> (w, w z), the linear predictor, the packed Cholesky solve of the weighted normal equations
// with the [0, 0] entry of their inverse, and the convergence rule.  Shared by the kernel (gwas.hip) and by the CPU
// statement (tests/native/gwas_ref.cpp): the two cannot drift apart.
//
// The model of a variant is y ~ x + 1 + covar, columns in that order (P = q + 2); the null model drops x.  One iteration
// solves (C' W C) beta = C' W z with w = p (1 - p), z = eta + (y - p) / w.  Only the product w z is ever formed,
//     w z = w eta + (y - p),
// so nothing divides by a weight that underflows (|eta| beyond about 36 for a separated variant).
//
// exp is gibbs_step.hpp's (+ - * / only, every operation rounded on its own), so host and device map the same eta to
// the same bits; what differs between them is the order of the sums over the samples, nothing else.
#pragma once
#include "gibbs_step.hpp"

#if defined(__HIPCC__)
#define BSN_IRLS_HD __host__ __device__ inline
#else
#define BSN_IRLS_HD inline
#endif

namespace bsn {
namespace irls {

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

constexpr int kMaxP = 32;             // columns of a variant's model: the variant, the intercept, at most 30 covariates
constexpr double kPivotTol = 1e-14;   // a Cholesky pivot at or below this times its diagonal entry: singular
constexpr int kNullMaxIter = 100;     // the covariates-only fit: run to convergence at kNullTol
constexpr double kNullTol = 1e-10;

BSN_IRLS_HD double qnan() { return gibbs::from_bits(0x7ff8000000000000ull); }

// index of (i, j), i <= j, in an upper triangle packed by columns
BSN_IRLS_HD int packed(int i, int j) { return j * (j + 1) / 2 + i; }

// eta = beta[0] x + sum_c beta[xoff + c] row[c]: row = (1, covar_1 .. covar_q), xoff = 1 with the variant, 0 without
BSN_IRLS_HD double eta_of(const double *beta, bool has_x, double x, const double *row, int q1) {
  double e = has_x ? beta[0] * x : 0.0;
  const double *b = beta + (has_x ? 1 : 0);
  for (int c = 0; c < q1; c++) e = e + b[c] * row[c];
  return e;
}

// y is 0 or 1.  p and 1 - p are formed from exp(-|eta|), so neither loses its digits in a tail.
BSN_IRLS_HD void sample_map(double eta, double y, double &w, double &wz) {
  const double e = gibbs::exp_det(eta < 0 ? eta : -eta);
  const double d = 1.0 + e;
  const double big = 1.0 / d, small = e / d;          // max(p, 1 - p), min(p, 1 - p)
  const double p = eta < 0 ? small : big, omp = eta < 0 ? big : small;
  w = big * small;
  wz = w * eta + (y > 0.5 ? omp : -p);
}

// H (P x P, upper triangle packed by columns) = U' U in place; false when a pivot is at or below kPivotTol times its
// diagonal entry (or is not a number)
BSN_IRLS_HD bool chol_packed(double *H, int P) {
  for (int j = 0; j < P; j++) {
    double *cj = H + packed(0, j);
    for (int i = 0; i < j; i++) {
      const double *ci = H + packed(0, i);
      double s = cj[i];
      for (int k = 0; k < i; k++) s = s - ci[k] * cj[k];
      cj[i] = s / ci[i];
    }
    const double diag = cj[j];
    double s = diag;
    for (int k = 0; k < j; k++) s = s - cj[k] * cj[k];
    if (!(s > kPivotTol * diag)) return false;
    cj[j] = gibbs::sqrt_rn(s);
  }
  return true;
}

// beta = H^-1 rhs from the factor, and (H^-1)[0, 0] = |U^-T e_0|^2; work: P doubles
BSN_IRLS_HD double solve_packed(const double *U, int P, const double *rhs, double *beta, double *work) {
  for (int j = 0; j < P; j++) {          // U' v = rhs, U' t = e_0
    const double *cj = U + packed(0, j);
    double s = rhs[j], t = j == 0 ? 1.0 : 0.0;
    for (int k = 0; k < j; k++) {
      s = s - cj[k] * beta[k];
      t = t - cj[k] * work[k];
    }
    beta[j] = s / cj[j];
    work[j] = t / cj[j];
  }
  double inv00 = 0.0;
  for (int j = 0; j < P; j++) inv00 = inv00 + work[j] * work[j];
  for (int j = P - 1; j >= 0; j--) {     // U beta = v
    double s = beta[j];
    for (int k = j + 1; k < P; k++) s = s - U[packed(j, k)] * beta[k];
    beta[j] = s / U[packed(j, j)];
  }
  return inv00;
}

// max_k 2 |new - old| / (|new| + |old|) <= tol; a coefficient that is 0 before and after has not moved
BSN_IRLS_HD bool converged(const double *bnew, const double *bold, int P, double tol) {
  double worst = 0.0;
  for (int k = 0; k < P; k++) {
    const double a = bnew[k] < 0 ? -bnew[k] : bnew[k], b = bold[k] < 0 ? -bold[k] : bold[k];
    const double diff = bnew[k] - bold[k], den = a + b;
    const double r = den > 0 ? 2.0 * (diff < 0 ? -diff : diff) / den : (den == 0 ? 0.0 : qnan());
    if (r != r) return false;
    if (r > worst) worst = r;
  }
  return worst <= tol;
}

// One solve.  G: the (P + 1) x (P + 1) upper triangle packed by columns of [C | z]' W [C | z] — H in its first P
// columns, C' W z in the last (G is overwritten).  beta: in the previous iterate, out the new one.  Returns 0 = go on,
// 1 = converged, -1 = singular (beta untouched).  *inv00 = (H^-1)[0, 0] of this solve.  work: 2 P doubles.
BSN_IRLS_HD int solve_step(double *G, int P, double *beta, double tol, double *inv00, double *work) {
  if (!chol_packed(G, P)) return -1;
  double *bnew = work + P;
  *inv00 = solve_packed(G, P, G + packed(0, P), bnew, work);
  const bool conv = converged(bnew, beta, P, tol);
  for (int k = 0; k < P; k++) beta[k] = bnew[k];
  return conv ? 1 : 0;
}

#if defined(__clang__)
#pragma clang fp contract(on)
#endif

}  // namespace irls
}  // namespace bsn
