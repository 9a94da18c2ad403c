// gwas_ref.cpp — a CPU statement of big_univLinReg and big_univLogReg over a dense matrix of decoded genotypes (n x m
// doubles, column-major, NaN = missing), for the parity tests and the timing probe.
//
// The per-sample map, the linear predictor, the packed Cholesky solve and the convergence rule come from
// bigsnpr_amd/csrc/irls_step.hpp, the header the kernel is compiled from; this file adds the sums over the samples (in
// sample order) and the loop over the iterations.  Built with g++ -O2 -ffp-contract=off.  Variants run in parallel
// (OpenMP); each is one sequential computation, so the thread count changes no bit.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "irls_step.hpp"

using namespace bsn::irls;

// One fit.  x: the variant over the samples (NULL: the null model), rows: n x (q + 1) row-major (1, covar), beta: in the
// start, out the last iterate.  Returns niter as bsn_univ_logreg defines it (0: singular); *inv00 of the last solve.
static int fit(const double *x, const double *rows, const double *y, int64_t n, int q, double *beta, double tol, int maxiter,
               double *inv00) {
  const bool has_x = x != nullptr;
  const int q1 = q + 1, P = q1 + (has_x ? 1 : 0);
  std::vector<double> G((size_t)(P + 1) * (P + 2) / 2), c((size_t)P + 1), work((size_t)2 * P);
  for (int it = 1; it <= maxiter; it++) {
    std::fill(G.begin(), G.end(), 0.0);
    for (int64_t i = 0; i < n; i++) {
      const double *row = rows + i * q1;
      const double xi = has_x ? x[i] : 0.0;
      double w, wz;
      sample_map(eta_of(beta, has_x, xi, row, q1), y[i], w, wz);
      if (has_x) c[0] = xi;
      for (int k = 0; k < q1; k++) c[(size_t)k + (has_x ? 1 : 0)] = row[k];
      for (int j = 0; j < P; j++) {
        const double wc = w * c[(size_t)j];
        double *gj = G.data() + packed(0, j);
        for (int i2 = 0; i2 <= j; i2++) gj[i2] = gj[i2] + c[(size_t)i2] * wc;
      }
      double *gz = G.data() + packed(0, P);
      for (int i2 = 0; i2 < P; i2++) gz[i2] = gz[i2] + c[(size_t)i2] * wz;
    }
    const int st = solve_step(G.data(), P, beta, tol, inv00, work.data());
    if (st < 0) return 0;
    if (st == 1) return it;
  }
  return -1;
}

extern "C" {

// returns 0, or 1 when the covariates-only model is singular.  estim, se, niter: [m]
int gwas_logreg(const double *X, int64_t n, int64_t m, const double *y, const double *covar, int q, double tol, int maxiter,
                double *estim, double *se, int32_t *niter, int nthreads) {
  const int q1 = q + 1;
  std::vector<double> rows((size_t)n * q1), beta0((size_t)q1, 0.0);
  for (int64_t i = 0; i < n; i++) {
    rows[(size_t)(i * q1)] = 1.0;
    for (int k = 0; k < q; k++) rows[(size_t)(i * q1 + 1 + k)] = covar[i + (int64_t)k * n];
  }
  double inv00 = 0.0;
  if (fit(nullptr, rows.data(), y, n, q, beta0.data(), kNullTol, kNullMaxIter, &inv00) == 0) return 1;
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t j = 0; j < m; j++) {
    const double *x = X + j * n;
    bool na = false, varies = false;
    for (int64_t i = 0; i < n; i++) {
      na |= x[i] != x[i];
      varies |= x[i] != x[0];
    }
    double beta[kMaxP], i00 = 0.0;
    int it = 0;
    if (!na && varies) {
      beta[0] = 0.0;
      for (int k = 0; k < q1; k++) beta[k + 1] = beta0[(size_t)k];
      it = fit(x, rows.data(), y, n, q, beta, tol, maxiter, &i00);
    }
    niter[j] = it;
    estim[j] = it == 0 ? qnan() : beta[0];
    se[j] = it == 0 ? qnan() : sqrt(i00);
  }
  return 0;
}

// U: n x K column-major, orthonormal
void gwas_linreg(const double *X, int64_t n, int64_t m, const double *y, const double *U, int K, double *estim, double *se,
                 int nthreads) {
  std::vector<double> yt((size_t)n), c((size_t)K, 0.0);
  for (int k = 0; k < K; k++)
    for (int64_t i = 0; i < n; i++) c[(size_t)k] += U[i + (int64_t)k * n] * y[i];
  double yy = 0.0;
  for (int64_t i = 0; i < n; i++) {
    double r = y[i];
    for (int k = 0; k < K; k++) r -= U[i + (int64_t)k * n] * c[(size_t)k];
    yt[(size_t)i] = r;
    yy += r * r;
  }
  const double df = (double)(n - K - 1);
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
#pragma omp parallel for schedule(static)
  for (int64_t j = 0; j < m; j++) {
    const double *x = X + j * n;
    bool na = false, varies = false;
    double num = 0.0, xx = 0.0, proj = 0.0;
    for (int64_t i = 0; i < n; i++) {
      na |= x[i] != x[i];
      varies |= x[i] != x[0];
      num += x[i] * yt[(size_t)i];
      xx += x[i] * x[i];
    }
    for (int k = 0; k < K; k++) {
      double t = 0.0;
      for (int64_t i = 0; i < n; i++) t += U[i + (int64_t)k * n] * x[i];
      proj += t * t;
    }
    const double den = xx - proj;
    if (na || !varies || !(den > kPivotTol * xx)) {
      estim[j] = se[j] = qnan();
      continue;
    }
    estim[j] = num / den;
    se[j] = sqrt((yy - estim[j] * num) / (den * df));
  }
}

// irls_step.hpp's sample_map on its own (in: eta, y; out: w, w z)
void gwas_sample_map(const double *eta, const double *y, int64_t len, double *w, double *wz) {
  for (int64_t i = 0; i < len; i++) sample_map(eta[i], y[i], w[i], wz[i]);
}

}  // extern "C"
