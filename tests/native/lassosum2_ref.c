/* lassosum2_ref.c — a CPU statement of lassosum2's coordinate descent (src/lassosum2.cpp:8-70 of the reference) and of
 * the column update it leans on (bigsparser's SFBM::incr_mult_col), for the parity tests and the timing probe.
 *
 * The matrix is a CSC with full columns: p [m2 + 1] int64 offsets, rows r [p[m2]] int32, values x [p[m2]].
 * Built with -O2 -ffp-contract=off: every product and sum is rounded on its own, in the order written here.
 * ls2_grid runs the grid points in parallel (OpenMP, one grid point per thread at a time); each grid point is one
 * sequential sweep loop, so the thread count changes no bit of the result. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static double shrink(double z, double l1, double denom) {
  double t;
  if (z > 0) {
    t = z - l1;
    if (t > 0) return t / denom;
    return 0;
  }
  t = z + l1;
  if (t < 0) return t / denom;
  return 0;
}

/* one grid point: pen [m] and den [m] are the per-variant L1 weight and 1 + L2 weight.  Returns the number of sweeps
 * (the reference's k + 1); *moves counts the coordinate steps with a non-zero shift. */
int ls2_one(const int64_t *p, const int32_t *r, const double *x, int64_t m2, const double *bhat, int64_t m,
            const double *pen, const double *den, const int64_t *sub, double dfmax, int maxiter, double tol,
            double *beta, int64_t *moves) {
  double *dp = calloc((size_t)(m2 > 0 ? m2 : 1), sizeof(double));
  double bound = 0.0, sumsq = 0.0;
  int64_t nmove = 0;
  int it, bad = 0;
  for (int64_t j = 0; j < m; j++) beta[j] = 0.0;
  for (int64_t j = 0; j < m; j++) sumsq = sumsq + bhat[j] * bhat[j];
  bound = 2 * sumsq;
  for (it = 0; it < maxiter; it++) {
    int stable = 1;
    double nonzero = 0, norm2 = 0;
    for (int64_t j = 0; j < m; j++) {
      const int64_t col = sub ? sub[j] : j;
      const double resid = bhat[j] - (dp[col] - beta[j]);
      const double b = shrink(resid, pen[j], den[j]);
      double step;
      if (b != 0) {
        norm2 += b * b;
        nonzero++;
      }
      step = b - beta[j];
      if (step != 0) {
        if (stable && fabs(step) > tol) stable = 0;
        beta[j] = b;
        for (int64_t e = p[col]; e < p[col + 1]; e++) dp[r[e]] += x[e] * step;
        nmove++;
      }
    }
    if (norm2 > bound) {
      bad = 1;
      break;
    }
    if (stable || nonzero > dfmax) break;
  }
  if (bad)
    for (int64_t j = 0; j < m; j++) beta[j] = NAN;
  free(dp);
  if (moves) *moves = nmove;
  return it + 1;
}

/* G grid points: pen_j = pf[j] * lambda[g], den_j = pf[j] * delta[g] + 1 (R/lassosum2.R:59-60); beta [m * G]
 * column-major; secs [g] (may be NULL) the wall time of each grid point */
#ifdef _OPENMP
#include <omp.h>
#endif
void ls2_grid(const int64_t *p, const int32_t *r, const double *x, int64_t m2, const double *bhat, int64_t m,
              const double *pf, const double *lambda, const double *delta, int64_t G, const int64_t *sub, double dfmax,
              int maxiter, double tol, double *beta, int32_t *iters, int64_t *moves, double *secs, int nthreads) {
  int64_t g;
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic, 1)
#endif
  for (g = 0; g < G; g++) {
    double *pen = malloc((size_t)(m > 0 ? m : 1) * sizeof(double));
    double *den = malloc((size_t)(m > 0 ? m : 1) * sizeof(double));
#ifdef _OPENMP
    const double t0 = omp_get_wtime();
#endif
    for (int64_t j = 0; j < m; j++) {
      pen[j] = pf[j] * lambda[g];
      den[j] = pf[j] * delta[g] + 1;
    }
    iters[g] = ls2_one(p, r, x, m2, bhat, m, pen, den, sub, dfmax, maxiter, tol, beta + g * m, moves ? moves + g : NULL);
#ifdef _OPENMP
    if (secs) secs[g] = omp_get_wtime() - t0;
#else
    if (secs) secs[g] = NAN;
#endif
    free(pen);
    free(den);
  }
}
