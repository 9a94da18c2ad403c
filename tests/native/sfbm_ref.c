/* CPU statement of the sparse symmetric product of tools/probe_sfbm.py: y = A x over full columns (CSC: p [m + 1], rows
 * i ascending in each column, values x), one column per loop iteration, OpenMP over the columns.  A is symmetric, so
 * column j of A is row j: y[j] = sum_e a[e] * v[i[e]]. */
#include <stdint.h>
#ifdef _OPENMP
#include <omp.h>
#endif

void sfbm_prodvec(const int64_t *p, const int32_t *i, const double *a, int64_t m, const double *v, double *y, int nthreads) {
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
#pragma omp parallel for schedule(dynamic, 256)
  for (int64_t j = 0; j < m; j++) {
    double s = 0;
    for (int64_t e = p[j]; e < p[j + 1]; e++) s += a[e] * v[i[e]];
    y[j] = s;
  }
}

/* sum of squares of every column (ld_scores_sfbm over all columns) */
void sfbm_colsumsq(const int64_t *p, const double *a, int64_t m, double *y, int nthreads) {
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
#pragma omp parallel for schedule(dynamic, 256)
  for (int64_t j = 0; j < m; j++) {
    double s = 0;
    for (int64_t e = p[j]; e < p[j + 1]; e++) s += a[e] * a[e];
    y[j] = s;
  }
}
