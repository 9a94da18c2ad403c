// ibd_ref.cpp — the CPU statement of bed_ibd: plain loops over decoded genotypes, the moments, their order of summation and
// the estimate through ibd_step.hpp (the header the kernels of bigsnpr_amd/csrc/ibd.hip use).  Built by ibd_ref.py with
// -ffp-contract=off -fopenmp.
#include <stdint.h>

#include <cstddef>
#include <vector>

#include "ibd_step.hpp"

using namespace bsn::ibd;

extern "C" {

// the five terms of every variant from its counts (counts[3 j ..] = n0, n1, n2): a[5 j ..], used[j]
void ibd_terms(const int64_t *counts, int64_t m, double *a, uint8_t *used) {
  for (int64_t j = 0; j < m; j++) used[j] = terms(counts[3 * j], counts[3 * j + 1], counts[3 * j + 2], a + 5 * j) ? 1 : 0;
}

// G: n x m row-major codes (0, 1, 2 = allele count, 3 = missing); freq[i] != 0: sample i counts for the allele frequencies.
// E[5] and *n_used in the header's order: leaves of kLeaf variants summed ascending, then the leaves ascending.
void ibd_moments(const int8_t *G, int64_t n, int64_t m, const uint8_t *freq, double *E, int64_t *n_used) {
  double top[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  int64_t used = 0;
  for (int64_t j0 = 0; j0 < m; j0 += kLeaf) {
    double leaf[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t j = j0; j < j0 + kLeaf; j++) {   // (a leaf past m adds zeros, as the kernel's idle threads do)
      double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      if (j < m) {
        int64_t c[4] = {0, 0, 0, 0};
        for (int64_t i = 0; i < n; i++)
          if (freq[i]) c[G[i * m + j]]++;
        if (terms(c[0], c[1], c[2], a)) used++;
      }
      for (int k = 0; k < 5; k++) leaf[k] += a[k];
    }
    for (int k = 0; k < 5; k++) top[k] += leaf[k];
  }
  const Moments M = means(top, used);
  E[0] = M.e00;
  E[1] = M.e01;
  E[2] = M.e02;
  E[3] = M.e11;
  E[4] = M.e12;
  *n_used = used;
}

// Every pair i < j in the order (i, j): row k of the table at ibs[3 k ..] (IBS0, IBS1, IBS2), est[5 k ..] (Z0, Z1, Z2,
// PI_HAT, DST), i1[k], i2[k].  fired[kBranches]: how often each branch of the estimate fired.
void ibd_table(const int8_t *G, int64_t n, int64_t m, const double *E, int32_t *i1, int32_t *i2, int32_t *ibs, double *est,
               int64_t *fired) {
  const Moments M = {E[0], E[1], E[2], E[3], E[4]};
  int64_t f[kBranches] = {0, 0, 0, 0, 0, 0, 0};
  std::vector<int64_t> first((std::size_t)n);   // row of the pair (i, i + 1)
  int64_t at = 0;
  for (int64_t i = 0; i < n; i++) {
    first[(std::size_t)i] = at;
    at += n - 1 - i;
  }
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : f[:kBranches])
  for (int64_t i = 0; i < n; i++) {
    const int8_t *gi = G + i * m;
    for (int64_t j = i + 1; j < n; j++) {
      const int64_t k = first[(std::size_t)i] + (j - i - 1);
      const int8_t *gj = G + j * m;
      int64_t c[3] = {0, 0, 0};   // by |a - b|: IBS2, IBS1, IBS0
      for (int64_t v = 0; v < m; v++) {
        const int a = gi[v], b = gj[v];
        if (a == 3 || b == 3) continue;
        c[a > b ? a - b : b - a]++;
      }
      const Estimate e = estimate(c[2], c[1], c[0], M, f);
      i1[k] = (int32_t)i;
      i2[k] = (int32_t)j;
      ibs[3 * k] = (int32_t)c[2];
      ibs[3 * k + 1] = (int32_t)c[1];
      ibs[3 * k + 2] = (int32_t)c[0];
      est[5 * k] = e.z0;
      est[5 * k + 1] = e.z1;
      est[5 * k + 2] = e.z2;
      est[5 * k + 3] = e.pi_hat;
      est[5 * k + 4] = e.dst;
    }
  }
  for (int q = 0; q < kBranches; q++) fired[q] = f[q];
}

// the estimate of the header over columns of counts (no branch counts)
void ibd_estimate(const int64_t *ibs, int64_t count, const double *E, double *est) {
  const Moments M = {E[0], E[1], E[2], E[3], E[4]};
  for (int64_t k = 0; k < count; k++) {
    const Estimate e = estimate(ibs[3 * k], ibs[3 * k + 1], ibs[3 * k + 2], M);
    est[5 * k] = e.z0;
    est[5 * k + 1] = e.z1;
    est[5 * k + 2] = e.z2;
    est[5 * k + 3] = e.pi_hat;
    est[5 * k + 4] = e.dst;
  }
}

// the filter of the header over a PI_HAT column: keep[k] = 1 where the row passes
void ibd_filter(const double *pi_hat, int64_t count, double min_pi_hat, uint8_t *keep) {
  for (int64_t k = 0; k < count; k++) keep[k] = passes(pi_hat[k], min_pi_hat) ? 1 : 0;
}

}  // extern "C"
