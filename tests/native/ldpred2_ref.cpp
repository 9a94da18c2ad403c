// ldpred2_ref.cpp — a CPU statement of LDpred2-grid's Gibbs sampler (src/ldpred2.cpp:9-69 and
// src/ldpred2-sampling.cpp:9-59 of the reference) over full CSC columns, for the parity tests and the timing probe.
//
// The per-coordinate arithmetic and the two random numbers come from bigsnpr_amd/csrc/gibbs_step.hpp, the header the
// kernel is compiled from; this file adds the two sequential loops around it.  Built with g++ -O2 -ffp-contract=off:
// every product and sum is rounded on its own, in the order written.  Chains run in parallel (OpenMP, one chain per
// thread at a time); each is one sequential loop, so the thread count changes no bit.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "gibbs_step.hpp"

using namespace bsn::gibbs;

// one chain.  SAMPLING: out is sample_beta [m x num_iter], else avg_beta / num_iter [m] (all NaN on divergence).
template <bool SAMPLING>
static void chain(const int64_t *P, const int32_t *I, const double *X, int64_t m2, const double *beta_hat, const double *n_vec,
                  int64_t m, const int64_t *sub, double h2, double p, bool sparse, uint64_t stream, int burn_in, int num_iter,
                  uint64_t seed, double *out, int64_t *moves) {
  std::vector<double> curr((size_t)m, 0.0), dotprods((size_t)m2, 0.0);
  if (SAMPLING)
    for (int64_t t = 0; t < m * num_iter; t++) out[t] = 0.0;
  else
    for (int64_t j = 0; j < m; j++) out[j] = 0.0;
  const double h2_per_var = h2 / (m * p);
  const double inv_odd_p = (1 - p) / p;
  double ss = 0.0;
  for (int64_t j = 0; j < m; j++) ss = ss + beta_hat[j] * beta_hat[j];
  const double gap0 = 2 * ss;
  int64_t nmove = 0;
  for (int k = -burn_in; k < num_iter; k++) {
    double gap = 0;
    for (int64_t j = 0; j < m; j++) {
      const int64_t j2 = sub ? sub[j] : j;
      const Coord c = coord(n_vec[j], h2_per_var, inv_odd_p, draw(seed, stream, (uint32_t)(k + burn_in), (uint32_t)j));
      const Step s = step<SAMPLING>(beta_hat[j], dotprods[(size_t)j2], curr[(size_t)j], c, p, sparse);
      const double diff = s.beta - curr[(size_t)j];
      curr[(size_t)j] = s.beta;
      if (s.drawn) {
        if (SAMPLING) {
          if (k >= 0) out[j + (int64_t)k * m] = s.beta;
        } else {
          if (s.nonzero) gap += s.beta * s.beta;
          if (k >= 0) out[j] += s.mean;
        }
      }
      if (diff != 0) {
        for (int64_t e = P[j2]; e < P[j2 + 1]; e++) dotprods[(size_t)I[e]] += X[e] * diff;
        nmove++;
      }
    }
    if (!SAMPLING && gap > gap0) {
      for (int64_t j = 0; j < m; j++) out[j] = NAN;
      if (moves) *moves = nmove;
      return;
    }
  }
  if (!SAMPLING)
    for (int64_t j = 0; j < m; j++) out[j] = out[j] / num_iter;
  if (moves) *moves = nmove;
}

extern "C" {

// G chains; stream NULL: 0 .. G-1; beta [m x G] column-major; moves [G] committed (non-zero diff) steps; secs [G]
void ldp_grid(const int64_t *P, const int32_t *I, const double *X, int64_t m2, const double *beta_hat, const double *n_vec,
              int64_t m, const int64_t *sub, const double *h2, const double *p, const int32_t *sparse, const uint64_t *stream,
              int64_t G, int burn_in, int num_iter, uint64_t seed, double *beta, int64_t *moves, double *secs, int nthreads) {
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic, 1)
#endif
  for (int64_t g = 0; g < G; g++) {
#ifdef _OPENMP
    const double t0 = omp_get_wtime();
#endif
    chain<false>(P, I, X, m2, beta_hat, n_vec, m, sub, h2[g], p[g], sparse[g] != 0, stream ? stream[g] : (uint64_t)g, burn_in,
                 num_iter, seed, beta + g * m, moves ? moves + g : nullptr);
#ifdef _OPENMP
    if (secs) secs[g] = omp_get_wtime() - t0;
#else
    if (secs) secs[g] = NAN;
#endif
  }
}

void ldp_sampling(const int64_t *P, const int32_t *I, const double *X, int64_t m2, const double *beta_hat, const double *n_vec,
                  int64_t m, const int64_t *sub, double h2, double p, int32_t sparse, uint64_t stream, int burn_in,
                  int num_iter, uint64_t seed, double *sample, int64_t *moves) {
  chain<true>(P, I, X, m2, beta_hat, n_vec, m, sub, h2, p, sparse != 0, stream, burn_in, num_iter, seed, sample, moves);
}

// ---- the pieces of the shared header, one by one ---------------------------------------------------------------------------
void ldp_philox(const uint32_t *ctr, const uint32_t *key, uint32_t *out) {
  const Philox o = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
  for (int t = 0; t < 4; t++) out[t] = o.v[t];
}

// U, Z [n] of positions j0 .. j0 + n - 1
void ldp_draws(uint64_t seed, uint64_t stream, uint32_t sweep, uint32_t j0, int64_t n, double *U, double *Z) {
  for (int64_t t = 0; t < n; t++) {
    const Draw d = draw(seed, stream, sweep, j0 + (uint32_t)t);
    U[t] = d.U;
    Z[t] = d.Z;
  }
}

// which: 0 exp, 1 log, 2 inverse normal CDF, 3 sqrt
void ldp_math(int which, const double *x, int64_t n, double *out) {
  for (int64_t t = 0; t < n; t++)
    out[t] = which == 0 ? exp_det(x[t]) : which == 1 ? log_det(x[t]) : which == 2 ? qnorm_det(x[t]) : sqrt_rn(x[t]);
}

// the host rule of the LDS window on a CSC with full columns: rows the ring has to hold (0 when ind_sub does not ascend),
// and whether the window path is taken
int ldp_envelope(const int64_t *P, const int32_t *I, int64_t m2, const int64_t *sub, int64_t m, int64_t *rows_out) {
  std::vector<int32_t> lo((size_t)m2), hi((size_t)m2);
  for (int64_t j = 0; j < m2; j++) {
    lo[(size_t)j] = P[j] < P[j + 1] ? I[P[j]] : 1;
    hi[(size_t)j] = P[j] < P[j + 1] ? I[P[j + 1] - 1] : 0;
  }
  const Envelope e = gibbs_envelope(lo.data(), hi.data(), sub, m);
  if (rows_out) *rows_out = e.rows;
  return gibbs_window_fits(e) ? 1 : 0;
}

int64_t ldp_window_rows(void) { return kGibbsWindowRows; }

}  // extern "C"
