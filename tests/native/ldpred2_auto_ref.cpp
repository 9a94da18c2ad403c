// ldpred2_auto_ref.cpp — a CPU statement of LDpred2-auto's Gibbs sampler (src/ldpred2-auto.cpp:57-202 of the reference)
// over full CSC columns, for the parity tests and the timing probe.
//
// The coordinate step, the draws, rbeta, the bootstrap and the bounded MLE come from bigsnpr_amd/csrc/gibbs_auto.hpp, the
// header the kernel is compiled from; this file adds the sequential loop around them.  Built with g++ -O2
// -ffp-contract=off.  Chains run in parallel (OpenMP, one chain per thread at a time); each is one sequential loop, so
// the thread count changes no bit.
#include <math.h>
#include <stdint.h>

#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "gibbs_auto.hpp"

using namespace bsn::gibbs;

// the sums of the MLE on the host: every thread's share, then the tree
static MleSums host_sums(const double *a, const double *b, int64_t nb, double alpha1) {
  double pa[kSumThreads], pS[kSumThreads], pSa[kSumThreads];
  for (int t = 0; t < kSumThreads; t++) {
    const MleSums s = mle_partial(a, b, nb, alpha1, t);
    pa[t] = s.a, pS[t] = s.S, pSa[t] = s.Sa;
  }
  MleSums r;
  r.a = tree_sum(pa), r.S = tree_sum(pS), r.Sa = tree_sum(pSa);
  return r;
}

static MlePar host_mle(const double *a, const double *b, int64_t nb, double alpha_lo, double alpha_hi, double sigma2_prev) {
  return mle_solve([&](double al) { return host_sums(a, b, nb, al); }, nb, alpha_lo, alpha_hi, sigma2_prev);
}

struct AutoOut {
  double *beta_est, *postp_est, *corr_est;   // [m]
  double *sample_beta;                       // [m x n_report], zeroed here
  double *path_p, *path_h2, *path_alpha;     // [burn_in + num_iter]
  int32_t *path_nb;                          // [burn_in + num_iter] size of the causal set after each sweep (-1: not run)
  int64_t *moves;
};

static void chain(const int64_t *P, const int32_t *I, const double *X, int64_t m2, const double *beta_hat, const double *n_vec,
                  const double *log_var, int64_t m, const int64_t *sub, double p_init, uint64_t stream, double h2_init,
                  int burn_in, int num_iter, int report_step, bool no_jump_sign, double shrink_corr, bool use_mle, double p_lo,
                  double p_hi, double alpha_lo, double alpha_hi, double mean_ld, uint64_t seed, const AutoOut &o) {
  const int tot = burn_in + num_iter;
  if (report_step > num_iter) report_step = num_iter + 1;
  const int64_t n_report = num_iter / report_step;
  std::vector<double> curr((size_t)m, 0.0), dotprods((size_t)m2, 0.0), ba((size_t)m), bb((size_t)m);
  std::vector<int32_t> causal;
  for (int64_t j = 0; j < m; j++) o.beta_est[j] = o.postp_est[j] = o.corr_est[j] = 0.0;
  for (int64_t t = 0; t < m * n_report; t++) o.sample_beta[t] = 0.0;
  for (int k = 0; k < tot; k++) {
    o.path_p[k] = o.path_h2[k] = o.path_alpha[k] = NAN;
    if (o.path_nb) o.path_nb[k] = -1;
  }
  int ind_report = 0, next_report = burn_in + report_step - 1;
  double cur_h2 = 0;
  double h2 = h2_init < kAutoMinH2 ? kAutoMinH2 : h2_init;
  double p = clamp_p(p_init, p_lo, p_hi);
  double alpha1 = 0, sigma2 = h2 / (m * p);
  double ss = 0.0;
  for (int64_t j = 0; j < m; j++) ss = ss + beta_hat[j] * beta_hat[j];
  const double gap0 = 2 * ss;
  int64_t nmove = 0;
  bool diverged = false;
  for (int k = 0; k < tot; k++) {
    const double inv_odd_p = (1 - p) / p;
    double gap = 0;
    causal.clear();
    for (int64_t j = 0; j < m; j++) {
      const int64_t j2 = sub ? sub[j] : j;
      const Coord c = coord_auto(n_vec[j], use_mle ? log_var[j] : 0.0, alpha1, sigma2, inv_odd_p, use_mle,
                                 draw(seed, stream, (uint32_t)k, (uint32_t)j));
      const StepAuto s = step_auto(beta_hat[j], dotprods[(size_t)j2], curr[(size_t)j], c, shrink_corr, no_jump_sign);
      if (k >= burn_in) {
        o.postp_est[j] += s.postp;
        o.beta_est[j] += s.mean;
        o.corr_est[j] += s.shrunk;
      }
      curr[(size_t)j] = s.beta;
      if (s.causal) {
        causal.push_back((int32_t)j);
        gap += s.beta * s.beta;
      }
      if (s.diff != 0) {
        cur_h2 += h2_term(s);
        for (int64_t e = P[j2]; e < P[j2 + 1]; e++) dotprods[(size_t)I[e]] += X[e] * s.diff;
        nmove++;
      }
    }
    if (gap > gap0) {
      diverged = true;
      break;
    }
    const int64_t nb = (int64_t)causal.size();
    p = next_p(nb, m, mean_ld, p_lo, p_hi, seed, stream, (uint32_t)k);
    h2 = cur_h2 < kAutoMinH2 ? kAutoMinH2 : cur_h2;
    if (use_mle) {
      if (nb > 0) {
        for (int64_t kk = 0; kk < nb; kk++) {
          const int32_t jj = causal[(size_t)boot_index(nb, seed, stream, (uint32_t)k, (uint32_t)kk)];
          ba[(size_t)kk] = log_var[jj];
          bb[(size_t)kk] = curr[(size_t)jj] * curr[(size_t)jj];
        }
        const MlePar par = host_mle(ba.data(), bb.data(), nb, alpha_lo, alpha_hi, sigma2);
        alpha1 = par.alpha1;
        sigma2 = par.sigma2;
      }
    } else {
      sigma2 = h2 / (m * p);
    }
    o.path_p[k] = p;
    o.path_h2[k] = h2;
    if (use_mle) o.path_alpha[k] = alpha1 - 1;
    if (o.path_nb) o.path_nb[k] = (int32_t)nb;
    if (k == next_report) {
      for (const int32_t jj : causal) o.sample_beta[jj + (int64_t)ind_report * m] = curr[(size_t)jj];
      ind_report++;
      next_report += report_step;
    }
  }
  for (int64_t j = 0; j < m; j++) {
    o.beta_est[j] = diverged ? NAN : o.beta_est[j] / num_iter;
    o.postp_est[j] = diverged ? NAN : o.postp_est[j] / num_iter;
    o.corr_est[j] = diverged ? NAN : o.corr_est[j] / num_iter;
  }
  if (o.moves) *o.moves = nmove;
}

extern "C" {

// G chains; stream NULL: 0 .. G-1; outputs column-major per chain as bsn_ldpred2_auto lays them out; path_nb, moves, secs
// may be NULL
void lda_auto(const int64_t *P, const int32_t *I, const double *X, int64_t m2, const double *beta_hat, const double *n_vec,
              const double *log_var, int64_t m, const int64_t *sub, const double *p_init, const uint64_t *stream, int64_t G,
              double h2_init, int burn_in, int num_iter, int report_step, int no_jump_sign, double shrink_corr, int use_mle,
              double p_lo, double p_hi, double alpha_lo, double alpha_hi, double mean_ld, uint64_t seed, double *beta_est,
              double *postp_est, double *corr_est, double *sample_beta, double *path_p, double *path_h2, double *path_alpha,
              int32_t *path_nb, int64_t *moves, double *secs, int nthreads) {
  const int64_t tot = (int64_t)burn_in + num_iter;
  const int64_t n_report = report_step > num_iter ? 0 : num_iter / report_step;
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic, 1)
#endif
  for (int64_t g = 0; g < G; g++) {
#ifdef _OPENMP
    const double t0 = omp_get_wtime();
#endif
    AutoOut o;
    o.beta_est = beta_est + g * m, o.postp_est = postp_est + g * m, o.corr_est = corr_est + g * m;
    o.sample_beta = sample_beta + g * m * n_report;
    o.path_p = path_p + g * tot, o.path_h2 = path_h2 + g * tot, o.path_alpha = path_alpha + g * tot;
    o.path_nb = path_nb ? path_nb + g * tot : nullptr;
    o.moves = moves ? moves + g : nullptr;
    chain(P, I, X, m2, beta_hat, n_vec, log_var, m, sub, p_init[g], stream ? stream[g] : (uint64_t)g, h2_init, burn_in,
          num_iter, report_step, no_jump_sign != 0, shrink_corr, use_mle != 0, p_lo, p_hi, alpha_lo, alpha_hi, mean_ld, seed, o);
#ifdef _OPENMP
    if (secs) secs[g] = omp_get_wtime() - t0;
#else
    if (secs) secs[g] = NAN;
#endif
  }
}

// ---- the pieces of the shared header, one by one ---------------------------------------------------------------------------
// par [2] = (alpha + 1, sigma2) in and out; nb == 0 leaves it as it was
void lda_mle(const double *a, const double *b, int64_t nb, double alpha_lo, double alpha_hi, double *par) {
  if (nb <= 0) return;
  const MlePar r = host_mle(a, b, nb, alpha_lo, alpha_hi, par[1]);
  par[0] = r.alpha1, par[1] = r.sigma2;
}

// the three sums at one alpha + 1, in the fixed order
void lda_sums(const double *a, const double *b, int64_t nb, double alpha1, double *out) {
  const MleSums s = host_sums(a, b, nb, alpha1);
  out[0] = s.a, out[1] = s.S, out[2] = s.Sa;
}

// n draws of rbeta(a, b): draw t at the sweep word sweep0 + t
void lda_rbeta(double a, double b, uint64_t seed, uint64_t stream, uint32_t sweep0, int64_t n, double *out) {
  for (int64_t t = 0; t < n; t++) out[t] = rbeta_det(a, b, seed, stream, sweep0 + (uint32_t)t);
}

double lda_next_p(int64_t nb, int64_t m, double mean_ld, double p_lo, double p_hi, uint64_t seed, uint64_t stream, uint32_t sweep) {
  return next_p(nb, m, mean_ld, p_lo, p_hi, seed, stream, sweep);
}

int64_t lda_boot_pick(int64_t nb, double U) { return boot_pick(nb, U); }

// the bootstrap's indices of one sweep
void lda_boot(int64_t nb, uint64_t seed, uint64_t stream, uint32_t sweep, int64_t *out) {
  for (int64_t k = 0; k < nb; k++) out[k] = boot_index(nb, seed, stream, sweep, (uint32_t)k);
}

uint32_t lda_tagged_sweep(uint32_t sweep, uint32_t tag) { return tagged_sweep(sweep, tag); }

double lda_log(double x) { return log_det(x); }

}  // extern "C"
