// plr_ref.cpp — a CPU statement of big_spLinReg / big_spLogReg over a dense matrix of decoded values
// (n x m doubles, column-major, no missing value) followed by q covariates, for the parity tests and the timing probe.
//
// The coordinate updates, the per-row map of the logistic pass, the entry rule, the lambda grid and the bookkeeping
// come from bigsnpr_amd/csrc/plr_step.hpp, the header the kernels are compiled from; this file adds the sums over the
// rows and the loops.  `reverse` runs every sum over the rows from the last row to the first: the spread between the
// two orders is what the device tolerance is measured from.  Built with g++ -O2 -ffp-contract=off.  Chains run in
// parallel (OpenMP); each is one sequential computation, so the thread count changes no bit.
#include <math.h>
#include <stdint.h>

#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "plr_step.hpp"

using namespace bsn::plr;

namespace {

struct Opt {
  int family, nlambda, nlam_min, n_abort, dfmax, max_iter;
  double eps, ratio;
};

template <class F>
double rsum(int64_t n, bool rev, F f) {
  double s = 0.0;
  if (!rev)
    for (int64_t i = 0; i < n; i++) s += f(i);
  else
    for (int64_t i = n - 1; i >= 0; i--) s += f(i);
  return s;
}

struct Chain {
  const double *X, *cov, *y, *pf;
  const int32_t *fold;
  int64_t n, m;
  int q, k;
  double a;
  Opt o;
  bool exact, rev;
  int64_t p;
  double nt, nv, b0, nullv, thresh;
  std::vector<double> mk, cen, isd, beta, r, eta, w, g;
  std::vector<char> act;

  const double *col(int64_t j) const { return j < m ? X + j * n : cov + (j - m) * n; }

  void stats() {
    for (int64_t j = 0; j < p; j++) {
      const double *x = col(j);
      double lo = inf(), hi = -inf();
      for (int64_t i = 0; i < n; i++)
        if (mk[i] != 0.0) {
          lo = x[i] < lo ? x[i] : lo;
          hi = x[i] > hi ? x[i] : hi;
        }
      if (exact && j < m) {
        const double S1 = rsum(n, rev, [&](int64_t i) { return mk[i] * x[i]; });
        const double S2 = rsum(n, rev, [&](int64_t i) { return mk[i] * (x[i] * x[i]); });
        center_scale_sums(nt, S1, S2, cen[j], isd[j]);
      } else {
        const double c = rsum(n, rev, [&](int64_t i) { return mk[i] * x[i]; }) / nt;
        cen[j] = c;
        isd[j] = inv_scale_ss(nt, rsum(n, rev, [&](int64_t i) { return mk[i] * ((x[i] - c) * (x[i] - c)); }));
      }
      if (lo == hi) isd[j] = 0.0;
    }
  }

  // one run of the sweep at lambda; adds its passes to iter
  void sweep(double lam, int &iter) {
    while (iter < o.max_iter) {
      double maxupd = 0.0;
      if (o.family == 1) {
        for (int64_t i = 0; i < n; i++) {
          double s;
          log_map(eta[i], y[i], w[i], s, r[i]);
        }
        const double sw = rsum(n, rev, [&](int64_t i) { return mk[i] * w[i]; });
        const double ss = rsum(n, rev, [&](int64_t i) { return mk[i] * (w[i] * r[i]); });
        const double d = ss / sw;
        b0 = b0 + d;
        for (int64_t i = 0; i < n; i++) {
          r[i] = r[i] - d;
          eta[i] = eta[i] + d;
        }
        maxupd = d * d * (sw / nt);
      }
      for (int64_t j = 0; j < p; j++) {
        if (!act[j]) continue;
        const double *x = col(j);
        const double c = cen[j], is = isd[j];
        double shift, v = 1.0;
        if (o.family == 0) {
          const double dot = rsum(n, rev, [&](int64_t i) { return mk[i] * (xt(x[i], c, is) * r[i]); });
          shift = lin_coef(dot / nt + beta[j], lam, a, pf[j]) - beta[j];
        } else {
          v = rsum(n, rev, [&](int64_t i) { const double t = xt(x[i], c, is); return mk[i] * (w[i] * (t * t)); }) / nt;
          const double u = rsum(n, rev, [&](int64_t i) { return mk[i] * (w[i] * (xt(x[i], c, is) * r[i])); }) / nt + v * beta[j];
          shift = log_coef(u, v, lam, a, pf[j]) - beta[j];
        }
        if (shift != 0.0) {
          beta[j] = beta[j] + shift;
          for (int64_t i = 0; i < n; i++) {
            const double t = shift * xt(x[i], c, is);
            r[i] = r[i] - t;
            if (o.family == 1) eta[i] = eta[i] + t;
          }
          const double up = shift * shift * v;
          maxupd = up > maxupd ? up : maxupd;
        }
      }
      iter++;
      if (maxupd < thresh) break;
    }
  }

  // the losses of the current fit and the masked panel m o g of the scan
  void epilogue(double &loss, double &loss_val) {
    if (o.family == 0) {
      loss = rsum(n, rev, [&](int64_t i) { return mk[i] * (r[i] * r[i]); }) / nt;
      loss_val = rsum(n, rev, [&](int64_t i) { return (1.0 - mk[i]) * (r[i] * r[i]); }) / nv;
      for (int64_t i = 0; i < n; i++) g[i] = mk[i] * r[i];
    } else {
      loss = rsum(n, rev, [&](int64_t i) { return mk[i] * log_loss(eta[i], y[i]); }) / nt;
      loss_val = rsum(n, rev, [&](int64_t i) { return (1.0 - mk[i]) * log_loss(eta[i], y[i]); }) / nv;
      for (int64_t i = 0; i < n; i++) g[i] = mk[i] * log_grad(eta[i], y[i]);
    }
  }

  double z_of(int64_t j) const {
    const double *x = col(j);
    const double c = cen[j], is = isd[j];
    return rsum(n, rev, [&](int64_t i) { return xt(x[i], c, is) * g[i]; }) / nt;
  }

  int nnz() const {
    int c = 0;
    for (int64_t j = 0; j < p; j++) c += beta[j] != 0.0;
    return c;
  }

  void run(double *intercept, double *beta_out, double *lambda, double *loss_o, double *lossv_o, int32_t *iter_o,
           int32_t *nb_o, int32_t *n_done, int32_t *best, int32_t *status, int32_t *turns) {
    p = m + q;
    mk.resize(n);
    nt = 0;
    for (int64_t i = 0; i < n; i++) {
      mk[i] = fold[i] != k ? 1.0 : 0.0;
      nt += mk[i];
    }
    nv = (double)n - nt;
    cen.assign(p, 0.0);
    isd.assign(p, 0.0);
    beta.assign(p, 0.0);
    r.assign(n, 0.0);
    eta.assign(n, 0.0);
    w.assign(n, 0.0);
    g.assign(n, 0.0);
    act.assign(p, 0);
    stats();
    const double ybar = rsum(n, rev, [&](int64_t i) { return mk[i] * y[i]; }) / nt;
    if (o.family == 0) {
      b0 = ybar;
      for (int64_t i = 0; i < n; i++) r[i] = y[i] - ybar;
      nullv = rsum(n, rev, [&](int64_t i) { return mk[i] * (r[i] * r[i]); }) / nt;
      thresh = o.eps * nullv;
    } else {
      b0 = logit(ybar);
      for (int64_t i = 0; i < n; i++) eta[i] = b0;
      nullv = rsum(n, rev, [&](int64_t i) { return mk[i] * log_loss(b0, y[i]); }) / nt;
      thresh = o.eps * (2.0 * nullv);
    }
    for (int64_t j = 0; j < p; j++) act[j] = pf[j] == 0.0 && isd[j] != 0.0;
    int iter = 0;
    double loss, loss_val;
    sweep(0.0, iter);
    epilogue(loss, loss_val);
    double lmax = 0.0;
    for (int64_t j = 0; j < p; j++)
      if (!act[j] && isd[j] != 0.0) {
        const double t = absd(z_of(j)) / (a * pf[j]);
        lmax = t > lmax ? t : lmax;
      }
    for (int l = 0; l < o.nlambda; l++) lambda[l] = lambda_at(lmax, o.ratio, l, o.nlambda);
    Book bk;
    book_init(bk);
    std::vector<double> best_beta(p, 0.0);
    double best_b0 = b0;
    int l = 0, st, nturn = 0;
    for (;;) {
      bool improved;
      loss_o[l] = loss;
      lossv_o[l] = loss_val;
      iter_o[l] = iter;
      nb_o[l] = nnz();
      st = book(bk, l, loss_val, o.family == 1 ? loss / nullv : 1.0, nb_o[l], o.nlambda, o.nlam_min, o.n_abort, o.dfmax,
                improved);
      if (improved) {
        best_beta = beta;
        best_b0 = b0;
      }
      if (st != kLive) break;
      l++;
      iter = 0;
      for (;;) {
        sweep(lambda[l], iter);
        nturn++;
        epilogue(loss, loss_val);
        int added = 0;
        for (int64_t j = 0; j < p; j++)
          if (!act[j] && isd[j] != 0.0 && enters(z_of(j), lambda[l], a, pf[j])) {
            act[j] = 1;
            added++;
          }
        if (added == 0 || iter >= o.max_iter) break;
      }
    }
    *n_done = l + 1;
    *best = bk.best_l;
    *status = st;
    if (turns) *turns = nturn;
    double b = best_b0;
    for (int64_t j = 0; j < p; j++) {
      beta_out[j] = best_beta[j] * isd[j];
      b = b - cen[j] * beta_out[j];
    }
    *intercept = b;
  }
};

}  // namespace

extern "C" {

// X: n x m column-major; covar: n x q column-major (NULL when q = 0); pf [m + q]; fold [n] in 0 .. K - 1; chain
// c = a K + k.  opt_i: family (0 linear, 1 logistic), nlambda, nlam_min, n_abort, dfmax, max_iter; opt_d: eps,
// lambda_min_ratio.  exact != 0: the columns of X hold values whose sums are exact integers (a decoded 2-bit image).
// Outputs as bsn_bed_sp_reg's (include/bigsnpr_hip.h); turns [C] (may be NULL): the calls of sweep inside the lambda loop,
// which is the number of turns of the device's host loop in which the chain is live.
void plr_ref_fit(const double *X, int64_t n, int64_t m, const double *y, const double *covar, int q, const double *pf,
                 const int32_t *fold, int K, const double *alphas, int n_alpha, const int32_t *opt_i, const double *opt_d,
                 int exact, int reverse, int nthreads, double *intercept, double *beta, double *lambda, double *loss,
                 double *loss_val, int32_t *iter, int32_t *nb_active, int32_t *n_done, int32_t *best, int32_t *status,
                 int32_t *turns) {
  const Opt o{opt_i[0], opt_i[1], opt_i[2], opt_i[3], opt_i[4], opt_i[5], opt_d[0], opt_d[1]};
  const int C = K * n_alpha;
  const int64_t p = m + q;
  for (int64_t t = 0; t < (int64_t)o.nlambda * C; t++) {
    lambda[t] = loss[t] = loss_val[t] = nan("");
    iter[t] = nb_active[t] = 0;
  }
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
#pragma omp parallel for schedule(dynamic, 1)
  for (int c = 0; c < C; c++) {
    Chain ch;
    ch.X = X;
    ch.cov = covar;
    ch.y = y;
    ch.pf = pf;
    ch.fold = fold;
    ch.n = n;
    ch.m = m;
    ch.q = q;
    ch.k = c % K;
    ch.a = alphas[c / K];
    ch.o = o;
    ch.exact = exact != 0;
    ch.rev = reverse != 0;
    const int64_t L = (int64_t)o.nlambda * c;
    ch.run(intercept + c, beta + p * c, lambda + L, loss + L, loss_val + L, iter + L, nb_active + L, n_done + c, best + c,
           status + c, turns ? turns + c : nullptr);
  }
}

}  // extern "C"
