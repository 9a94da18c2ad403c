// plr_step.hpp — the statement of big_spLinReg / big_spLogReg apart from the sums over the rows: the
// standardisation of a column, the start of a chain, the coordinate updates of the two families, the per-row map of the
// logistic pass, the entry rule of the scan, the lambda grid and the bookkeeping of a path.  Shared by the kernels
// (plr.hip) and by the CPU statement (tests/native/plr_ref.cpp): the two cannot drift apart.  What differs between them
// is the order of the sums over the rows and the form of a 2-bit or byte column's integer sums, nothing else.
//
// exp, log and sqrt are gibbs_step.hpp's (+ - * / only, every operation rounded on its own), so host and device map the
// same eta to the same p and the same lambda_max to the same grid.
#pragma once
#include "gibbs_step.hpp"

#if defined(__HIPCC__)
#define BSN_PLR_HD __host__ __device__ inline
#else
#define BSN_PLR_HD inline
#endif

namespace bsn {
namespace plr {

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// how a chain ended (0: still running); the messages of the host mirror, in this order
enum Status { kLive = 0, kNoImprovement = 1, kTooManyVariables = 2, kSaturated = 3, kCompletePath = 4 };

constexpr double kPClamp = 1e-4;      // p beyond 1 - 1e-4 (below 1e-4) counts as 1 (0) with weight 1e-4
constexpr double kSaturated01 = 0.01; // training deviance / null deviance below this: "Model saturated"

BSN_PLR_HD double inf() { return gibbs::from_bits(0x7ff0000000000000ull); }
BSN_PLR_HD double absd(double x) { return x < 0 ? -x : x; }

// centre and 1 / (population standard deviation) of a column over the nt training rows.
// From the integer sums S1 = sum x, S2 = sum x^2 (exact for a 2-bit column; a byte column's come from its sums of k):
BSN_PLR_HD void center_scale_sums(double nt, double S1, double S2, double &c, double &inv_s) {
  c = S1 / nt;
  const double v = S2 / nt - c * c;
  inv_s = v > 0 ? 1.0 / gibbs::sqrt_rn(v) : 0.0;
}
// ... and of a dense column from ss = sum (x - c)^2 (two passes)
BSN_PLR_HD double inv_scale_ss(double nt, double ss) { return ss > 0 ? 1.0 / gibbs::sqrt_rn(ss / nt) : 0.0; }
// the standardised value
BSN_PLR_HD double xt(double x, double c, double inv_s) { return (x - c) * inv_s; }

BSN_PLR_HD double soft(double z, double t) { return z > t ? z - t : (z < -t ? z + t : 0.0); }
// linear: z = sum m x~ r / nt + beta
BSN_PLR_HD double lin_coef(double z, double lam, double a, double pf) {
  return soft(z, lam * a * pf) / (1.0 + lam * (1.0 - a) * pf);
}
// logistic: u = sum m w x~ r / nt + v beta, v = sum m w x~^2 / nt
BSN_PLR_HD double log_coef(double u, double v, double lam, double a, double pf) {
  return soft(u, lam * a * pf) / (v + lam * (1.0 - a) * pf);
}
// the scan: a column outside the active set enters when |z| > lambda a pf
BSN_PLR_HD bool enters(double z, double lam, double a, double pf) { return absd(z) > lam * a * pf; }

// y is 0 or 1.  p and 1 - p from exp(-|eta|); s = y - p, w the clamped weight, r = s / w
BSN_PLR_HD void log_map(double eta, double y, double &w, double &s, double &r) {
  const double e = gibbs::exp_det(eta < 0 ? eta : -eta);
  const double d = 1.0 + e;
  double p = eta < 0 ? e / d : 1.0 / d;
  if (p > 1.0 - kPClamp) {
    p = 1.0;
    w = kPClamp;
  } else if (p < kPClamp) {
    p = 0.0;
    w = kPClamp;
  } else {
    w = p * (1.0 - p);
  }
  s = y - p;
  r = s / w;
}
// y - p without the clamp: what the scan correlates the columns with
BSN_PLR_HD double log_grad(double eta, double y) {
  const double e = gibbs::exp_det(eta < 0 ? eta : -eta);
  const double d = 1.0 + e;
  return y - (eta < 0 ? e / d : 1.0 / d);
}
// -[y log p + (1 - y) log(1 - p)] = log(1 + exp(-|eta|)) + (the part of eta on the wrong side of y)
BSN_PLR_HD double log_loss(double eta, double y) {
  const double e = gibbs::exp_det(eta < 0 ? eta : -eta);
  const double l = gibbs::log_det(1.0 + e);
  const double wrong = y != 0.0 ? (eta < 0 ? -eta : 0.0) : (eta > 0 ? eta : 0.0);
  return l + wrong;
}
BSN_PLR_HD double logit(double p) { return gibbs::log_det(p) - gibbs::log_det(1.0 - p); }

// lambda_l, l = 0 .. nlambda - 1: log-spaced from lambda_max to ratio lambda_max
BSN_PLR_HD double lambda_at(double lmax, double ratio, int l, int nlambda) {
  if (l == 0 || nlambda < 2 || !(lmax > 0)) return lmax;
  return lmax * gibbs::exp_det(gibbs::log_det(ratio) * ((double)l / (double)(nlambda - 1)));
}

// The bookkeeping of a path once lambda_l is settled.  dev_ratio: training deviance / null deviance (pass 1 for the
// linear family); nnz: the number of non-zero coefficients.  Returns the chain's status.
struct Book {
  double best_val;
  int best_l, no_change;
};
BSN_PLR_HD void book_init(Book &b) {
  b.best_val = inf();
  b.best_l = 0;
  b.no_change = 0;
}
BSN_PLR_HD int book(Book &b, int l, double loss_val, double dev_ratio, int nnz, int nlambda, int nlam_min, int n_abort,
                    int dfmax, bool &improved) {
  improved = loss_val < b.best_val;
  if (improved) {
    b.best_val = loss_val;
    b.best_l = l;
    b.no_change = 0;
  } else if (l >= nlam_min) {
    b.no_change = b.no_change + 1;
  }
  if (dev_ratio < kSaturated01) return kSaturated;
  if (b.no_change >= n_abort) return kNoImprovement;
  if (l >= nlambda - 1) return kCompletePath;
  if (nnz >= dfmax) return kTooManyVariables;   // (checked before lambda_{l + 1} starts)
  return kLive;
}

#if defined(__clang__)
#pragma clang fp contract(on)
#endif

}  // namespace plr
}  // namespace bsn
