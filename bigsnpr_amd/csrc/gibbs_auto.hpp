// gibbs_auto.hpp — what LDpred2-auto adds to the Gibbs sampler of gibbs_step.hpp (src/ldpred2-auto.cpp:57-202 and
// src/optim-MLE-alpha.h of the reference): the coordinate step with shrink_corr, the frequency-dependent prior and
// no_jump_sign, and the epilogue of a sweep — a beta draw for p, the bootstrap of the causal set and the bounded
// maximum-likelihood estimate of (alpha + 1, sigma2).  Shared by k_ldpred2_auto (sparse_ld.hip) and by the CPU statement
// (tests/native/ldpred2_auto_ref.cpp) under the rules of gibbs_step.hpp: + - * /, sqrt and integer operations only, no
// contraction, so both sides give the same bits.
//
// Two documented deviations from the reference, of the same kind:
//   * the random numbers (R's generator cannot be reproduced): every draw comes from Philox at a counter of its own;
//   * the MLE.  The reference runs L-BFGS-B from the previous estimate, whose iterates cannot be reproduced bit for
//     bit and which stops at a tolerance.  Here the minimiser it approximates is computed.  With t = log sigma2 the
//     objective  f = alpha1 sum_a + nb t + sum_k b_k exp(-alpha1 a_k - t)  is jointly convex in (alpha1, t) and the box
//     [alpha bounds] x [sigma2_prev / 2, 2 sigma2_prev] is convex.  For a fixed alpha1 the best sigma2 is
//     clamp(S(alpha1) / nb, lo, hi) with S = sum_k b_k exp(-alpha1 a_k); the derivative of the profile,
//     sum_a - S_a(alpha1) / sigma2*(alpha1) with S_a = sum_k a_k b_k exp(-alpha1 a_k), is non-decreasing, so its root is
//     bracketed by the bounds or the minimum lies at one of them, and kMleHalvings bisections on its sign locate it to
//     the last place of a double.
//   The sums over the nb bootstrap entries have one order, a function of nb alone: kSumThreads strided partial sums
//   (thread t adds entries t, t + kSumThreads, ... in that order), then the pairwise tree of tree_sum below.
#pragma once
#include "gibbs_step.hpp"

namespace bsn {
namespace gibbs {

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

constexpr double kAutoMinH2 = 1e-3;   // MIN_H2 of src/ldpred2-auto.cpp
constexpr int kSumThreads = 256;      // strided partial sums of the MLE (the kernel's workgroup)
constexpr int kMleHalvings = 64;
constexpr int kAutoSweepBits = 30;    // the sweep word of a counter keeps its two top bits for the purpose tag

// ---- counters of the epilogue -------------------------------------------------------------------------------------------
// The coordinate draw stays draw(seed, stream, sweep, j): tag 0.  The epilogue of sweep k draws at (index, k | tag << 30,
// stream): tag 1 the attempts of the first gamma, 2 those of the second, 3 the bootstrap positions.  sweep < 2^30.
enum : uint32_t { kTagCoord = 0, kTagGammaA = 1, kTagGammaB = 2, kTagBoot = 3 };

BSN_GIBBS_HD uint32_t tagged_sweep(uint32_t sweep, uint32_t tag) { return sweep | (tag << kAutoSweepBits); }

// ---- one coordinate --------------------------------------------------------------------------------------------------------
// What does not depend on the chain's state: coord() of gibbs_step.hpp with scale_freq * sigma2 in the place of
// h2_per_var, C1 = scale_freq * sigma2 * n_j as the reference associates it.
BSN_GIBBS_HD Coord coord_auto(double n_j, double log_var_j, double alpha_plus_one, double sigma2, double inv_odd_p, bool use_mle,
                              Draw d) {
  const double scale_freq = use_mle ? exp_det(alpha_plus_one * log_var_j) : 1;
  return coord(n_j, scale_freq * sigma2, inv_odd_p, d);
}

struct StepAuto {
  double beta;     // the new curr_beta[j]
  double postp;    // avg_postp[j] receives it
  double mean;     // C3 * postp: avg_beta[j]
  double shrunk;   // dotprod_shrunk: avg_beta_hat[j], and the h2 update
  double diff;     // beta - prev
  bool causal;     // joins ind_causal, gap receives beta^2
};

BSN_GIBBS_HD StepAuto step_auto(double beta_hat_j, double dot_j2, double prev, const Coord &c, double shrink_corr,
                                bool no_jump_sign) {
  const double res = beta_hat_j - shrink_corr * (dot_j2 - prev);
  const double C3 = c.C2 * res;
  StepAuto s;
  s.postp = 1 / (1 + c.odds * exp_det(-C3 * C3 / c.C4 / 2));
  s.mean = C3 * s.postp;
  s.shrunk = shrink_corr * dot_j2 + (1 - shrink_corr) * prev;
  s.beta = 0;
  s.causal = false;
  if (s.postp > c.U) {
    const double samp = C3 + c.noise;
    if (!(no_jump_sign && samp * prev < 0)) {
      s.beta = samp;
      s.causal = true;
    }
  }
  s.diff = s.beta - prev;
  return s;
}

// what cur_h2_est receives from a coordinate whose diff is not 0
BSN_GIBBS_HD double h2_term(const StepAuto &s) { return s.diff * (2 * s.shrunk + s.diff); }

// ---- rbeta ------------------------------------------------------------------------------------------------------------------
// Marsaglia & Tsang (2000), "A simple method for generating gamma variables", for a shape >= 1 (no boost step): attempt
// i takes U and Z of the counter (i, sweep word, stream).  1 + c Z > 0 is at least 2^-53 and at most 5, its cube and U are
// positive normal numbers: log_det is inside its domain.
BSN_GIBBS_HD double rgamma_det(double shape, uint64_t seed, uint64_t stream, uint32_t sweep_word) {
  const double d = shape - 1.0 / 3.0;
  const double c = 1 / sqrt_rn(9 * d);
  for (uint32_t i = 0;; i++) {
    const Draw r = draw(seed, stream, sweep_word, i);
    double v = 1 + c * r.Z;
    if (v <= 0) continue;
    v = v * v * v;
    if (log_det(r.U) < 0.5 * r.Z * r.Z + d - d * v + d * log_det(v)) return d * v;
  }
}

// Ga / (Ga + Gb), both shapes >= 1
BSN_GIBBS_HD double rbeta_det(double a, double b, uint64_t seed, uint64_t stream, uint32_t sweep) {
  const double ga = rgamma_det(a, seed, stream, tagged_sweep(sweep, kTagGammaA));
  const double gb = rgamma_det(b, seed, stream, tagged_sweep(sweep, kTagGammaB));
  return ga / (ga + gb);
}

// std::min(std::max(p_bounds[0], p), p_bounds[1])
BSN_GIBBS_HD double clamp_p(double p, double p_lo, double p_hi) {
  const double q = p_lo < p ? p : p_lo;
  return p_hi < q ? p_hi : q;
}

// p of the next sweep: rbeta(1 + nb / mean_ld, 1 + (m - nb) / mean_ld), clamped to p_bounds
BSN_GIBBS_HD double next_p(int64_t nb, int64_t m, double mean_ld, double p_lo, double p_hi, uint64_t seed, uint64_t stream,
                           uint32_t sweep) {
  const double p = rbeta_det(1 + nb / mean_ld, 1 + (m - nb) / mean_ld, seed, stream, sweep);
  return clamp_p(p, p_lo, p_hi);
}

// ---- bootstrap ----------------------------------------------------------------------------------------------------------------
// position k of the bootstrap takes entry k2 = (int64)(nb U) of ind_causal.  The min keeps the index below nb whatever the
// product rounds to (with U <= 1 - 2^-53 and nb < 2^53 it stays below nb; a uniform that reached 1 would not).
BSN_GIBBS_HD int64_t boot_pick(int64_t nb, double U) {
  const int64_t k2 = (int64_t)((double)nb * U);
  return k2 < nb - 1 ? k2 : nb - 1;
}

BSN_GIBBS_HD int64_t boot_index(int64_t nb, uint64_t seed, uint64_t stream, uint32_t sweep, uint32_t k) {
  const Philox o = philox4x32_10(k, tagged_sweep(sweep, kTagBoot), (uint32_t)stream, (uint32_t)(stream >> 32), (uint32_t)seed,
                                 (uint32_t)(seed >> 32));
  return boot_pick(nb, unit_open(o.v[0], o.v[1]));
}

// ---- the sums of the MLE ------------------------------------------------------------------------------------------------------
struct MleSums {
  double a, S, Sa;   // sum a_k; sum b_k exp(-alpha1 a_k); sum a_k b_k exp(-alpha1 a_k)
};

// thread t's share, entries t, t + kSumThreads, ... in that order
BSN_GIBBS_HD MleSums mle_partial(const double *a, const double *b, int64_t nb, double alpha1, int t) {
  MleSums s = {0, 0, 0};
  for (int64_t k = t; k < nb; k += kSumThreads) {
    const double ck = b[k] * exp_det(-alpha1 * a[k]);
    s.a = s.a + a[k];
    s.S = s.S + ck;
    s.Sa = s.Sa + a[k] * ck;
  }
  return s;
}

// The tree over the kSumThreads partial sums: at distance s = 1, 2, 4, ..., element t (a multiple of 2 s) receives
// element t + s.  The kernel runs the distances below 64 inside each wave (tree_wave) and the last two over four LDS
// doubles (tree_four); the host runs all of them on an array.  The same additions in the same order.
inline double tree_sum(double *part) {
  for (int s = 1; s < kSumThreads; s <<= 1)
    for (int t = 0; t < kSumThreads; t += 2 * s) part[t] = part[t] + part[t + s];
  return part[0];
}

BSN_GIBBS_HD double tree_four(double w0, double w1, double w2, double w3) { return (w0 + w1) + (w2 + w3); }

#if defined(__HIPCC__)
// lane 0 of each wave ends with the tree sum of its 64 partial sums
__device__ __forceinline__ double tree_wave(double v) {
  for (int s = 1; s < 64; s <<= 1) v = v + __shfl_down(v, s, 64);
  return v;
}
#endif

// ---- the MLE, given a way to form the sums at an alpha1 --------------------------------------------------------------------
struct MlePar {
  double alpha1, sigma2;
};

BSN_GIBBS_HD double clamp_det(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// sums(alpha1) -> MleSums over all nb entries, in the fixed order.  nb > 0.
template <class Sums>
BSN_GIBBS_HD MlePar mle_solve(Sums sums, int64_t nb, double alpha_lo, double alpha_hi, double sigma2_prev) {
  const double lo = sigma2_prev / 2, hi = sigma2_prev * 2;
  MlePar r;
  MleSums s = sums(alpha_lo);
  double sig = clamp_det(s.S / (double)nb, lo, hi);
  if (!(alpha_lo < alpha_hi) || s.a - s.Sa / sig >= 0) {
    r.alpha1 = alpha_lo, r.sigma2 = sig;
    return r;
  }
  s = sums(alpha_hi);
  sig = clamp_det(s.S / (double)nb, lo, hi);
  if (s.a - s.Sa / sig <= 0) {
    r.alpha1 = alpha_hi, r.sigma2 = sig;
    return r;
  }
  double x0 = alpha_lo, x1 = alpha_hi;   // derivative < 0 at x0, > 0 at x1
  for (int it = 0; it < kMleHalvings; it++) {
    const double mid = x0 + (x1 - x0) / 2;
    s = sums(mid);
    sig = clamp_det(s.S / (double)nb, lo, hi);
    if (s.a - s.Sa / sig >= 0) x1 = mid; else x0 = mid;
  }
  r.alpha1 = x0 + (x1 - x0) / 2;
  s = sums(r.alpha1);
  r.sigma2 = clamp_det(s.S / (double)nb, lo, hi);
  return r;
}

#if defined(__clang__)
#pragma clang fp contract(on)
#endif

}  // namespace gibbs
}  // namespace bsn
