// gibbs_step.hpp — what one coordinate step of LDpred2's Gibbs sampler computes (src/ldpred2.cpp:36-62 and
// src/ldpred2-sampling.cpp:33-54 of the reference), the counter-based generator its two random numbers come from, and
// the rule that decides whether a chain's slice of dotprods fits the LDS window.  Shared by the kernel (sparse_ld.hip)
// and by the CPU statement (tests/native/ldpred2_ref.cpp): the two cannot drift apart.
//
// Bit equality of host and device.  exp, log and the inverse normal CDF are written here with + - * /, sqrt and integer
// operations only, every one of them rounded on its own (no contraction: the pragma below on the device, -ffp-contract=off
// on the host).  fp64 division and square root are correctly rounded on both sides, so the same inputs give the same
// bits.  The libm of either side is not used: device and host exp differ in the last place, and one flipped
// `post_p > U` sends a chain elsewhere.  Accuracy: a few units in the last place (tests/test_ldpred2_gibbs_cpu.py holds
// all three within 1e-13 relative of libm), ten orders below the Monte Carlo noise of any chain.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define BSN_GIBBS_HD __host__ __device__ __forceinline__
#else
#define BSN_GIBBS_HD inline
#endif

namespace bsn {
namespace gibbs {

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

BSN_GIBBS_HD double sqrt_rn(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(x);
#else
  return std::sqrt(x);
#endif
}

BSN_GIBBS_HD double from_bits(uint64_t b) {
  union {
    uint64_t u;
    double d;
  } v;
  v.u = b;
  return v.d;
}

BSN_GIBBS_HD uint64_t to_bits(double d) {
  union {
    uint64_t u;
    double d;
  } v;
  v.d = d;
  return v.u;
}

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) -------------------
struct Philox {
  uint32_t v[4];
};

BSN_GIBBS_HD Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    const uint64_t a = (uint64_t)0xD2511F53u * c0, b = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(b >> 32) ^ c1 ^ k0, n1 = (uint32_t)b;
    const uint32_t n2 = (uint32_t)(a >> 32) ^ c3 ^ k1, n3 = (uint32_t)a;
    c0 = n0, c1 = n1, c2 = n2, c3 = n3;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  Philox o;
  o.v[0] = c0, o.v[1] = c1, o.v[2] = c2, o.v[3] = c3;
  return o;
}

// an odd 53-bit integer over 2^53: in the open interval (0, 1), symmetric about 1/2, exact in a double
BSN_GIBBS_HD double unit_open(uint32_t a, uint32_t b) {
  const uint64_t n = ((uint64_t)a << 20) | (b >> 12);   // 52 bits
  return (double)(2 * n + 1) * 1.1102230246251565e-16;  // 2^-53
}

// ---- exp, log, inverse normal CDF -----------------------------------------------------------------------------------------
constexpr double kLn2Hi = 6.93147180369123816490e-01;   // the high 32 bits of ln 2: k * kLn2Hi is exact for |k| < 2^20
constexpr double kLn2Lo = 1.90821492927058770002e-10;

// x = k ln 2 + r with |r| <= ln 2 / 2, exp(r) by its Taylor series to r^13 (remainder below 4e-18), times 2^k.
// Below -708 the result is 0 (the true value is below 3.4e-308); above 709 it is +inf; a NaN stays one.
BSN_GIBBS_HD double exp_det(double x) {
  if (x != x) return x;
  if (x < -708.0) return 0.0;
  if (x > 709.0) return from_bits(0x7ff0000000000000ull);
  const int k = (int)(x * 1.4426950408889634 + (x < 0 ? -0.5 : 0.5));
  const double r = (x - k * kLn2Hi) - k * kLn2Lo;
  double s = 1.0 / 6227020800.0;
  s = s * r + 1.0 / 479001600.0;
  s = s * r + 1.0 / 39916800.0;
  s = s * r + 1.0 / 3628800.0;
  s = s * r + 1.0 / 362880.0;
  s = s * r + 1.0 / 40320.0;
  s = s * r + 1.0 / 5040.0;
  s = s * r + 1.0 / 720.0;
  s = s * r + 1.0 / 120.0;
  s = s * r + 1.0 / 24.0;
  s = s * r + 1.0 / 6.0;
  s = s * r + 0.5;
  s = s * r + 1.0;
  s = s * r + 1.0;
  // 2^k in two factors: k reaches 1023 + 1 after rounding (x = 709), and -1022 - 1 at the low end
  const int k1 = k / 2, k2 = k - k1;
  return s * from_bits((uint64_t)(1023 + k1) << 52) * from_bits((uint64_t)(1023 + k2) << 52);
}

// x = 2^e m with m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(s), s = (m - 1) / (m + 1), |s| < 0.1716: the series to s^23
// (next term below 7e-19 relative).  For positive normal x; the sampler calls it on (2^-53, 0.075].
BSN_GIBBS_HD double log_det(double x) {
  uint64_t b = to_bits(x);
  int e = (int)(b >> 52) - 1023;
  b = (b & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
  double m = from_bits(b);
  if (m > 1.4142135623730951) {
    m = m * 0.5;
    e = e + 1;
  }
  const double f = m - 1.0;
  const double s = f / (2.0 + f);
  const double z = s * s;
  double t = 1.0 / 23.0;
  t = t * z + 1.0 / 21.0;
  t = t * z + 1.0 / 19.0;
  t = t * z + 1.0 / 17.0;
  t = t * z + 1.0 / 15.0;
  t = t * z + 1.0 / 13.0;
  t = t * z + 1.0 / 11.0;
  t = t * z + 1.0 / 9.0;
  t = t * z + 1.0 / 7.0;
  t = t * z + 1.0 / 5.0;
  t = t * z + 1.0 / 3.0;
  t = t * z + 1.0;
  return e * kLn2Hi + (2.0 * s * t + e * kLn2Lo);
}

// Wichura (1988), Algorithm AS241 (PPND16): the percentage points of the normal distribution, for 0 < p < 1
BSN_GIBBS_HD double qnorm_det(double p) {
  const double q = p - 0.5;
  double r, num, den;
  if ((q < 0 ? -q : q) <= 0.425) {
    r = 0.180625 - q * q;
    num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
               4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
             1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
    den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
               2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
             4.2313330701600911252e+1) * r + 1.0);
    return num / den;
  }
  r = q <= 0.0 ? p : 1.0 - p;
  r = sqrt_rn(-log_det(r));
  if (r <= 5.0) {
    r = r - 1.6;
    num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
               1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
             4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
    den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
               1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
             2.05319162663775882187e+0) * r + 1.0);
  } else {
    r = r - 5.0;
    num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
               2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
             5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
    den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
               7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
             5.99832206555887937690e-1) * r + 1.0);
  }
  const double x = num / den;
  return q < 0.0 ? -x : x;
}

// ---- the two random numbers of a coordinate ----------------------------------------------------------------------------
// key: the 64-bit seed; counter: (position j in the subset, sweep k + burn_in, the chain's 64-bit stream id).  Nothing
// else enters: not what other coordinates did, not batching, not the kernel path.  j is the position in ind_sub, not
// the column of corr, so that a run on corr with ind.corr = sub draws what a run on corr[sub, sub] draws.
struct Draw {
  double U, Z;   // uniform on (0, 1); standard normal, as the inverse CDF of a second uniform
};

BSN_GIBBS_HD Draw draw(uint64_t seed, uint64_t stream, uint32_t sweep, uint32_t j) {
  const Philox o = philox4x32_10(j, sweep, (uint32_t)stream, (uint32_t)(stream >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
  Draw d;
  d.U = unit_open(o.v[0], o.v[1]);
  d.Z = qnorm_det(unit_open(o.v[2], o.v[3]));
  return d;
}

// ---- one coordinate ----------------------------------------------------------------------------------------------------
// What does not depend on the chain's state, formed once per coordinate and sweep (the reference forms the same
// values, in the same operations, inside its loop):
//   C1 = h2_per_var n_j, C2 = 1 / (1 + 1 / C1), C4 = C2 / n_j, odds = inv_odd_p sqrt(1 + C1), noise = sqrt(C4) Z
struct Coord {
  double C2, C4, odds, noise, U;
};

BSN_GIBBS_HD Coord coord(double n_j, double h2_per_var, double inv_odd_p, Draw d) {
  Coord c;
  const double C1 = h2_per_var * n_j;
  c.C2 = 1 / (1 + 1 / C1);
  c.C4 = c.C2 / n_j;
  c.odds = inv_odd_p * sqrt_rn(1 + C1);
  c.noise = sqrt_rn(c.C4) * d.Z;
  c.U = d.U;
  return c;
}

struct Step {
  double beta;    // the new curr_beta[j]
  double mean;    // C3 * post_p: what avg_beta[j] receives (grid)
  bool drawn;     // the non-sparse branch was taken: avg_beta / sample_beta are touched
  bool nonzero;   // post_p > U: gap receives beta^2 (grid)
};

// SAMPLING picks the association of the residual: beta_hat - (dot - curr) in ldpred2.cpp, beta_hat + curr - dot in
// ldpred2-sampling.cpp
template <bool SAMPLING>
BSN_GIBBS_HD Step step(double beta_hat_j, double dot_j2, double curr_j, const Coord &c, double p, bool sparse) {
  const double res = SAMPLING ? beta_hat_j + curr_j - dot_j2 : beta_hat_j - (dot_j2 - curr_j);
  const double C3 = c.C2 * res;
  const double post_p = 1 / (1 + c.odds * exp_det(-C3 * C3 / c.C4 / 2));
  Step s;
  s.beta = 0;
  s.mean = 0;
  s.drawn = !(sparse && post_p < p);
  s.nonzero = false;
  if (s.drawn) {
    s.nonzero = post_p > c.U;
    if (s.nonzero) s.beta = C3 + c.noise;
    s.mean = C3 * post_p;
  }
  return s;
}

#if defined(__clang__)
#pragma clang fp contract(on)
#endif

// ---- the LDS window: does a chain's live slice of dotprods fit? ----------------------------------------------------------
// The kernel decides 64 coordinates at a time.  While block b (positions 64 b .. 64 b + 63) is worked on, the rows
// of dotprods that can still be read or written are
//   lo[b] = min over the columns of blocks >= b of their first row (and of j2 itself, which is read),
//   hi[b] = max over the columns of blocks <= b of their last row (and of j2),
// both non-decreasing in b when ind_sub ascends, also for thresholded matrices whose raw spans are not monotone.
// rows = max_b (hi[b] - lo[b] + 1) is what the ring in LDS has to hold.
constexpr int kGibbsBlock = 64;                  // coordinates decided together (one per lane)
constexpr int64_t kGibbsWindowRows = 16384;      // 128 KiB of the CU's 160 KiB

struct Envelope {
  bool ascending = true;
  int64_t rows = 0;
  std::vector<int32_t> lo, hi;   // per block of kGibbsBlock positions
};

inline Envelope gibbs_envelope(const int32_t *col_lo, const int32_t *col_hi, const int64_t *ind_sub, int64_t m) {
  Envelope e;
  const int64_t nb = (m + kGibbsBlock - 1) / kGibbsBlock;
  e.lo.assign((size_t)nb, 0);
  e.hi.assign((size_t)nb, 0);
  for (int64_t j = 1; j < m && ind_sub; j++)
    if (ind_sub[j] <= ind_sub[j - 1]) e.ascending = false;
  if (!e.ascending || m == 0) return e;
  int64_t run = -1;
  for (int64_t j = 0; j < m; j++) {
    const int64_t j2 = ind_sub ? ind_sub[j] : j;
    run = std::max<int64_t>(run, std::max<int64_t>(j2, col_lo[j2] <= col_hi[j2] ? col_hi[j2] : j2));
    e.hi[(size_t)(j / kGibbsBlock)] = (int32_t)run;
  }
  run = INT64_MAX;
  for (int64_t j = m - 1; j >= 0; j--) {
    const int64_t j2 = ind_sub ? ind_sub[j] : j;
    run = std::min<int64_t>(run, std::min<int64_t>(j2, col_lo[j2] <= col_hi[j2] ? col_lo[j2] : j2));
    e.lo[(size_t)(j / kGibbsBlock)] = (int32_t)run;
  }
  for (int64_t b = 0; b < nb; b++) e.rows = std::max<int64_t>(e.rows, (int64_t)e.hi[(size_t)b] - e.lo[(size_t)b] + 1);
  return e;
}

inline bool gibbs_window_fits(const Envelope &e) { return e.ascending && e.rows > 0 && e.rows <= kGibbsWindowRows; }

}  // namespace gibbs
}  // namespace bsn
