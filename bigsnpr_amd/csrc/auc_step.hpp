// auc_step.hpp — what AUC and AUCBoot compute, stated once for the kernels (auc.hip) and for the CPU statement
// (tests/native/auc_ref.cpp): the two cannot drift apart.  DESIGN.md 3.5t.
//
// The definition.  `pred` holds n scores, `target` a 0 / 1 per row; n1 rows are cases (1), n0 controls (0).  Over the pairs
// (case i, control j)
//     twoU = 2 #{x_i > x_j} + #{x_i = x_j}                        (a uint64: at most 2 n1 n0 <= n^2 / 2 < 2^61 for n < 2^31)
//     AUC  = (double)twoU / (2.0 * (double)n1 * (double)n0)       (three conversions, one product of exact integers below
//                                                                  2^62 rounded once, one product by 2, one division)
// -0.0 ties with +0.0, +-Inf are ordinary values, a NaN is refused before anything is computed.
//
// How it is evaluated.  The scores are mapped to 64-bit keys whose unsigned order is the order of the doubles (order_key),
// the keys are sorted, equal keys form a tie group, groups are numbered 0 .. G-1 in ascending order, and with
// (c0_g, c1_g) the controls and cases of group g
//     twoU = sum_g c1_g (2 sum_{h<g} c0_h + c0_g).
// Everything is an integer: the order of additions is immaterial and device, statement and definition agree bit for bit.
//
// The bootstrap.  Replicate b of a call with seed s draws n rows with replacement: draw t (0 <= t < n) is
//     word (t & 3) of philox4x32_10(t >> 2, b, kDrawTag, 0, s_lo, s_hi),        row = ((uint64)word * n) >> 32.
// The draws depend on (t, b, s, n) alone — not on the column, so all columns of a call see the same resamples and the
// difference of two models' AUCs is paired — and R's sample() is NOT emulated.  A replicate's value is the definition above
// on the resampled vectors, i.e. with counts (c0_g, c1_g) of the DRAWN rows per tie group of the original column: the
// histogram a replicate accumulates at index 2 g + y.  A replicate without a case or without a control is NaN.
// The multiply-shift maps 2^32 words onto n rows, so a row's probability is off 1/n by at most 2^-32: for n = 10^6 a
// relative 2.3e-4 of 1/n, four orders below the bootstrap's own noise at any nboot that fits in memory.
#pragma once
#include <stdint.h>

#include "gibbs_step.hpp"

namespace bsn {
namespace auc {

constexpr uint32_t kDrawTag = 0x41554342u;   // "AUCB": counter word 2 of every draw; no other consumer of philox4x32_10 uses it
constexpr int64_t kMaxRows = ((int64_t)1 << 31) - 1;
constexpr int kMaxCovar = 31;                // columns of [1, z] that pcor takes (one lane-private accumulator each)
constexpr int64_t kPcorSlabRows = 4096;      // rows of one slab of the two pcor passes: fixed, so the sums do not depend on the grid

// The unsigned order of the keys is the order of the doubles; -0.0 and +0.0 share a key.  Not for a NaN (is_nan first).
BSN_GIBBS_HD uint64_t order_key(double x) {
  uint64_t b = gibbs::to_bits(x);
  if ((b << 1) == 0) b = 0;                                  // -0.0 -> +0.0
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

BSN_GIBBS_HD bool is_nan(double x) { return x != x; }

// the value of one column or replicate from its exact counts
BSN_GIBBS_HD double value(uint64_t twoU, uint64_t n1, uint64_t n0) {
  if (n1 == 0 || n0 == 0) return gibbs::from_bits(0x7ff8000000000000ull);
  return (double)twoU / (2.0 * ((double)n1 * (double)n0));
}

// row of draw t of replicate b
BSN_GIBBS_HD uint32_t row_of_word(uint32_t word, uint32_t n) { return (uint32_t)(((uint64_t)word * n) >> 32); }

BSN_GIBBS_HD gibbs::Philox draw_words(uint32_t t_over_4, uint32_t b, uint64_t seed) {
  return gibbs::philox4x32_10(t_over_4, b, kDrawTag, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

BSN_GIBBS_HD uint32_t draw_row(uint32_t t, uint32_t b, uint64_t seed, uint32_t n) {
  return row_of_word(draw_words(t >> 2, b, seed).v[t & 3], n);
}

// One group's term of twoU, given the controls before it.
BSN_GIBBS_HD uint64_t group_term(uint64_t c0_before, uint64_t c0, uint64_t c1) { return c1 * (2 * c0_before + c0); }

// twoU, n1, n0 from a histogram hist[2 g + y], g < G, in ascending group order (the serial form of the kernels' prefix sum)
inline void eval_hist(const uint32_t *hist, int64_t G, uint64_t *twoU, uint64_t *n1, uint64_t *n0) {
  uint64_t before = 0, u = 0, c1s = 0;
  for (int64_t g = 0; g < G; g++) {
    const uint64_t c0 = hist[2 * g], c1 = hist[2 * g + 1];
    u += group_term(before, c0, c1);
    before += c0;
    c1s += c1;
  }
  *twoU = u, *n1 = c1s, *n0 = before;
}

}  // namespace auc
}  // namespace bsn
