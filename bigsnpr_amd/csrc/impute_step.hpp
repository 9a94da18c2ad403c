// impute_step.hpp — what snp_fastImputeSimple writes at the missing positions of one variant (src/impute-simple.cpp:44-69 of
// the reference): the `mode` rule with its ties, the two rounded means, the draw of `random`, the byte the FBM receives and
// the rewrite of one dword of sixteen 2-bit fields.  Shared by the kernels (impute.hip), the CPU statement
// (tests/native/impute_ref.cpp) and the stand-alone check (tests/native/impute_check.cpp): the three cannot drift apart.
//
// Bit equality of host and device.  Everything is integer arithmetic except the two means and the allele frequency: one
// fp64 division (correctly rounded on both sides), for `mean2` one fp64 multiplication by 100 that is never contracted
// with anything (the pragma below on the device, -ffp-contract=off on the host), and a round-to-nearest-even.  The
// rounding is pinned to these double operations, as the reference performs them, and NOT to the exact rational:
// 100 * (23.0 / 40) is 57.49999999999999 and rounds to 57 where 2300 / 40 = 57.5 would round to 58.
#pragma once
#include <stdint.h>

#include <cmath>

#include "gibbs_step.hpp"

#if defined(__HIPCC__)
#define BSN_IMPUTE_HD __host__ __device__ __forceinline__
#else
#define BSN_IMPUTE_HD inline
#endif

namespace bsn {
namespace impute {

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// `method` of bsn_impute_simple: the reference's numbers (R/impute.R:199) plus 0
constexpr int kZero = 0, kMode = 1, kMean0 = 2, kMean2 = 3, kRandom = 4;

// third word of the Philox counter of every draw of this function ("IMPS")
constexpr uint32_t kCounterTag = 0x494D5053u;

// Rf_fround(x, 0) is R's private_rint: nearbyint under the default rounding mode, ties to even
BSN_IMPUTE_HD double round_even(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return ::rint(x);
#else
  return std::nearbyint(x);
#endif
}

// src/impute-simple.cpp:52-56: the most frequent call, ties to the smaller one
BSN_IMPUTE_HD int mode_call(int64_t c0, int64_t c1, int64_t c2) {
  int v = 0;
  if (c1 > c0) v = 1;
  if (v == 0 && c2 > c0) v = 2;
  if (v == 1 && c2 > c1) v = 2;
  return v;
}

// What a variant with c1 calls 1, c2 calls 2 and c non-missing calls (over all samples) receives.
//   val: the call 0 / 1 / 2 (zero, mode, mean0), r = 0 .. 200 with value r / 100 (mean2), 0 (random: see af);
//        -1: the variant has no observed call and stays missing (mean0, mean2, random: the reference casts a NaN to
//        unsigned char there; its `mode` gives 0, and so does this)
//   af:  allele frequency of `random`, line 48 (0 otherwise)
struct Rule {
  int32_t val;
  double af;
};

BSN_IMPUTE_HD Rule rule(int method, int64_t c1, int64_t c2, int64_t c) {
  Rule r;
  r.val = 0;
  r.af = 0.0;
  if (method == kZero) return r;
  if (method == kMode) {
    r.val = mode_call(c - (c1 + c2), c1, c2);
    return r;
  }
  if (c <= 0) {
    r.val = -1;
    return r;
  }
  if (method == kRandom) {
    r.af = (0.5 * (double)c1 + (double)c2) / (double)c;
    return r;
  }
  const double mean = ((double)c1 + 2.0 * (double)c2) / (double)c;
  if (method == kMean0) {
    r.val = (int32_t)round_even(mean);
  } else {
    const double h = 100 * mean;
    r.val = (int32_t)round_even(h);
  }
  return r;
}

// `random`: the call drawn for sample i of variant j — Binomial(2, af) as the sum of two uniform comparisons.  One Philox
// call: key = seed, counter = (i, j, tag, high halves of i and j).  Nothing else enters: not the launch geometry, not
// the other missing positions, not whether the FBM bytes were asked for.
BSN_IMPUTE_HD int draw(uint64_t seed, uint64_t i, uint64_t j, double af) {
  const gibbs::Philox o = gibbs::philox4x32_10((uint32_t)i, (uint32_t)j, kCounterTag,
                                               (uint32_t)(i >> 32) ^ ((uint32_t)(j >> 32) << 16), (uint32_t)seed,
                                               (uint32_t)(seed >> 32));
  const double u0 = gibbs::unit_open(o.v[0], o.v[1]), u1 = gibbs::unit_open(o.v[2], o.v[3]);
  return (int)(u0 < af) + (int)(u1 < af);
}

// the byte the reference's file holds at an imputed position: 4 + call (CODE_IMPUTE_PRED), 7 + r (CODE_DOSAGE), or the
// missing code 3 where nothing was written (`zero`, which only changes the decode table, and variants left missing)
BSN_IMPUTE_HD uint8_t fbm_byte(int method, int32_t val) {
  if (method == kZero || val < 0) return 3;
  return (uint8_t)((method == kMean2 ? 7 : 4) + val);
}

// the int8 grid index of the CODE_DOSAGE image (v_off = 1, v_step = 0.01) at an imputed position; -128 = missing
BSN_IMPUTE_HD int8_t grid_index(int32_t val) { return (int8_t)(val < 0 ? -128 : val - 100); }

// ---- one dword = sixteen 2-bit fields in the device coding (0, 1, 2 = call, 3 = missing) --------------------------------
// bit 2 e set iff field e is missing
BSN_IMPUTE_HD uint32_t missing_mask(uint32_t x) { return x & (x >> 1) & 0x55555555u; }
// every missing field -> call v (0 .. 2); the other fields, pad fields (zero) among them, stay
BSN_IMPUTE_HD uint32_t fill_word(uint32_t x, uint32_t v) {
  const uint32_t m = missing_mask(x);
  return (x & ~(3u * m)) | (v * m);
}
// `random`: a draw for every missing field; i0 = sample of field 0
BSN_IMPUTE_HD uint32_t fill_word_random(uint32_t x, uint64_t seed, uint64_t i0, uint64_t j, double af) {
  uint32_t m = missing_mask(x), out = x & ~(3u * m);
  while (m) {
    const int b = __builtin_ctz(m);
    out |= (uint32_t)draw(seed, i0 + (uint64_t)(b >> 1), j, af) << b;
    m &= m - 1;
  }
  return out;
}

#if defined(__clang__)
#pragma clang fp contract(on)
#endif

}  // namespace impute
}  // namespace bsn
