// bgen_step.hpp — what snp_readBGEN / snp_prodBGEN make of the inflated probabilities of one sample of one variant
// (src/read-bgen.cpp:49-75 and src/prod-bgen.cpp:48-62 of the reference): the table rule of the dosages, the draw of
// read_as = "random", the map of an FBM byte of CODE_DOSAGE onto the int8 grid image, and the INFO score / allele
// frequency of a variant from its three exact integer sums.  Shared by the kernels (bgen.hip) and the CPU statement
// (tests/native/bgen_ref.cpp): the two cannot drift apart.
//
// Bit equality of host and device: the sums are integers; info and freq are a handful of fp64 products, one difference
// and one division each, in the reference's order, never contracted (the pragma below on the device, -ffp-contract=off
// on the host).
#pragma once
#include <stdint.h>

#include "gibbs_step.hpp"

#if defined(__HIPCC__)
#define BSN_BGEN_HD __host__ __device__ __forceinline__
#else
#define BSN_BGEN_HD inline
#endif

namespace bsn {
namespace bgen {

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// third word of the Philox counter of every draw of these functions ("BGEN")
constexpr uint32_t kCounterTag = 0x4247454Eu;
constexpr int kTable = 511;          // 2 p0 + p1 = 0 .. 510
constexpr int kMaxFbmByte = 207;     // the last byte of CODE_DOSAGE that decodes to a value (2.00)

// an inflated block of one variant (layout 2, 8 bits, two alleles, unphased): 8 bytes of counts, N ploidy bytes
// (bit 7 = missing), 2 bytes (phased, bits), then p0, p1 of every sample as bytes = probability * 255
BSN_BGEN_HD int64_t ploidy_at(int64_t i) { return 8 + i; }
BSN_BGEN_HD int64_t prob_at(int64_t N, int64_t i) { return 10 + N + 2 * i; }

// the reference's table: FBM byte of dosage k / 255 (k = 2 p0 + p1 counts the FIRST allele), rounded to 2 decimals and
// turned round — 207 - round(k * 100 / 255); no k is a tie (R/read-bgen.R:206)
BSN_BGEN_HD uint8_t table_byte(int k) { return (uint8_t)(207 - (k * 200 + 255) / 510); }

// u in (0, 1) for (position in ind_row, global column): one Philox call, nothing else enters
BSN_BGEN_HD double unit(uint64_t seed, uint64_t i, uint64_t j) {
  const gibbs::Philox o = gibbs::philox4x32_10((uint32_t)i, (uint32_t)j, kCounterTag,
                                               (uint32_t)(i >> 32) ^ ((uint32_t)(j >> 32) << 16), (uint32_t)seed,
                                               (uint32_t)(seed >> 32));
  return gibbs::unit_open(o.v[0], o.v[1]);
}

// src/read-bgen.cpp:11-14: the hard call 0 / 1 / 2 drawn from (p0, p1, 255 - p0 - p1) / 255
BSN_BGEN_HD int random_call(double u, int p0, int p1) {
  const double first = u * 255 - p0;
  return first < 0 ? 0 : (first < p1 ? 1 : 2);
}

// FBM byte of CODE_DOSAGE -> int8 grid index about 1.00 in steps of 0.01 (what bsn_fbm_open makes of the same byte):
// 0, 1, 2 and 4, 5, 6 are calls, 7 .. 207 are 0.00 .. 2.00, everything else is missing (-128)
BSN_BGEN_HD int8_t grid_of_byte(uint8_t b) {
  if (b < 3) return (int8_t)(100 * (int)b - 100);
  if (b >= 4 && b <= 6) return (int8_t)(100 * ((int)b - 4) - 100);
  if (b >= 7 && b <= kMaxFbmByte) return (int8_t)((int)b - 107);
  return (int8_t)-128;
}

// what one non-missing sample adds to the sums of its variant
BSN_BGEN_HD int64_t af_term(int p0, int p1) { return 2 * p0 + p1; }
BSN_BGEN_HD int64_t num_term(int p0, int p1) {
  const int64_t e = 2 * p0 + p1, f = 4 * p0 + p1;
  return 255 * f - e * e;
}

// src/read-bgen.cpp:72-75, operation by operation (https://doi.org/10.1038/nrg2796); nona == 0 gives NaN twice
struct InfoFreq {
  double info, freq;
};
BSN_BGEN_HD InfoFreq info_freq(int64_t nona, int64_t af_sum, int64_t num_sum) {
  const double af = (double)af_sum, num = (double)num_sum, dn = (double)nona;
  const double coef = 255 * (2 * dn);
  InfoFreq r;
  const double top = num * 2 * dn;
  const double bottom = af * (coef - af);
  r.info = 1 - top / bottom;
  r.freq = 1 - af / coef;
  return r;
}

#if defined(__clang__)
#pragma clang fp contract(on)
#endif

}  // namespace bgen
}  // namespace bsn
