// bgen_ref.cpp — the CPU statement of what bsn_bgen_read makes of inflated probabilities: bgen_step.hpp, the header the
// kernels of bgen.hip are compiled from.  tests/native/bgen_ref.py builds it with -ffp-contract=off.
#include <stdint.h>

#include "bgen_step.hpp"

using namespace bsn::bgen;

extern "C" {

int bgen_table_byte(int k) { return table_byte(k); }
int bgen_grid_of_byte(int b) { return grid_of_byte((uint8_t)b); }
double bgen_unit(uint64_t seed, uint64_t i, uint64_t j) { return unit(seed, i, j); }
int bgen_random_call(double u, int p0, int p1) { return random_call(u, p0, p1); }
void bgen_info_freq(int64_t nona, int64_t af, int64_t num, double *out) {
  const InfoFreq r = info_freq(nona, af, num);
  out[0] = r.info;
  out[1] = r.freq;
}

// one inflated block (10 + 3 N bytes) -> the FBM bytes of the rows ind_row[0 .. n) and the three sums of the variant
void bgen_variant_ref(const uint8_t *block, int64_t N, const int64_t *ind_row, int64_t n, const uint8_t *decode, int dosage,
                      uint64_t seed, int64_t col, uint8_t *bytes, int64_t *sums) {
  int64_t nona = 0, af = 0, num = 0;
  for (int64_t i = 0; i < n; i++) {
    const int64_t ig = ind_row[i];
    uint8_t fb = 3;
    if (block[ploidy_at(ig)] < 0x80) {
      const int p0 = block[prob_at(N, ig)], p1 = block[prob_at(N, ig) + 1];
      nona++;
      af += af_term(p0, p1);
      num += num_term(p0, p1);
      fb = dosage ? decode[2 * p0 + p1] : (uint8_t)(4 + random_call(unit(seed, (uint64_t)i, (uint64_t)col), p0, p1));
    }
    bytes[i] = fb;
  }
  sums[0] = nona, sums[1] = af, sums[2] = num;
}

}  // extern "C"
