// impute_ref.cpp — the CPU statement of snp_fastImputeSimple over bigsnpr_amd/csrc/impute_step.hpp: the loop of the
// reference (count, decide, rewrite every missing position) on an FBM's bytes, with the rules, the rounding and the draw
// of the header the kernels compile from.  Built by impute_ref.py with -ffp-contract=off.
#include <stdint.h>

#include "impute_step.hpp"

using namespace bsn::impute;

extern "C" {

// bytes: n x m column-major, 0 / 1 / 2 = call, anything else = missing (CODE_012).  out: the FBM's bytes afterwards (calls
// as they were, 4 + call / 7 + r / 3 at the missing positions).  val (m, may be NULL): the rule's value per variant.
// Returns the number of variants without any call.
int64_t impute_simple_ref(const uint8_t *bytes, int64_t n, int64_t m, int method, uint64_t seed, uint8_t *out, int32_t *val,
                          int nthreads) {
  int64_t n_all = 0;
#if defined(_OPENMP)
#pragma omp parallel for schedule(static) reduction(+ : n_all) num_threads(nthreads > 0 ? nthreads : 1)
#endif
  for (int64_t j = 0; j < m; j++) {
    const uint8_t *col = bytes + j * n;
    uint8_t *dst = out + j * n;
    int64_t c1 = 0, c2 = 0, c = n;
    for (int64_t i = 0; i < n; i++) {
      const uint8_t g = col[i];
      if (g == 1) c1++;
      else if (g == 2) c2++;
      else if (g != 0) c--;
    }
    const Rule r = rule(method, c1, c2, c);
    if (val) val[j] = r.val;
    if (c == 0) n_all++;
    for (int64_t i = 0; i < n; i++) {
      const uint8_t g = col[i];
      if (g <= 2) dst[i] = g;
      else dst[i] = fbm_byte(method, method == kRandom && r.val >= 0 ? draw(seed, (uint64_t)i, (uint64_t)j, r.af) : r.val);
    }
  }
  return n_all;
}

// the pieces, for the tests of the rules
int32_t impute_rule_val(int method, int64_t c1, int64_t c2, int64_t c) { return rule(method, c1, c2, c).val; }
double impute_rule_af(int64_t c1, int64_t c2, int64_t c) { return rule(kRandom, c1, c2, c).af; }
int impute_draw(uint64_t seed, uint64_t i, uint64_t j, double af) { return draw(seed, i, j, af); }

}  // extern "C"
