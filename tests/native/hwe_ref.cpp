// hwe_ref.cpp — the CPU statement of the exact Hardy–Weinberg test and the QC comparisons over
// bigsnpr_amd/csrc/hwe_step.hpp, the header the kernels of qc.hip compile from.  Built by hwe_ref.py with
// -ffp-contract=off -fopenmp.
#include <stdint.h>

#include "hwe_step.hpp"

using namespace bsn::hwe;

extern "C" {

// counts: 3 x m (hom1, het, hom2 of variant j at 3 j).  p (m); steps (m, may be NULL): the terms the two walks formed.
void hwe_ref_exact(const int32_t *counts, int64_t m, int midp, double *p, int64_t *steps) {
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t j = 0; j < m; j++) {
    int64_t st = 0;
    p[j] = hwe_exact(counts[3 * j], counts[3 * j + 1], counts[3 * j + 2], midp != 0, &st);
    if (steps) steps[j] = st;
  }
}

// the two walks of one variant on their own: out = total_down, tail_down, total_up, tail_up
void hwe_ref_walks(int32_t hom1, int32_t het, int32_t hom2, int midp, double *out) {
  const Start s = start(hom1, het, hom2);
  const Walk d = walk_down(s.het, s.homr, s.homc, midp != 0), u = walk_up(s.het, s.homr, s.homc, s.rare, midp != 0);
  out[0] = d.total, out[1] = d.tail, out[2] = u.total, out[3] = u.tail;
}

int hwe_ref_too_many_missing(int64_t na, int64_t of, double rate) { return too_many_missing(na, of, rate) ? 1 : 0; }
double hwe_ref_missing_rate(int64_t na, int64_t of) { return missing_rate(na, of); }
double hwe_ref_maf(int64_t c0, int64_t c1, int64_t c2) { return maf_from_counts(c0, c1, c2); }
int hwe_ref_maf_too_low(double maf_j, double maf) { return maf_too_low(maf_j, maf) ? 1 : 0; }
int hwe_ref_rejected(double p, double hwe) { return hwe_rejected(p, hwe) ? 1 : 0; }

}  // extern "C"
