// king_ref.cpp — the CPU statement of bed_king: plain loops over decoded genotypes, the pair through king_step.hpp (the
// header the kernels of bigsnpr_amd/csrc/king.hip use).  Built by king_ref.py with -ffp-contract=off -fopenmp.
#include <stdint.h>

#include <cstddef>
#include <vector>

#include "king_step.hpp"

using namespace bsn::king;

extern "C" {

// G: n x m row-major codes (0, 1, 2 = allele count, 3 = missing).  Every pair i < j in the order (i, j): row k of the
// table at counts[5 k ..] (NSNP, HETHET, IBS0, HET1HOM2, HET2HOM1), kinship[k], i1[k], i2[k].
void king_table(const int8_t *G, int64_t n, int64_t m, int32_t *i1, int32_t *i2, int32_t *counts, double *kinship) {
  std::vector<int64_t> first((std::size_t)n);   // row of the pair (i, i + 1)
  int64_t at = 0;
  for (int64_t i = 0; i < n; i++) {
    first[(std::size_t)i] = at;
    at += n - 1 - i;
  }
#pragma omp parallel for schedule(dynamic, 4)
  for (int64_t i = 0; i < n; i++) {
    const int8_t *gi = G + i * m;
    for (int64_t j = i + 1; j < n; j++) {
      const int8_t *gj = G + j * m;
      Sums s = {0, 0, 0, 0, 0, 0, 0};
      for (int64_t v = 0; v < m; v++) {
        const int a = gi[v], b = gj[v];
        if (a == 3 || b == 3) continue;
        s.xx += a * b;
        s.hh += (a == 1) && (b == 1);
        s.xP += a;
        s.x2P += a * a;
        s.Px += b;
        s.Px2 += b * b;
        s.PP += 1;
      }
      const Pair p = pair_from_sums(s);
      const int64_t k = first[(std::size_t)i] + (j - i - 1);
      i1[k] = (int32_t)i;
      i2[k] = (int32_t)j;
      counts[5 * k] = p.nsnp;
      counts[5 * k + 1] = p.hethet;
      counts[5 * k + 2] = p.ibs0;
      counts[5 * k + 3] = p.het1hom2;
      counts[5 * k + 4] = p.het2hom1;
      kinship[k] = p.kinship;
    }
  }
}

// the filter of the header over a kinship column: keep[k] = 1 where the row passes
void king_filter(const double *kinship, int64_t count, double thr, uint8_t *keep) {
  for (int64_t k = 0; k < count; k++) keep[k] = passes(kinship[k], thr) ? 1 : 0;
}

}  // extern "C"
