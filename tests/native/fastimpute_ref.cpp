// fastimpute_ref.cpp — the CPU statement of snp_fastImpute over bigsnpr_amd/csrc/fastimpute_step.hpp: a plain loop over
// targets, rounds, levels, features and samples on an FBM's bytes, with the roles, gradients, candidate scan and leaf
// weights of the header the kernels compile from.  Built by fastimpute_ref.py with -O2 -ffp-contract=off (OpenMP over
// targets when the compiler has it); fastimpute_check.cpp includes this file to run it under a sanitizer.
#include <stdint.h>

#include <cmath>
#include <limits>
#include <vector>

#include "fastimpute_step.hpp"

using namespace bsn::fimp;

namespace {

// one target: col = its n bytes, feat(f) = the n bytes of predictor f.  dst receives col with 4 + call at the missing
// positions; returns the share of validation samples whose call differs from the observed one (NaN without any).
// trace (may be NULL): feat, t, dir of the 31 nodes of the first round's tree (feat -1 = leaf, -2 = absent).
double one_target(const uint8_t *bytes, int64_t n, int64_t j, const int32_t *P, int64_t np, double p_train, uint64_t seed,
                  uint8_t *dst, int32_t *trace) {
  const uint8_t *col = bytes + j * n;
  std::vector<int> role((size_t)n);
  int64_t T = 0;
  for (int64_t i = 0; i < n; i++) {
    role[(size_t)i] = col[i] > 2 ? kFill : draws_train(seed, (uint64_t)i, (uint64_t)j, p_train) ? kTrain : kValid;
    T += role[(size_t)i] == kTrain;
  }
  if (T == 0)
    for (int64_t i = 0; i < n; i++)
      if (role[(size_t)i] == kValid) role[(size_t)i] = kTrain, T++;
  int64_t c1 = 0, c2 = 0;
  for (int64_t i = 0; i < n; i++)
    if (role[(size_t)i] == kTrain) c1 += col[i] == 1, c2 += col[i] == 2;
  std::vector<double> margin((size_t)n, start_margin(c1, c2, T));
  std::vector<int32_t> gq((size_t)n, 0), hq((size_t)n, 0);
  std::vector<int> node((size_t)n);

  for (int round = 0; round < kRounds; round++) {
    int32_t feat[kNodes], thr[kNodes], dir[kNodes];
    int64_t G[kNodes], H[kNodes];
    double w[kNodes];
    for (int k = 0; k < kNodes; k++) feat[k] = -2, thr[k] = dir[k] = 0, G[k] = H[k] = 0, w[k] = 0.0;
    feat[0] = -1;
    for (int64_t i = 0; i < n; i++) {
      node[(size_t)i] = 0;
      if (role[(size_t)i] != kTrain) continue;
      grad(margin[(size_t)i], col[i], &gq[(size_t)i], &hq[(size_t)i]);
      G[0] += gq[(size_t)i];
      H[0] += hq[(size_t)i];
    }
    for (int level = 0; level <= kMaxDepth; level++) {
      const int first = (1 << level) - 1, cnt = 1 << level;
      if (level < kMaxDepth) {
        std::vector<Best> best((size_t)cnt, no_split());
        for (int64_t f = 0; f < np; f++) {
          const uint8_t *x = bytes + (int64_t)P[f] * n;
          std::vector<int64_t> gc((size_t)cnt * 4, 0), hc((size_t)cnt * 4, 0);
          for (int64_t i = 0; i < n; i++) {
            const int k = node[(size_t)i] - first;
            if (role[(size_t)i] != kTrain || k < 0) continue;
            const int c = x[i] > 2 ? 3 : x[i];
            gc[(size_t)(4 * k + c)] += gq[(size_t)i];
            hc[(size_t)(4 * k + c)] += hq[(size_t)i];
          }
          for (int k = 0; k < cnt; k++)
            if (feat[first + k] == -1) scan_feature(&gc[(size_t)(4 * k)], &hc[(size_t)(4 * k)], G[first + k], H[first + k], (int32_t)f, &best[(size_t)k]);
        }
        for (int k = 0; k < cnt; k++) {
          const int id = first + k;
          const Best &b = best[(size_t)k];
          if (feat[id] != -1 || b.feat < 0) continue;
          feat[id] = b.feat, thr[id] = b.t, dir[id] = b.dir;
          feat[2 * id + 1] = feat[2 * id + 2] = -1;
          G[2 * id + 1] = b.GL, H[2 * id + 1] = b.HL;
          G[2 * id + 2] = G[id] - b.GL, H[2 * id + 2] = H[id] - b.HL;
        }
        for (int64_t i = 0; i < n; i++) {
          const int id = node[(size_t)i];
          if (id < first || feat[id] < 0) continue;
          const uint8_t x = bytes[(int64_t)P[feat[id]] * n + i];
          node[(size_t)i] = goes_left(x > 2 ? 3 : x, thr[id], dir[id]) ? 2 * id + 1 : 2 * id + 2;
        }
      }
      for (int k = 0; k < cnt; k++)
        if (feat[first + k] == -1) w[first + k] = leaf_weight(G[first + k], H[first + k]);
    }
    for (int64_t i = 0; i < n; i++) margin[(size_t)i] += w[node[(size_t)i]];
    if (trace && round == 0)
      for (int k = 0; k < kNodes; k++) trace[3 * k] = feat[k], trace[3 * k + 1] = thr[k], trace[3 * k + 2] = dir[k];
  }

  int64_t nval = 0, nerr = 0;
  for (int64_t i = 0; i < n; i++) {
    const int call = call_of(margin[(size_t)i]);
    if (role[(size_t)i] == kFill) {
      dst[i] = (uint8_t)(4 + call);
    } else {
      dst[i] = col[i];
      if (role[(size_t)i] == kValid) nval++, nerr += call != col[i];
    }
  }
  return nval ? (double)nerr / (double)nval : std::numeric_limits<double>::quiet_NaN();
}

}  // namespace

extern "C" {

// bytes: n x m column-major, 0 / 1 / 2 = call, anything else = missing (CODE_012).  pred_off (m + 1) / pred_idx: the
// predictor list of every variant.  out: the FBM's bytes afterwards (4 + call at an imputed position, 3 where a variant
// has no observed call).  infos: 2 x m row-major.  trace (may be NULL): 31 x 3 per variant, see one_target.  Returns the
// number of variants without any observed call.
int64_t fast_impute_ref(const uint8_t *bytes, int64_t n, int64_t m, const int64_t *pred_off, const int32_t *pred_idx,
                        double p_train, uint64_t seed, uint8_t *out, double *infos, int32_t *trace, int nthreads) {
  int64_t n_all = 0;
#if defined(_OPENMP)
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : n_all) num_threads(nthreads > 0 ? nthreads : 1)
#endif
  for (int64_t j = 0; j < m; j++) {
    const uint8_t *col = bytes + j * n;
    uint8_t *dst = out + j * n;
    int64_t miss = 0;
    for (int64_t i = 0; i < n; i++) miss += col[i] > 2;
    infos[j] = (double)miss / (double)n;
    infos[m + j] = std::numeric_limits<double>::quiet_NaN();
    if (miss == 0 || miss == n) {
      for (int64_t i = 0; i < n; i++) dst[i] = col[i] > 2 ? 3 : col[i];
      n_all += miss == n;
      continue;
    }
    infos[m + j] = one_target(bytes, n, j, pred_idx + pred_off[j], pred_off[j + 1] - pred_off[j], p_train, seed, dst,
                              trace ? trace + j * 3 * kNodes : nullptr);
  }
  return n_all;
}

}  // extern "C"
