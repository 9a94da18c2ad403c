// The CPU statement of AUC / AUCBoot over bigsnpr_amd/csrc/auc_step.hpp (the header the kernels of auc.hip are compiled
// from): keys, a plain sort, tie groups, the histogram at 2 gid + y, auc::eval_hist.  Built by auc_ref.py as a shared
// library for the tests and tools/probe_auc.py, and included by auc_check.cpp (the sanitizer program).
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "auc_step.hpp"

namespace twin {

// code[row] = 2 gid + y[row] of one column; returns the number of tie groups, or -1 for a NaN
inline int64_t codes(const double *x, int64_t n, const uint8_t *y, std::vector<uint32_t> &code) {
  std::vector<std::pair<uint64_t, uint32_t>> kv((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    if (bsn::auc::is_nan(x[i])) return -1;
    kv[(size_t)i] = {bsn::auc::order_key(x[i]), (uint32_t)i};
  }
  std::sort(kv.begin(), kv.end());
  code.assign((size_t)n, 0u);
  int64_t g = 0;
  for (int64_t p = 0; p < n; p++) {
    if (p > 0 && kv[(size_t)p].first != kv[(size_t)p - 1].first) g++;
    code[kv[(size_t)p].second] = (uint32_t)(2 * g) + y[kv[(size_t)p].second];
  }
  return n > 0 ? g + 1 : 0;
}

inline void column(const std::vector<uint32_t> &code, int64_t G, uint64_t out[3]) {
  std::vector<uint32_t> hist((size_t)(2 * G), 0u);
  for (uint32_t c : code) hist[c]++;
  bsn::auc::eval_hist(hist.data(), G, out, out + 1, out + 2);
}

inline void replicate(const std::vector<uint32_t> &code, int64_t G, uint32_t b, uint64_t seed, std::vector<uint32_t> &hist,
                      uint64_t out[3]) {
  const uint32_t n = (uint32_t)code.size();
  hist.assign((size_t)(2 * G), 0u);
  for (uint32_t t = 0; t < n; t++) hist[code[bsn::auc::draw_row(t, b, seed, n)]]++;
  bsn::auc::eval_hist(hist.data(), G, out, out + 1, out + 2);
}

}  // namespace twin

extern "C" {

// counts: (twoU, n1, n0) per column; returns -1, or the first column that holds a NaN
int64_t auc_twin(const double *x, int64_t ld, int64_t n, int64_t K, const uint8_t *y, uint64_t *counts, double *auc) {
  int64_t bad = K;
#pragma omp parallel for schedule(dynamic, 1) reduction(min : bad)
  for (int64_t j = 0; j < K; j++) {
    std::vector<uint32_t> code;
    const int64_t G = twin::codes(x + j * ld, n, y, code);
    if (G < 0) {
      bad = std::min(bad, j);
      continue;
    }
    twin::column(code, G, counts + 3 * j);
    auc[j] = bsn::auc::value(counts[3 * j], counts[3 * j + 1], counts[3 * j + 2]);
  }
  return bad < K ? bad : -1;
}

void auc_draws(int64_t n, int64_t b, uint64_t seed, int32_t *rows) {
  for (int64_t t = 0; t < n; t++) rows[t] = (int32_t)bsn::auc::draw_row((uint32_t)t, (uint32_t)b, seed, (uint32_t)n);
}

// rep: nboot x K, column-major
int64_t auc_boot_twin(const double *x, int64_t ld, int64_t n, int64_t K, const uint8_t *y, int64_t nboot, uint64_t seed, double *rep) {
  for (int64_t j = 0; j < K; j++) {
    std::vector<uint32_t> code;
    const int64_t G = twin::codes(x + j * ld, n, y, code);
    if (G < 0) return j;
#pragma omp parallel
    {
      std::vector<uint32_t> hist;
#pragma omp for schedule(dynamic, 4)
      for (int64_t b = 0; b < nboot; b++) {
        uint64_t out[3];
        twin::replicate(code, G, (uint32_t)b, seed, hist, out);
        rep[j * nboot + b] = bsn::auc::value(out[0], out[1], out[2]);
      }
    }
  }
  return -1;
}

uint64_t auc_order_key(double x) { return bsn::auc::order_key(x); }
uint32_t auc_draw_tag(void) { return bsn::auc::kDrawTag; }

}  // extern "C"
