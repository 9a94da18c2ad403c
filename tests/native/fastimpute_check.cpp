// fastimpute_check.cpp — a stand-alone program over fastimpute_step.hpp and the CPU statement (fastimpute_ref.cpp, included
// below): the pieces of the rule (routing, admissibility, the tie between equal candidates, the quantised gradients at
// extreme margins) and a few hundred small random cases with sample counts that are no multiple of 4, empty and
// repeated predictor lists, variants without a missing or without an observed call.  Meant to be compiled with
// -fsanitize=address,undefined and run as a program (tests/test_fastimpute_cpu.py does both).  Exit status 0 = every
// check held.
#include <stdio.h>

#include <cmath>
#include <vector>

#include "fastimpute_ref.cpp"

static int failures = 0;
#define CHECK(cond)                                          \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAILED line %d: %s\n", __LINE__, #cond);       \
      failures++;                                            \
    }                                                        \
  } while (0)

static void pieces() {
  CHECK(goes_left(0, 0, 0) && !goes_left(1, 0, 0) && goes_left(1, 1, 0) && goes_left(2, 2, 1));
  CHECK(!goes_left(3, 2, 0) && goes_left(3, 0, 1));
  CHECK(kNodes == 31 && kLevelNodes == 8);
  int32_t g, h;
  grad(800.0, 0, &g, &h);   // p = 1: the hessian's floor is one unit
  CHECK(g == (int32_t)kQuant && h == 1);
  grad(-800.0, 2, &g, &h);
  CHECK(g == -(int32_t)kQuant && h == 1);
  grad(0.0, 1, &g, &h);
  CHECK(g == 0 && h == (int32_t)(kQuant / 4));
  CHECK(call_of(-800.0) == 0 && call_of(0.0) == 1 && call_of(800.0) == 2);
  CHECK(start_margin(0, 0, 5) < -16.0 && start_margin(0, 5, 5) > 16.0 && start_margin(0, 1, 2) == 0.0);

  const int64_t one = (int64_t)kQuant;
  // two features with the same sums: the first keeps the split
  const int64_t gc[4] = {-3 * one, 3 * one, 0, 0}, hc[4] = {2 * one, 2 * one, 0, 0};
  Best b = no_split();
  scan_feature(gc, hc, 0, 4 * one, 0, &b);
  CHECK(b.feat == 0 && b.t == 0 && b.dir == 0 && b.GL == -3 * one && b.HL == 2 * one);
  const Best first = b;
  scan_feature(gc, hc, 0, 4 * one, 1, &b);
  CHECK(b.feat == 0 && b.chg == first.chg);
  Best c = no_split();
  scan_feature(gc, hc, 0, 4 * one, 1, &c);
  CHECK(c.feat == 1 && !better(c, first));
  // a child below min_child_weight: no candidate is admissible
  const int64_t hs[4] = {one - 1, 3 * one, 0, 0};
  b = no_split();
  scan_feature(gc, hs, 0, 4 * one - 1, 0, &b);
  CHECK(b.feat == -1);
  // missing exactly where the gradient differs: t = 2.5 with missing to the right is the first to separate them
  const int64_t gm[4] = {one, one, one, -3 * one}, hm[4] = {one, one, one, 3 * one};
  b = no_split();
  scan_feature(gm, hm, 0, 6 * one, 0, &b);
  CHECK(b.feat == 0 && b.t == 2 && b.dir == 0);
}

static uint64_t lcg(uint64_t *s) {
  *s = *s * 6364136223846793005ull + 1442695040888963407ull;
  return *s >> 33;
}

static void random_cases() {
  uint64_t s = 12345;
  for (int rep = 0; rep < 300; rep++) {
    const int64_t n = 1 + (int64_t)(lcg(&s) % 41), m = 1 + (int64_t)(lcg(&s) % 7);
    std::vector<uint8_t> g((size_t)(n * m));
    for (auto &x : g) x = (uint8_t)(lcg(&s) % 10 < 2 ? 3 : lcg(&s) % 3);
    if (m > 1 && rep % 3 == 0)
      for (int64_t i = 0; i < n; i++) g[(size_t)(n + i)] = 3;            // variant 1 without an observed call
    if (m > 2 && rep % 3 == 1)
      for (int64_t i = 0; i < n; i++) g[(size_t)(2 * n + i)] = (uint8_t)(i % 3);   // variant 2 without a missing one
    std::vector<int64_t> off((size_t)(m + 1), 0);
    std::vector<int32_t> idx;
    for (int64_t j = 0; j < m; j++) {
      const int64_t want = m > 1 ? (int64_t)(lcg(&s) % 14) : 0;
      for (int64_t q = 0; q < want; q++) {
        const int32_t k = (int32_t)(lcg(&s) % (uint64_t)m);
        if (k != j) idx.push_back(k);   // in any order, repeats allowed: the statement only asks for k != j
      }
      off[(size_t)(j + 1)] = (int64_t)idx.size();
    }
    idx.push_back(0);   // keeps data() valid for an empty list; never read
    const double p_train = rep % 5 == 0 ? 1.0 : rep % 5 == 1 ? 1e-9 : 0.6;
    std::vector<uint8_t> out((size_t)(n * m)), again((size_t)(n * m));
    std::vector<double> infos((size_t)(2 * m)), infos2((size_t)(2 * m));
    std::vector<int32_t> trace((size_t)(m * 3 * kNodes), -2);
    const int64_t n_all = fast_impute_ref(g.data(), n, m, off.data(), idx.data(), p_train, 77 + rep, out.data(), infos.data(), trace.data(), 1);
    const int64_t n_all2 = fast_impute_ref(g.data(), n, m, off.data(), idx.data(), p_train, 77 + rep, again.data(), infos2.data(), nullptr, 2);
    CHECK(n_all == n_all2 && out == again);
    int64_t all_missing = 0;
    for (int64_t j = 0; j < m; j++) {
      int64_t miss = 0;
      for (int64_t i = 0; i < n; i++) miss += g[(size_t)(j * n + i)] == 3;
      all_missing += miss == n;
      CHECK(infos[(size_t)j] == (double)miss / (double)n);
      const double e = infos[(size_t)(m + j)], e2 = infos2[(size_t)(m + j)];
      CHECK((std::isnan(e) && std::isnan(e2)) || e == e2);
      CHECK(std::isnan(e) || (e >= 0.0 && e <= 1.0));
      if (miss == 0 || miss == n || p_train == 1.0) CHECK(std::isnan(e));
      for (int64_t i = 0; i < n; i++) {
        const uint8_t a = g[(size_t)(j * n + i)], b = out[(size_t)(j * n + i)];
        if (a != 3) CHECK(b == a);
        else if (miss == n) CHECK(b == 3);
        else CHECK(b >= 4 && b <= 6);
      }
      for (int k = 0; k < kNodes; k++) {
        const int32_t f = trace[(size_t)((j * kNodes + k) * 3)];
        CHECK(f >= -2 && f < off[(size_t)(j + 1)] - off[(size_t)j]);
      }
    }
    CHECK(n_all == all_missing);
  }
}

int main() {
  pieces();
  random_cases();
  printf(failures ? "%d checks failed\n" : "all checks held\n", failures);
  return failures ? 1 : 0;
}
