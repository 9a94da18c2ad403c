// Stand-alone program for the sanitizers (tests/test_auc_cpu.py compiles it with -fsanitize=address,undefined on the CPU):
// the CPU statement of AUC / AUCBoot (auc_ref.cpp over auc_step.hpp) against the O(n1 n0) definition written out here, over
// the case list of the tests plus every 0 / 1 target with both classes for n = 1 .. 9.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "auc_ref.cpp"

namespace {

int g_fail = 0, g_checks = 0;

void expect(bool ok, const char *what, long a = 0, long b = 0) {
  g_checks++;
  if (!ok) {
    g_fail++;
    std::printf("FAILED %s (%ld, %ld)\n", what, a, b);
  }
}

// the definition: pairs (case i, control j)
void definition(const std::vector<double> &x, const std::vector<uint8_t> &y, uint64_t out[3]) {
  uint64_t u = 0, n1 = 0, n0 = 0;
  for (size_t i = 0; i < x.size(); i++) {
    (y[i] ? n1 : n0)++;
    if (!y[i]) continue;
    for (size_t j = 0; j < x.size(); j++)
      if (!y[j]) u += x[i] > x[j] ? 2 : (x[i] == x[j] ? 1 : 0);
  }
  out[0] = u, out[1] = n1, out[2] = n0;
}

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t next() {   // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double unit() { return (double)(next() >> 11) * 0x1.0p-53; }

void check_column(const std::vector<double> &x, const std::vector<uint8_t> &y, const char *what) {
  const int64_t n = (int64_t)x.size();
  uint64_t want[3], got[3];
  double auc = 0.0;
  definition(x, y, want);
  const int64_t bad = auc_twin(x.data(), n, n, 1, y.data(), got, &auc);
  expect(bad == -1, what);
  expect(got[0] == want[0] && got[1] == want[1] && got[2] == want[2], what, (long)got[0], (long)want[0]);
  const double ref = (want[1] && want[2]) ? (double)want[0] / (2.0 * ((double)want[1] * (double)want[2])) : NAN;
  expect(auc == ref || (auc != auc && ref != ref), what);
}

void check_boot(const std::vector<double> &x, const std::vector<uint8_t> &y, int64_t nboot, uint64_t seed, const char *what) {
  const int64_t n = (int64_t)x.size();
  std::vector<double> rep((size_t)nboot);
  expect(auc_boot_twin(x.data(), n, n, 1, y.data(), nboot, seed, rep.data()) == -1, what);
  std::vector<int32_t> rows((size_t)n);
  for (int64_t b = 0; b < nboot; b++) {
    auc_draws(n, b, seed, rows.data());
    std::vector<double> xb((size_t)n);
    std::vector<uint8_t> yb((size_t)n);
    for (int64_t t = 0; t < n; t++) {
      expect(rows[(size_t)t] >= 0 && rows[(size_t)t] < n, "draw in range");
      xb[(size_t)t] = x[(size_t)rows[(size_t)t]], yb[(size_t)t] = y[(size_t)rows[(size_t)t]];
    }
    uint64_t want[3];
    definition(xb, yb, want);
    const double ref = (want[1] && want[2]) ? (double)want[0] / (2.0 * ((double)want[1] * (double)want[2])) : NAN;
    expect(rep[(size_t)b] == ref || (rep[(size_t)b] != rep[(size_t)b] && ref != ref), what, (long)b);
  }
}

std::vector<uint8_t> random_target(int64_t n) {
  std::vector<uint8_t> y((size_t)n);
  for (;;) {
    int64_t s = 0;
    for (auto &v : y) v = (uint8_t)(next() & 1), s += v;
    if (s > 0 && s < n) return y;
  }
}

}  // namespace

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  // random doubles and lattices
  for (int64_t n : {2, 3, 17, 64, 257, 600}) {
    std::vector<double> x((size_t)n);
    const std::vector<uint8_t> y = random_target(n);
    for (auto &v : x) v = unit() * 8.0 - 4.0;
    check_column(x, y, "random doubles");
    for (int L : {2, 3, 17}) {
      for (auto &v : x) v = (double)(next() % (uint64_t)L) - 1.0;
      check_column(x, y, "lattice");
    }
    for (auto &v : x) v = 0.25;
    check_column(x, y, "all equal");
    for (auto &v : x) v = (next() & 1) ? -0.0 : 0.0;
    check_column(x, y, "-0.0 beside +0.0");
    const double pool[6] = {-inf, inf, -0.0, 0.0, 1.5, -1.5};
    for (auto &v : x) v = pool[next() % 6];
    check_column(x, y, "+-Inf");
  }
  check_column({1.0, 0.0}, {1, 0}, "one case, one control");
  check_column({0.0, 1.0}, {1, 0}, "one case, one control");
  check_column({-0.0, 0.0}, {1, 0}, "one case, one control");
  // a NaN is refused and named
  {
    std::vector<double> x = {0.0, 1.0, 2.0, 0.0, NAN, 2.0};
    const std::vector<uint8_t> y = {0, 1, 1};
    uint64_t c[6];
    double a[2];
    expect(auc_twin(x.data(), 3, 3, 2, y.data(), c, a) == 1, "NaN column named");
  }
  // n = 1 .. 9: every target with both classes, three value patterns
  for (int n = 1; n <= 9; n++)
    for (unsigned mask = 1; mask + 1 < (1u << n); mask++) {
      std::vector<uint8_t> y((size_t)n);
      for (int i = 0; i < n; i++) y[(size_t)i] = (mask >> i) & 1;
      std::vector<double> x((size_t)n);
      for (int i = 0; i < n; i++) x[(size_t)i] = (double)((i * 5) % n);
      check_column(x, y, "exhaustive, distinct");
      for (int i = 0; i < n; i++) x[(size_t)i] = (double)((i * 7 + (int)mask) % 3);
      check_column(x, y, "exhaustive, three values");
      for (int i = 0; i < n; i++) x[(size_t)i] = 1.0;
      check_column(x, y, "exhaustive, equal");
    }
  // replicates against the definition on the resampled vectors
  {
    std::vector<double> x(6);
    for (auto &v : x) v = unit();
    check_boot(x, {0, 0, 1, 0, 0, 0}, 64, 7, "replicates, one case");
    std::vector<double> z(150);
    for (auto &v : z) v = (double)(next() % 5);
    check_boot(z, random_target(150), 40, 0xFFFFFFFF12345678ull, "replicates, lattice");
  }
  if (g_fail) {
    std::printf("%d of %d checks FAILED\n", g_fail, g_checks);
    return 1;
  }
  std::printf("all checks held (%d)\n", g_checks);
  return 0;
}
