// ancestry_check.cpp — a stand-alone program over qp_step.hpp and the CPU statement (ancestry_ref.cpp, included below): the
// edge cases of the quadratic program (K = 1, 2, 3, an interior minimum, a vertex, sum w < 1, w = 0, two identical
// reference columns, K at the cap, K above it, a matrix without a Cholesky factor, NaN and infinity in d) and a few hundred
// random problems of every K, each held to feasibility and to the stationarity of its minimiser; then the moments, the
// summary and the rows entry on a small table.  Meant to be compiled with -fsanitize=address,undefined and run as a program
// (tests/test_ancestry_cpu.py does both).  Exit status 0 = every check held.
#include <stdio.h>

#include <cmath>
#include <vector>

#include "ancestry_ref.cpp"

static int failures = 0;
#define CHECK(cond)                                          \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAILED line %d: %s\n", __LINE__, #cond);       \
      failures++;                                            \
    }                                                        \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double unif() {   // xorshift64*, (0, 1)
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return ((double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) + 0.5) / 9007199254740992.0;
}

// D = A'A / rows + ridge I for a random A (rows x K); twin: column 1 repeats column 0
static std::vector<double> gram(int K, int rows, double ridge, bool twin, std::vector<double> *A_out = nullptr) {
  std::vector<double> A((size_t)rows * K), D((size_t)K * K);
  for (auto &v : A) v = 2.0 * unif() - 1.0;
  if (twin && K > 1)
    for (int i = 0; i < rows; i++) A[(size_t)rows + i] = A[(size_t)i];
  for (int a = 0; a < K; a++)
    for (int b = 0; b < K; b++) {
      double s = 0.0;
      for (int i = 0; i < rows; i++) s += A[(size_t)a * rows + i] * A[(size_t)b * rows + i];
      D[(size_t)b * K + a] = s / rows + (a == b ? ridge : 0.0);
    }
  if (A_out) *A_out = A;
  return D;
}

static std::vector<double> times(const std::vector<double> &D, int K, const std::vector<double> &w) {
  std::vector<double> g((size_t)K, 0.0);
  for (int a = 0; a < K; a++)
    for (int b = 0; b < K; b++) g[(size_t)a] += D[(size_t)b * K + a] * w[(size_t)b];
  return g;
}

// feasibility, and the KKT conditions with the multiplier of the sum read off the free coordinates: on w_k > 0 the
// gradient is -lambda, on w_k = 0 it is at least -lambda; lambda >= 0 for the inequality, 0 when it is slack
static void check_minimiser(const std::vector<double> &D, int K, const std::vector<double> &d, const std::vector<double> &w, bool s1) {
  double sum = 0.0, dmax = 0.0;
  for (int k = 0; k < K; k++) {
    CHECK(w[(size_t)k] >= 0.0);
    sum += w[(size_t)k];
    dmax = fmax(dmax, fabs(d[(size_t)k]));
  }
  for (double v : D) dmax = fmax(dmax, fabs(v));
  CHECK(s1 ? fabs(sum - 1.0) <= 1e-12 : sum <= 1.0 + 1e-12);
  const double tol = 1e-10 * dmax;
  std::vector<double> g = times(D, K, w);
  double lam = 0.0;
  int nfree = 0;
  for (int k = 0; k < K; k++) {
    g[(size_t)k] -= d[(size_t)k];
    if (w[(size_t)k] > 0.0) lam -= g[(size_t)k], nfree++;
  }
  const bool sum_active = s1 || fabs(sum - 1.0) <= 1e-12;
  lam = nfree && sum_active ? lam / nfree : 0.0;
  if (!s1) CHECK(lam >= -tol);
  for (int k = 0; k < K; k++) {
    if (w[(size_t)k] > 0.0)
      CHECK(fabs(g[(size_t)k] + lam) <= tol);
    else
      CHECK(g[(size_t)k] + lam >= -tol);
  }
}

static std::vector<double> solve(const std::vector<double> &D, int K, const std::vector<double> &d, bool s1, int *steps_out = nullptr) {
  std::vector<double> w((size_t)K, -7.0);
  int32_t steps = 0;
  int64_t failed = -1;
  CHECK(qp_simplex(D.data(), K, d.data(), 1, s1, w.data(), &steps, &failed) == 0);
  CHECK(failed == 0 && steps >= 0 && steps <= iter_cap(K));
  if (steps_out) *steps_out = steps;
  return w;
}

static void edge_cases() {
  for (int K = 1; K <= 3; K++)
    for (int s1 = 0; s1 < 2; s1++) {
      std::vector<double> D = gram(K, K + 3, 0.0, false), d((size_t)K);
      for (auto &v : d) v = 2.0 * unif() - 1.0;
      check_minimiser(D, K, d, solve(D, K, d, s1), s1);
    }
  const int K = 7;
  std::vector<double> D = gram(K, 10, 0.0, false), wi((size_t)K);
  double s = 0.0;
  for (auto &v : wi) v = 0.5 + unif(), s += v;
  for (auto &v : wi) v /= s;
  std::vector<double> d = times(D, K, wi), w = solve(D, K, d, true);   // interior: the unconstrained minimum sums to 1
  for (int k = 0; k < K; k++) CHECK(fabs(w[(size_t)k] - wi[(size_t)k]) <= 1e-9 && w[(size_t)k] > 0.0);
  check_minimiser(D, K, d, w, true);
  std::vector<double> e((size_t)K, 0.0);   // a vertex: K - 1 bounds active
  e[2] = 1.0;
  d = times(D, K, e);
  for (int k = 0; k < K; k++) d[(size_t)k] += 0.5 - (k == 2 ? 0.0 : 1.0);
  w = solve(D, K, d, true);
  for (int k = 0; k < K; k++) CHECK(w[(size_t)k] == e[(size_t)k] || (k == 2 && fabs(w[2] - 1.0) <= 1e-12));
  check_minimiser(D, K, d, w, true);
  std::vector<double> half = wi;   // sum w = 1/2 < 1
  for (auto &v : half) v *= 0.5;
  d = times(D, K, half);
  int steps = -1;
  w = solve(D, K, d, false, &steps);
  CHECK(steps == 0);
  for (int k = 0; k < K; k++) CHECK(fabs(w[(size_t)k] - half[(size_t)k]) <= 1e-9);
  for (auto &v : d) v = -0.1 - unif();   // all negative: w = 0
  w = solve(D, K, d, false);
  for (int k = 0; k < K; k++) CHECK(w[(size_t)k] == 0.0);
  check_minimiser(D, K, d, w, false);
  // two identical reference columns: D singular up to a ridge of 1e-8 (what nearPD leaves), d in the range
  std::vector<double> A;
  D = gram(K, 9, 1e-8, true, &A);
  std::vector<double> wt((size_t)K, 0.0);
  wt[3] = 0.7, wt[5] = 0.3;
  d = times(D, K, wt);
  for (int s1 = 0; s1 < 2; s1++) check_minimiser(D, K, d, solve(D, K, d, s1), s1);
  // K at the cap, and above it
  D = gram(kMaxK, kMaxK + 10, 0.0, false);
  wt.assign((size_t)kMaxK, 0.0);
  wt[0] = 0.5, wt[17] = 0.3, wt[59] = 0.2;
  d = times(D, kMaxK, wt);
  for (auto &v : d) v += 0.05 * (2.0 * unif() - 1.0);
  for (int s1 = 0; s1 < 2; s1++) check_minimiser(D, kMaxK, d, solve(D, kMaxK, d, s1), s1);
  std::vector<double> big((size_t)(kMaxK + 1) * (kMaxK + 1), 0.0), dz((size_t)kMaxK + 1, 0.0), wz((size_t)kMaxK + 1, 0.0);
  int32_t st[3];
  int64_t failed = 0;
  CHECK(qp_simplex(big.data(), kMaxK + 1, dz.data(), 1, 1, wz.data(), st, &failed) == 2);
  CHECK(qp_simplex(big.data(), 0, dz.data(), 1, 1, wz.data(), st, &failed) == 1);
  const double indef[4] = {1.0, 2.0, 2.0, 1.0};
  CHECK(qp_simplex(indef, 2, dz.data(), 1, 1, wz.data(), st, &failed) == 3);
  // NaN and infinity in d: NaN rows, not counted as failed; the finite problem beside them is solved
  const double D3[9] = {1.1, 0.1, 0.1, 0.1, 1.1, 0.1, 0.1, 0.1, 1.1};
  const double d3[9] = {0.3, NAN, 0.1, 0.2, 0.5, INFINITY, 0.1, 0.2, 0.3};
  double w3[9];
  CHECK(qp_simplex(D3, 3, d3, 3, 1, w3, st, &failed) == 0 && failed == 0);
  CHECK(st[0] == kNanInput && st[1] == kNanInput && st[2] >= 0);
  for (int k = 0; k < 3; k++) CHECK(std::isnan(w3[0 + 3 * k]) && std::isnan(w3[1 + 3 * k]) && w3[2 + 3 * k] >= 0.0);
}

static void random_cases() {
  for (int K = 1; K <= kMaxK; K++)
    for (int rep = 0; rep < 6; rep++) {
      const bool thin = rep >= 4 && K > 2;   // fewer rows than columns: singular up to the ridge
      std::vector<double> D = gram(K, thin ? K - 2 : K + 3, thin ? 1e-8 : 0.0, false), wt((size_t)K), d;
      double s = 0.0;
      for (auto &v : wt) v = unif() < 0.7 ? 0.0 : unif(), s += v;
      for (auto &v : wt) v = s > 0.0 ? v / s : 1.0 / K;
      d = times(D, K, wt);
      if (!thin)
        for (auto &v : d) v += 0.3 * (rep % 3) * (2.0 * unif() - 1.0);
      for (int s1 = 0; s1 < 2; s1++) check_minimiser(D, K, d, solve(D, K, d, s1), s1);
    }
}

static void tables() {
  const int64_t M = 37;
  const int L = 3, K = 4, B = 2;
  std::vector<double> P((size_t)M * L), X0((size_t)M * K), F((size_t)M * B), corr((size_t)L, 1.0);
  for (auto &v : P) v = 2.0 * unif() - 1.0;
  for (auto &v : X0) v = unif();
  for (int64_t i = 0; i < M; i++) {
    F[(size_t)i] = 0.25 * X0[(size_t)i] + 0.75 * X0[(size_t)(2 * M + i)];   // a planted mixture
    F[(size_t)(M + i)] = unif();
  }
  std::vector<double> X((size_t)L * K), PtF((size_t)L * B), G0((size_t)K * K), XF((size_t)K * B), c0((size_t)K), sf((size_t)B), sff((size_t)B);
  anc_moments(P.data(), M, X0.data(), M, F.data(), M, M, L, K, B, X.data(), PtF.data(), G0.data(), XF.data(), c0.data(), sf.data(),
              sff.data());
  double s = 0.0;
  for (int64_t i = 0; i < M; i++) s += X0[(size_t)(M + i)] * F[(size_t)i];
  CHECK(fabs(XF[1] - s) <= 1e-12);
  std::vector<double> Dm((size_t)K * K);   // X'X + ridge: L < K
  for (int a = 0; a < K; a++)
    for (int b = 0; b < K; b++) {
      double t = 0.0;
      for (int j = 0; j < L; j++) t += X[(size_t)a * L + j] * X[(size_t)b * L + j];
      Dm[(size_t)b * K + a] = t + (a == b ? 1e-8 : 0.0);
    }
  std::vector<double> w((size_t)B * K), ce((size_t)B * K), cp((size_t)B);
  int32_t st[B];
  CHECK(ancestry_summary(F.data(), M, B, X0.data(), M, P.data(), M, corr.data(), M, L, K, Dm.data(), 1, w.data(), ce.data(), cp.data(),
                         st) == 0);
  CHECK(st[0] >= 0 && st[1] >= 0 && cp[0] > 1.0 - 1e-6 && fabs(cp[1]) <= 1.0 && fabs(ce[0]) <= 1.0 + 1e-12);
  // rows: genotypes 0 / 1 / 2, n x m with m = M
  const int64_t n = 5;
  std::vector<double> Gd((size_t)n * M), wr((size_t)n * K), cer((size_t)n * K), cpr((size_t)n);
  for (auto &v : Gd) v = floor(3.0 * unif());
  int32_t str[n];
  CHECK(ancestry_rows(Gd.data(), n, n, M, X0.data(), P.data(), corr.data(), L, K, Dm.data(), 1, wr.data(), cer.data(), cpr.data(), str) == 0);
  for (int64_t i = 0; i < n; i++) {
    double sum = 0.0;
    for (int k = 0; k < K; k++) sum += wr[(size_t)(i + k * n)];
    CHECK(str[i] >= 0 && fabs(sum - 1.0) <= 1e-12 && fabs(cpr[(size_t)i]) <= 1.0 + 1e-12);
  }
}

int main() {
  edge_cases();
  random_cases();
  tables();
  if (failures) {
    printf("%d checks FAILED\n", failures);
    return 1;
  }
  printf("all checks held\n");
  return 0;
}
