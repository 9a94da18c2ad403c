// irls_check.cpp — a stand-alone program over irls_step.hpp's packed Cholesky solve, the inverse's [0, 0] entry and the
// convergence rule on hand-made systems (P = 2, 16, 17, 32; one singular), meant to be compiled with
// -fsanitize=address,undefined and run as a program (tests/test_gwas_cpu.py does both).  Exit status 0 = every check held.
#include <stdio.h>

#include <cmath>
#include <vector>

#include "irls_step.hpp"

using namespace bsn::irls;

static int failures = 0;
#define CHECK(cond)                                          \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAILED line %d: %s\n", __LINE__, #cond);       \
      failures++;                                            \
    }                                                        \
  } while (0)

// H = M' M + I with M[i][j] = sin(1 + i + 2 j) (P x P): symmetric positive definite, dense
static std::vector<double> dense_spd(int P) {
  std::vector<double> M((size_t)P * P), H((size_t)P * P, 0.0);
  for (int i = 0; i < P; i++)
    for (int j = 0; j < P; j++) M[(size_t)i * P + j] = std::sin(1.0 + i + 2.0 * j);
  for (int i = 0; i < P; i++)
    for (int j = 0; j < P; j++) {
      double s = i == j ? 1.0 : 0.0;
      for (int k = 0; k < P; k++) s += M[(size_t)k * P + i] * M[(size_t)k * P + j];
      H[(size_t)i * P + j] = s;
    }
  return H;
}

static void one_system(int P) {
  const std::vector<double> H = dense_spd(P);
  std::vector<double> truth((size_t)P), G((size_t)(P + 1) * (P + 2) / 2, 0.0), beta((size_t)P, 0.0), work((size_t)2 * P);
  for (int k = 0; k < P; k++) truth[(size_t)k] = 0.5 - 0.1 * k;
  for (int j = 0; j < P; j++)
    for (int i = 0; i <= j; i++) G[(size_t)packed(i, j)] = H[(size_t)i * P + j];
  for (int i = 0; i < P; i++) {
    double s = 0.0;
    for (int k = 0; k < P; k++) s += H[(size_t)i * P + k] * truth[(size_t)k];
    G[(size_t)packed(i, P)] = s;
  }
  const std::vector<double> G0 = G;
  double inv00 = 0.0;
  int st = solve_step(G.data(), P, beta.data(), 1e-8, &inv00, work.data());
  CHECK(st == 0);   // from beta = 0 every coefficient moved
  for (int k = 0; k < P; k++) CHECK(std::fabs(beta[(size_t)k] - truth[(size_t)k]) < 1e-9);
  // H e = e_0 solved through the same routine gives the first column of the inverse: its [0] entry is inv00
  std::vector<double> G1 = G0, col((size_t)P, 0.0);
  for (int i = 0; i < P; i++) G1[(size_t)packed(i, P)] = i == 0 ? 1.0 : 0.0;
  double again = 0.0;
  CHECK(solve_step(G1.data(), P, col.data(), 1e-8, &again, work.data()) == 0);
  CHECK(std::fabs(col[0] - inv00) < 1e-12 * std::fabs(inv00));
  CHECK(again == inv00 && inv00 > 0);
  // a second solve of the same system from its solution has converged
  G = G0;
  st = solve_step(G.data(), P, beta.data(), 1e-8, &inv00, work.data());
  CHECK(st == 1);
}

static void singular_system() {
  // columns 0 and 1 proportional (a variant without variance beside the intercept): the second pivot is 0
  const int P = 3;
  const double C[4][3] = {{2, 1, 0.3}, {2, 1, -1.0}, {2, 1, 0.7}, {2, 1, 2.0}};
  std::vector<double> G((size_t)(P + 1) * (P + 2) / 2, 0.0), beta((size_t)P, 0.25), work((size_t)2 * P);
  for (int r = 0; r < 4; r++)
    for (int j = 0; j < P; j++)
      for (int i = 0; i <= j; i++) G[(size_t)packed(i, j)] += C[r][i] * C[r][j];
  double inv00 = -1.0;
  CHECK(solve_step(G.data(), P, beta.data(), 1e-8, &inv00, work.data()) == -1);
  for (int k = 0; k < P; k++) CHECK(beta[(size_t)k] == 0.25);   // untouched
  std::vector<double> Z((size_t)3, 0.0);   // a zero matrix: the first pivot
  CHECK(!chol_packed(Z.data(), 2));
}

static void convergence_rule() {
  const double a[3] = {1.0, -2.0, 0.0}, b[3] = {1.0 + 1e-9, -2.0, 0.0}, c[3] = {1.0, -2.0, 1e-300};
  CHECK(converged(a, a, 3, 0.0));          // nothing moved, a zero coefficient included
  CHECK(converged(b, a, 3, 1e-8));         // 2 * 1e-9 / 2 = 1e-9
  CHECK(!converged(b, a, 3, 1e-10));
  CHECK(!converged(c, a, 3, 1e-8));        // 0 -> 1e-300 is a relative change of 2
  const double d[3] = {1.0, qnan(), 0.0};
  CHECK(!converged(d, a, 3, 1e-8));
}

static void sample_maps() {
  const double etas[7] = {0.0, 1.0, -1.0, 36.5, -36.5, 745.0, -745.0};
  for (double eta : etas)
    for (double y : {0.0, 1.0}) {
      double w, wz;
      sample_map(eta, y, w, wz);
      CHECK(w >= 0 && w <= 0.25 && wz == wz && std::isfinite(wz));
      const double p = 1.0 / (1.0 + std::exp(-eta));
      CHECK(std::fabs(w - p * (1 - p)) <= 1e-13 * 0.25);
      CHECK(std::fabs(wz - (p * (1 - p) * eta + (y - p))) <= 1e-13 * (1.0 + std::fabs(wz)));
    }
}

int main() {
  for (int P : {2, 16, 17, 32}) one_system(P);
  singular_system();
  convergence_rule();
  sample_maps();
  printf(failures ? "%d checks failed\n" : "all checks held\n", failures);
  return failures ? 1 : 0;
}
