// ancestry_ref.cpp — the CPU statement of snp_ancestry_summary / bed_ancestry: plain loops for the moments, the quadratic
// program and the correlations through qp_step.hpp (the header the kernels of bigsnpr_amd/csrc/ancestry.hip use) with its
// one-lane group.  Built by ancestry_ref.py with -ffp-contract=off -fopenmp; ancestry_check.cpp includes this file.
#include <stdint.h>

#include <cstddef>
#include <vector>

#include "qp_step.hpp"

using namespace bsn::qp;

namespace {

// the per-problem part: d = X'(l o correction), the program, the correlations.  X: L x K; l: L values; xf: K values
int one_problem(int K, int L, const double *D, const double *J0, const double *X, const double *corr, const double *l, bool sum_to_one, double M,
                const double *G0, const double *c0, const double *xf, double sf, double sff, double *ws, double *w, int64_t ldw,
                double *cor_each, int64_t ldc, double *cor_pred) {
  std::vector<double> d((size_t)K);
  for (int k = 0; k < K; k++) {
    double a = 0.0;
    for (int j = 0; j < L; j++) a += X[(size_t)k * L + j] * (l[j] * corr[j]);
    d[(size_t)k] = a;
  }
  const Solo g;
  const int steps = solve_one(g, K, D, J0, d.data(), 1, sum_to_one, ws, w, ldw);
  *cor_pred = cor_one(g, K, M, G0, c0, xf, 1, sf, sff, ws, cor_each, ldc);
  return steps;
}

}  // namespace

extern "C" {

int qp_max_k() { return kMaxK; }
int qp_iter_cap(int K) { return iter_cap(K); }
int64_t anc_slab_rows() { return kSlabRows; }
int anc_max_l() { return kMaxL; }

// B problems that share D (K x K column-major); dvec: K x B column-major; w: B x K column-major; steps: B.
// Returns 0, or 1: K < 1, 2: K above the cap, 3: D has no Cholesky factor.
int qp_simplex(const double *D, int64_t K, const double *dvec, int64_t B, int sum_to_one, double *w, int32_t *steps,
               int64_t *n_failed) {
  if (K < 1) return 1;
  if (K > kMaxK) return 2;
  std::vector<double> J0((size_t)K * K, 0.0);
  if (!factor((int)K, D, J0.data())) return 3;
  int64_t failed = 0;
#pragma omp parallel reduction(+ : failed)
  {
    std::vector<double> ws(work_doubles((int)K));
#pragma omp for schedule(dynamic, 16)
    for (int64_t b = 0; b < B; b++) {
      steps[b] = solve_one(Solo(), (int)K, D, J0.data(), dvec + b * K, 1, sum_to_one != 0, ws.data(), w + b, B);
      failed += steps[b] == kNotSolved;
    }
  }
  *n_failed = failed;
  return 0;
}

// P (M x L), X0 (M x K), F (M x B): column-major with leading dimensions.  Out, all column-major and compact:
// PtX0 L x K, PtF L x B, G0 K x K, X0tF K x B, csX0 K, csF B, sqF B.
void anc_moments(const double *P, int64_t ldp, const double *X0, int64_t ldx, const double *F, int64_t ldf, int64_t M, int L, int K,
                 int64_t B, double *PtX0, double *PtF, double *G0, double *X0tF, double *csX0, double *csF, double *sqF) {
  const int64_t ncol = K + B;
  auto right = [&](int64_t c) { return c < K ? X0 + c * ldx : F + (c - K) * ldf; };
#pragma omp parallel for schedule(dynamic, 1)
  for (int64_t c = 0; c < ncol; c++) {
    const double *v = right(c);
    for (int a = 0; a < L + K; a++) {
      const double *u = a < L ? P + (int64_t)a * ldp : X0 + (int64_t)(a - L) * ldx;
      double s = 0.0;
      for (int64_t i = 0; i < M; i++) s += u[i] * v[i];
      if (c < K)
        (a < L ? PtX0[a + c * L] : G0[(a - L) + c * K]) = s;
      else
        (a < L ? PtF[a + (c - K) * L] : X0tF[(a - L) + (c - K) * K]) = s;
    }
    double s1 = 0.0, s2 = 0.0;
    for (int64_t i = 0; i < M; i++) s1 += v[i], s2 += v[i] * v[i];
    if (c < K)
      csX0[c] = s1;
    else
      csF[c - K] = s1, sqF[c - K] = s2;
  }
}

// snp_ancestry_summary for B frequency columns.  w, cor_each: B x K column-major; cor_pred, steps: B.  Returns as qp_simplex.
int ancestry_summary(const double *F, int64_t ldf, int64_t B, const double *X0, int64_t ldx, const double *P, int64_t ldp,
                     const double *corr, int64_t M, int L, int K, const double *Dmat, int sum_to_one, double *w, double *cor_each,
                     double *cor_pred, int32_t *steps) {
  if (K < 1) return 1;
  if (K > kMaxK) return 2;
  std::vector<double> J0((size_t)K * K, 0.0);
  if (!factor(K, Dmat, J0.data())) return 3;
  std::vector<double> X((size_t)L * K), PtF((size_t)L * B), G0((size_t)K * K), XF((size_t)K * B), c0((size_t)K), sf((size_t)B), sff((size_t)B);
  anc_moments(P, ldp, X0, ldx, F, ldf, M, L, K, B, X.data(), PtF.data(), G0.data(), XF.data(), c0.data(), sf.data(), sff.data());
#pragma omp parallel
  {
    std::vector<double> ws(work_doubles(K));
#pragma omp for schedule(dynamic, 16)
    for (int64_t b = 0; b < B; b++)
      steps[b] = one_problem(K, L, Dmat, J0.data(), X.data(), corr, PtF.data() + b * L, sum_to_one != 0, (double)M, G0.data(), c0.data(),
                             XF.data() + b * K, sf[(size_t)b], sff[(size_t)b], ws.data(), w + b, B, cor_each + b, B, cor_pred + b);
  }
  return 0;
}

// bed_ancestry on dense rows: Gd (n x m column-major, leading dimension ldg) holds allele counts, f = g / 2 per row.
// X0: m x K, P: m x L, compact.  Results as ancestry_summary with B = n.
int ancestry_rows(const double *Gd, int64_t ldg, int64_t n, int64_t m, const double *X0, const double *P, const double *corr, int L,
                  int K, const double *Dmat, int sum_to_one, double *w, double *cor_each, double *cor_pred, int32_t *steps) {
  if (K < 1) return 1;
  if (K > kMaxK) return 2;
  std::vector<double> J0((size_t)K * K, 0.0);
  if (!factor(K, Dmat, J0.data())) return 3;
  std::vector<double> X((size_t)L * K), G0((size_t)K * K), c0((size_t)K);
  anc_moments(P, m, X0, m, nullptr, 0, m, L, K, 0, X.data(), nullptr, G0.data(), nullptr, c0.data(), nullptr, nullptr);
#pragma omp parallel
  {
    std::vector<double> ws(work_doubles(K)), l((size_t)L), xf((size_t)K);
#pragma omp for schedule(dynamic, 4)
    for (int64_t i = 0; i < n; i++) {
      double sf = 0.0, sff = 0.0;
      for (int64_t j = 0; j < m; j++) {
        const double f = Gd[i + j * ldg] / 2.0;
        sf += f;
        sff += f * f;
      }
      for (int a = 0; a < L + K; a++) {
        const double *u = a < L ? P + (int64_t)a * m : X0 + (int64_t)(a - L) * m;
        double s = 0.0;
        for (int64_t j = 0; j < m; j++) s += u[j] * (Gd[i + j * ldg] / 2.0);
        (a < L ? l[(size_t)a] : xf[(size_t)(a - L)]) = s;
      }
      steps[i] = one_problem(K, L, Dmat, J0.data(), X.data(), corr, l.data(), sum_to_one != 0, (double)m, G0.data(), c0.data(), xf.data(),
                             sf, sff, ws.data(), w + i, n, cor_each + i, n, cor_pred + i);
    }
  }
  return 0;
}

}  // extern "C"
