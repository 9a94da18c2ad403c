// knn_ref.cpp — the CPU statement of knn_parallel / prob_dist / LOF: plain loops over every pair, the distance, the order,
// the list and the statistics through knn_step.hpp (the header the kernels of bigsnpr_amd/csrc/knn.hip use), and the
// planner of knn_plan.hpp as it stands.  Built by knn_ref.py with -ffp-contract=off -fopenmp.
#include <stdint.h>

#include <cstddef>
#include <vector>

#include "knn_plan.hpp"
#include "knn_step.hpp"

using namespace bsn::knn;

extern "C" {

// data: n x p, query: nq x p (NULL: self mode, nq ignored), both column-major with leading dimensions ld / ldq.  Queries
// q0 .. q1 - 1 only (rows q0 .. of the outputs; the other rows are left alone).  idx / d2 / dist: nq x k column-major.
void knn_table(const double *data, int64_t n, int64_t ld, const double *query, int64_t nq, int64_t ldq, int p, int k, int64_t q0,
               int64_t q1, int32_t *idx, double *d2, double *dist) {
  const bool self = query == nullptr;
  if (self) query = data, nq = n, ldq = ld;
#pragma omp parallel
  {
    std::vector<double> l2((std::size_t)k);
    std::vector<int32_t> li((std::size_t)k);
#pragma omp for schedule(dynamic, 16)
    for (int64_t i = q0; i < q1; i++) {
      for (int t = 0; t < k; t++) l2[(std::size_t)t] = no_dist2(), li[(std::size_t)t] = kNoIndex;
      for (int64_t j = 0; j < n; j++) {
        if (self && j == i) continue;
        offer(l2.data(), li.data(), 1, k, dist2(query + i, ldq, data + j, ld, p), (int32_t)j);
      }
      for (int t = 0; t < k; t++) {
        idx[i + (int64_t)t * nq] = li[(std::size_t)t];
        d2[i + (int64_t)t * nq] = l2[(std::size_t)t];
        dist[i + (int64_t)t * nq] = sqrt_rn(l2[(std::size_t)t]);
      }
    }
  }
}

// over the self-mode table (d2, nn: n x k column-major)
void knn_prob_dist(const double *d2, const int32_t *nn, int64_t n, int k, double *dist_self, double *dist_nn) {
  std::vector<double> m2((std::size_t)n);
  for (int64_t i = 0; i < n; i++) {
    m2[(std::size_t)i] = mean_d2(d2, n, i, k);
    dist_self[i] = sqrt_rn(m2[(std::size_t)i]);
  }
  for (int64_t i = 0; i < n; i++) dist_nn[i] = mean_over_nn(m2.data(), nn, n, i, k);
}

// over the self-mode table of distances (dist, nn: n x kmax column-major): out n x nk column-major
void knn_lof(const double *dist, const int32_t *nn, int64_t n, const int32_t *seq_k, int nk, double *out) {
  std::vector<double> l((std::size_t)n);
  for (int c = 0; c < nk; c++) {
    for (int64_t i = 0; i < n; i++) l[(std::size_t)i] = lrd(dist, nn, n, i, seq_k[c]);
    for (int64_t i = 0; i < n; i++) out[i + (int64_t)c * n] = lof(l.data(), nn, n, i, seq_k[c]);
  }
}

// the plan of a call: out = qb, nqb, S, partial bytes; lo [S + 1] = the slab bounds (NULL: not wanted)
void knn_plan(int64_t n, int64_t nq, int k, int ncu, int64_t forced, int64_t *out, int64_t *lo, int64_t lo_cap) {
  const Plan P = plan(n, nq, k, ncu, forced);
  out[0] = P.qb;
  out[1] = P.nqb;
  out[2] = P.S;
  out[3] = P.partial_bytes(nq, k);
  if (lo)
    for (int s = 0; s <= P.S && s < lo_cap; s++) lo[s] = P.lo(s);
}

int64_t knn_partial_cap() { return kPartialCap; }
int64_t knn_min_slab_points() { return kMinSlabPoints; }
int knn_padded_p(int p) { return padded_p(p); }

}  // extern "C"
