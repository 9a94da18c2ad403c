// knn_step.hpp — the exact k-nearest-neighbour rule of knn_parallel / prob_dist / LOF (bigutilsr's outlier-sample step of
// the reference's PCA workflow, vignettes/bedpca.Rmd): the squared distance of a query and a data point, the total order of
// the candidates, the sorted list of the k smallest, and the two statistics over the self-mode table.  Shared by the
// kernels (knn.hip) and the CPU statement (tests/native/knn_ref.cpp): the two cannot drift apart.  DESIGN.md 3.5r holds
// the statement in full.
//
// Everything is plain IEEE double in the order written here, never contracted (the pragma below on the device,
// -ffp-contract=off on the host) — but for the ONE explicit fused multiply-add of the squared distance.  Duplicated rows
// give distance 0, hence 1/0 = inf for a local reachability density and inf/inf = NaN for a LOF, as IEEE has them: no
// guard, nothing special-cased.
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#define BSN_KNN_HD __host__ __device__ __forceinline__
#else
#define BSN_KNN_HD inline
#endif

namespace bsn {
namespace knn {

constexpr int kMaxP = 64;   // coordinates of a point at most
constexpr int kMaxK = 64;   // neighbours at most

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

BSN_KNN_HD double fma_rn(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fma(a, b, c);
#else
  return std::fma(a, b, c);
#endif
}

BSN_KNN_HD double sqrt_rn(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(x);
#else
  return std::sqrt(x);
#endif
}

// one coordinate of the squared distance: acc <- fma(t, t, acc), t = q - x.  A coordinate that is 0 on both sides leaves
// acc as it is, bit for bit (fma(0, 0, acc) == acc): a kernel may pad p with zero coordinates.
BSN_KNN_HD double step(double q, double x, double acc) {
  const double t = q - x;
  return fma_rn(t, t, acc);
}

// the squared distance of q and x (p coordinates each, strides sq and sx): from 0, the coordinates in ascending order
BSN_KNN_HD double dist2(const double *q, int64_t sq, const double *x, int64_t sx, int p) {
  double acc = 0.0;
  for (int d = 0; d < p; d++) acc = step(q[d * sq], x[d * sx], acc);
  return acc;
}

// The total order of the candidates of one query: (squared distance, 0-based index of the data point), ascending and
// lexicographic.  No squared distance is NaN (non-finite coordinates are refused), so this is total; +inf (an overflow of
// finite coordinates) orders like any value.
BSN_KNN_HD bool before(double d2a, int32_t ia, double d2b, int32_t ib) { return d2a < d2b || (d2a == d2b && ia < ib); }

// what an unfilled place of a list holds: after every candidate (no data point has this index: n < 2^31)
constexpr int32_t kNoIndex = INT32_MAX;
BSN_KNN_HD double no_dist2() { return HUGE_VAL; }

// The sorted list of the k smallest candidates seen so far: place t at d2[t * stride], idx[t * stride].  Offers the
// candidate (c2, ci); returns whether it went in.  The result is the k smallest of everything offered, in the total order,
// whatever the order of the offers: tiles, slabs and launches cannot show.
BSN_KNN_HD bool offer(double *d2, int32_t *idx, int64_t stride, int k, double c2, int32_t ci) {
  if (!before(c2, ci, d2[(k - 1) * stride], idx[(k - 1) * stride])) return false;
  int t = k - 1;
  while (t > 0 && before(c2, ci, d2[(t - 1) * stride], idx[(t - 1) * stride])) {
    d2[t * stride] = d2[(t - 1) * stride];
    idx[t * stride] = idx[(t - 1) * stride];
    t--;
  }
  d2[t * stride] = c2;
  idx[t * stride] = ci;
  return true;
}

// ---- prob_dist over the self-mode table (d2, nn: n x k column-major, entry (i, t) at i + t * n) ---------------------------
// the mean squared distance of i to its k neighbours: plain additions, left to right, one division
BSN_KNN_HD double mean_d2(const double *d2, int64_t n, int64_t i, int k) {
  double s = d2[i];
  for (int t = 1; t < k; t++) s = s + d2[i + t * n];
  return s / (double)k;
}

// the mean of m2 over the neighbours of i, in the order of the list
BSN_KNN_HD double mean_over_nn(const double *v, const int32_t *nn, int64_t n, int64_t i, int k) {
  double s = v[nn[i]];
  for (int t = 1; t < k; t++) s = s + v[nn[i + t * n]];
  return s / (double)k;
}

// ---- LOF (Breunig, Kriegel, Ng, Sander 2000) over the self-mode table of distances (dist = sqrt_rn(d2)) ----------------
// local reachability density of i for kk neighbours; kdist[j] = dist[j + (kk - 1) * n]
BSN_KNN_HD double lrd(const double *dist, const int32_t *nn, int64_t n, int64_t i, int kk) {
  double s = 0.0;
  for (int t = 0; t < kk; t++) {
    const double kd = dist[nn[i + t * n] + (int64_t)(kk - 1) * n], di = dist[i + t * n];
    const double reach = kd > di ? kd : di;
    s = t == 0 ? reach : s + reach;
  }
  return 1.0 / (s / (double)kk);
}

// the local outlier factor of i from the densities
BSN_KNN_HD double lof(const double *lrd_v, const int32_t *nn, int64_t n, int64_t i, int kk) {
  return mean_over_nn(lrd_v, nn, n, i, kk) / lrd_v[i];
}

#if defined(__clang__)
#pragma clang fp contract(on)
#endif

}  // namespace knn
}  // namespace bsn
