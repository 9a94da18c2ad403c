// sparse_ld.hip — a sparse LD matrix resident in HBM (bigsparser's SFBM, as R/lassosum2.R receives it through
// `corr`) and snp_lassosum2's coordinate descent over it, the whole grid of (lambda, delta) in one launch.
//
// The matrix.  snp_cor / bed_cor hand back the upper triangle (with the diagonal) of a symmetric dsCMatrix;
// bigsparser::as_SFBM turns it into full columns, and SFBM::incr_mult_col(j, v, c) adds x_ij * c to v[i] over the
// stored entries of column j.  bsn_sfbm_from_csc checks the CSC on the host (p, row range, strictly ascending rows)
// before anything reaches the device, then expands an upper triangle on the device: column j of the full matrix is
// column j of the triangle (rows <= j, ascending) followed by row j of the triangle (rows > j), which a radix sort of
// the off-diagonal entries by (row, column) brings into column order.  Each column's row span is kept: its maximum
// distance to the column index is the bandwidth.
//
// The solver.  _bigsnpr_lassosum2 (8 args) src/lassosum2.cpp:8-70, for G grid points per call instead of one: one
// wave per grid point, its curr_beta [m] and dotprods [m2] in HBM.  The wave decides 64 coordinates at a time against
// the current dotprods.  A coordinate whose shift is exactly 0 changes no state, so every coordinate up to the first
// one with a non-zero shift is decided as the sequential loop would decide it; their gap / df terms are added in j
// order, the committing coordinate's column is added to dotprods by all 64 lanes (each row once: the order of the
// additions into any one element is the column order of the reference), and the wave decides again from the next
// coordinate.  Every floating-point operation is the reference's, in the reference's order, without contraction:
// the results equal the sequential loop bit for bit.
#include <algorithm>
#include <cmath>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "bsn_internal.hpp"

struct bsn_sfbm {
  int64_t m2 = 0, nnz = 0;
  bsn::DevBuf<int64_t> p;   // [m2 + 1] full columns
  bsn::DevBuf<int32_t> i;   // [nnz] ascending in each column
  bsn::DevBuf<double> x;    // [nnz]
  std::vector<int32_t> lo, hi;   // row span of each column (lo > hi: empty column)
  int64_t bandwidth = 0;         // max over columns of max(j - lo, hi - j)
};

namespace bsn {
namespace {

constexpr uint64_t kDiagKey = ~0ull;   // sorts after every off-diagonal (row, column) key

// one thread per stored entry of the upper triangle: copy it to its place in the full column, and give an off-diagonal
// entry (r < c) its key for the transposed half
__global__ void k_expand_upper(const int64_t *__restrict__ up_p, const int32_t *__restrict__ up_i, const double *__restrict__ up_x,
                               int64_t m2, int64_t nnz_up, const int64_t *__restrict__ full_p, int32_t *__restrict__ full_i,
                               double *__restrict__ full_x, uint64_t *__restrict__ key, double *__restrict__ val) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz_up) return;
  int64_t a = 0, b = m2;   // the column c with up_p[c] <= e < up_p[c + 1]
  while (b - a > 1) {
    const int64_t mid = (a + b) >> 1;
    if (up_p[mid] <= e) a = mid; else b = mid;
  }
  const int64_t c = a;
  const int32_t r = up_i[e];
  const int64_t at = full_p[c] + (e - up_p[c]);
  full_i[at] = r;
  full_x[at] = up_x[e];
  key[e] = r < c ? ((uint64_t)r << 32) | (uint64_t)c : kDiagKey;
  val[e] = up_x[e];
}

// the sorted off-diagonal entries (r, c) go after the triangle's own part of full column r
__global__ void k_place_transposed(const uint64_t *__restrict__ key, const double *__restrict__ val, int64_t n_off,
                                   const int64_t *__restrict__ up_p, const int64_t *__restrict__ t_p,
                                   const int64_t *__restrict__ full_p, int32_t *__restrict__ full_i, double *__restrict__ full_x) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_off) return;
  const uint64_t k = key[s];
  const int64_t r = (int64_t)(k >> 32), c = (int64_t)(k & 0xffffffffull);
  const int64_t at = full_p[r] + (up_p[r + 1] - up_p[r]) + (s - t_p[r]);
  full_i[at] = (int32_t)c;
  full_x[at] = val[s];
}

__global__ void k_row_span(const int64_t *__restrict__ p, const int32_t *__restrict__ i, int64_t m2, int32_t *__restrict__ lo,
                           int32_t *__restrict__ hi) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m2) return;
  const int64_t a = p[j], b = p[j + 1];
  lo[j] = a < b ? i[a] : 1;
  hi[j] = a < b ? i[b - 1] : 0;
}

#pragma clang fp contract(off)

__device__ __forceinline__ double soft_thres(double z, double l1, double one_plus_l2) {
  if (z > 0) {
    const double num = z - l1;
    return (num > 0) ? num / one_plus_l2 : 0;
  } else {
    const double num = z + l1;
    return (num < 0) ? num / one_plus_l2 : 0;
  }
}

__device__ __forceinline__ double lane_value(double v, int l) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, l);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__device__ __forceinline__ int64_t lane_index(int64_t v, int l) {
  const int lo = __builtin_amdgcn_readlane((int)v, l);
  const int hi = __builtin_amdgcn_readlane((int)(v >> 32), l);
  return (int64_t)(((uint64_t)(unsigned int)hi << 32) | (unsigned int)lo);
}

// gap0 = 2 * std::inner_product(beta_hat, beta_hat, 0.0) (src/lassosum2.cpp:36-37): a sequential sum on the host
double lassosum2_gap0(const double *beta_hat, int64_t m) {
  double ss = 0.0;
  for (int64_t j = 0; j < m; j++) ss = ss + beta_hat[j] * beta_hat[j];
  return 2 * ss;
}

constexpr int kAxpyBatch = 32;   // entries per lane and round of a column update (2 048 per round: a C5 column in two)

// One wave (64 lanes) per grid point g = g0 + blockIdx.x; dots / curs: this batch's dotprods [m2] and curr_beta [m].
__global__ __launch_bounds__(64) void k_lassosum2(const int64_t *__restrict__ P, const int32_t *__restrict__ I,
                                                  const double *__restrict__ X, int64_t m2, const double *__restrict__ beta_hat,
                                                  const double *__restrict__ pf, const int64_t *__restrict__ ind_sub, int64_t m,
                                                  const double *__restrict__ lambda, const double *__restrict__ delta, int64_t g0,
                                                  double gap0, double dfmax, int maxiter, double tol, double *dots, double *curs,
                                                  double *__restrict__ beta_out, int32_t *__restrict__ num_iter,
                                                  uint64_t *__restrict__ ticks) {
  const int lane = threadIdx.x;
  const int64_t g = g0 + blockIdx.x;
  double *dot = dots + (int64_t)blockIdx.x * m2;   // no __restrict__: lanes read what other lanes stored
  double *cur = curs + (int64_t)blockIdx.x * m;
  const double lam = lambda[g], del = delta[g];
  const uint64_t t0 = wall_clock64();
  bool diverged = false;
  int k = 0;
  for (; k < maxiter; k++) {
    bool conv = true;
    double df = 0, gap = 0;
    for (int64_t j0 = 0; j0 < m; j0 += 64) {
      const int64_t j = j0 + lane;
      const bool in = j < m;
      int64_t j2 = 0;
      double bh = 0, lj = 0, dpo = 0, cb = 0;
      if (in) {
        j2 = ind_sub ? ind_sub[j] : j;
        bh = beta_hat[j];
        const double pj = pf[j];
        lj = pj * lam;            // R/lassosum2.R:59  pf * grid_param$lambda[ic]
        dpo = pj * del + 1.0;     // R/lassosum2.R:60  pf * grid_param$delta[ic] + 1
        cb = cur[j];
      }
      int from = 0;   // lanes below `from` are decided
      for (;;) {
        const bool act = in && lane >= from;
        double nb = 0, sh = 0;
        if (act) {
          const double u = bh - (dot[j2] - cb);
          nb = soft_thres(u, lj, dpo);
          sh = nb - cb;
        }
        const uint64_t moves = __ballot(act && sh != 0);
        const int f = moves ? __ffsll((unsigned long long)moves) - 1 : 64;   // the first coordinate that changes state
        uint64_t nz = __ballot(act && nb != 0);
        if (f < 63) nz &= (2ull << f) - 1;
        df += (double)__popcll(nz);   // df++ per coordinate: exact on integers
        const double sq = nb * nb;
        while (nz) {
          const int l = __ffsll((unsigned long long)nz) - 1;
          gap += lane_value(sq, l);
          nz &= nz - 1;
        }
        if (f == 64) break;
        const double shift = lane_value(sh, f);
        if (conv && fabs(shift) > tol) conv = false;
        if (lane == f) {
          cb = nb;
          cur[j] = nb;
        }
        const int64_t c = lane_index(j2, f);
        // the column in rounds of kAxpyBatch entries per lane: all loads of a round in flight before its stores (one
        // load latency per round instead of one per entry; rows are distinct within a column, so nothing aliases)
        const int64_t e1 = P[c + 1];
        for (int64_t eb = P[c] + lane; eb < e1; eb += 64 * kAxpyBatch) {
          int32_t r[kAxpyBatch];
          double xv[kAxpyBatch], dv[kAxpyBatch];
#pragma unroll
          for (int u = 0; u < kAxpyBatch; u++) {
            const int64_t e = eb + 64 * u;
            r[u] = e < e1 ? I[e] : 0;
            xv[u] = e < e1 ? X[e] : 0.0;
          }
#pragma unroll
          for (int u = 0; u < kAxpyBatch; u++)
            if (eb + 64 * u < e1) dv[u] = dot[r[u]];
#pragma unroll
          for (int u = 0; u < kAxpyBatch; u++)
            if (eb + 64 * u < e1) dot[r[u]] = dv[u] + xv[u] * shift;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the stores above, before any lane reads dot again
        from = f + 1;
        if (from >= 64) break;
      }
    }
    if (gap > gap0) {
      diverged = true;
      break;
    }
    if (conv || df > dfmax) break;
  }
  for (int64_t j = lane; j < m; j += 64) beta_out[g * m + j] = diverged ? __builtin_nan("") : cur[j];
  if (lane == 0) {
    num_iter[g] = k + 1;
    ticks[g] = wall_clock64() - t0;
  }
}

#pragma clang fp contract(on)

}  // namespace
}  // namespace bsn

using namespace bsn;

extern "C" {

int bsn_sfbm_from_csc(const int64_t *p, const int32_t *i, const double *x, int64_t m2, int upper, bsn_sfbm **out) {
  return guarded([&] {
    if (!out) fail("bsn_sfbm_from_csc: out is NULL");
    *out = nullptr;
    if (m2 < 0 || m2 > 0x7fffffffLL) fail("'corr' must have between 0 and 2^31 - 1 columns.");
    if (!p) fail("'corr@p' is NULL.");
    if (p[0] != 0) fail("'corr@p' must start at 0.");
    for (int64_t j = 0; j < m2; j++)
      if (p[j + 1] < p[j]) fail("'corr@p' must be non-decreasing (column %lld).", (long long)j);
    const int64_t nnz = p[m2];
    if (nnz > 0 && (!i || !x)) fail("'corr@i' or 'corr@x' is NULL.");
    // host checks first: rows in range, strictly ascending, in the upper triangle when asked; count the transposed half
    std::vector<int64_t> t_cnt(upper ? (size_t)m2 + 1 : 0, 0);
    for (int64_t j = 0; j < m2; j++) {
      for (int64_t e = p[j]; e < p[j + 1]; e++) {
        const int64_t r = i[e];
        if (r < 0 || r >= m2) fail("row index %lld out of range [0, %lld) in column %lld.", (long long)r, (long long)m2, (long long)j);
        if (e > p[j] && r <= i[e - 1]) fail("row indices must be strictly increasing within column %lld.", (long long)j);
        if (upper) {
          if (r > j) fail("an upper-triangular 'corr' has row %lld > column %lld.", (long long)r, (long long)j);
          if (r < j) t_cnt[(size_t)r]++;
        }
      }
    }
    require_gpu();
    std::unique_ptr<bsn_sfbm> S(new bsn_sfbm);
    S->m2 = m2;
    std::vector<int64_t> full_p((size_t)m2 + 1), t_p;
    if (upper) {
      t_p.assign((size_t)m2 + 1, 0);
      for (int64_t j = 0; j < m2; j++) t_p[(size_t)j + 1] = t_p[(size_t)j] + t_cnt[(size_t)j];
      for (int64_t j = 0; j <= m2; j++) full_p[(size_t)j] = p[j] + t_p[(size_t)j];
    } else {
      std::copy(p, p + m2 + 1, full_p.begin());
    }
    S->nnz = full_p[(size_t)m2];
    BSN_HIP(hipMemcpy(S->p.ensure((size_t)m2 + 1), full_p.data(), ((size_t)m2 + 1) * 8, hipMemcpyHostToDevice));
    S->i.ensure((size_t)std::max<int64_t>(S->nnz, 1));
    S->x.ensure((size_t)std::max<int64_t>(S->nnz, 1));
    if (!upper) {
      if (nnz) {
        BSN_HIP(hipMemcpy(S->i.p, i, (size_t)nnz * 4, hipMemcpyHostToDevice));
        BSN_HIP(hipMemcpy(S->x.p, x, (size_t)nnz * 8, hipMemcpyHostToDevice));
      }
    } else if (nnz) {
      const int64_t n_off = t_p[(size_t)m2];
      DevBuf<int64_t> d_up_p, d_t_p;
      DevBuf<int32_t> d_up_i;
      DevBuf<double> d_up_x, d_val, d_val2;
      DevBuf<uint64_t> d_key, d_key2;
      BSN_HIP(hipMemcpy(d_up_p.ensure((size_t)m2 + 1), p, ((size_t)m2 + 1) * 8, hipMemcpyHostToDevice));
      BSN_HIP(hipMemcpy(d_t_p.ensure((size_t)m2 + 1), t_p.data(), ((size_t)m2 + 1) * 8, hipMemcpyHostToDevice));
      BSN_HIP(hipMemcpy(d_up_i.ensure((size_t)nnz), i, (size_t)nnz * 4, hipMemcpyHostToDevice));
      BSN_HIP(hipMemcpy(d_up_x.ensure((size_t)nnz), x, (size_t)nnz * 8, hipMemcpyHostToDevice));
      d_key.ensure((size_t)nnz);
      d_val.ensure((size_t)nnz);
      k_expand_upper<<<(unsigned)((nnz + 255) / 256), 256>>>(d_up_p.p, d_up_i.p, d_up_x.p, m2, nnz, S->p.p, S->i.p, S->x.p,
                                                             d_key.p, d_val.p);
      BSN_HIP(hipGetLastError());
      if (n_off) {
        int end_bit = 32;
        while (end_bit < 64 && ((uint64_t)m2 >> (end_bit - 32))) end_bit++;
        // diagonal keys (all ones) still sort last when only the low end_bit bits are compared
        d_key2.ensure((size_t)nnz);
        d_val2.ensure((size_t)nnz);
        size_t tmp = 0;
        BSN_HIP(rocprim::radix_sort_pairs(nullptr, tmp, d_key.p, d_key2.p, d_val.p, d_val2.p, (size_t)nnz, 0, end_bit,
                                          (hipStream_t) nullptr));
        DevBuf<char> d_tmp;
        d_tmp.ensure(std::max<size_t>(tmp, 1));
        BSN_HIP(rocprim::radix_sort_pairs((void *)d_tmp.p, tmp, d_key.p, d_key2.p, d_val.p, d_val2.p, (size_t)nnz, 0, end_bit,
                                          (hipStream_t) nullptr));
        k_place_transposed<<<(unsigned)((n_off + 255) / 256), 256>>>(d_key2.p, d_val2.p, n_off, d_up_p.p, d_t_p.p, S->p.p,
                                                                     S->i.p, S->x.p);
        BSN_HIP(hipGetLastError());
      }
      BSN_HIP(hipDeviceSynchronize());
    }
    S->lo.resize((size_t)m2);
    S->hi.resize((size_t)m2);
    if (m2) {
      DevBuf<int32_t> d_lo, d_hi;
      k_row_span<<<(unsigned)((m2 + 255) / 256), 256>>>(S->p.p, S->i.p, m2, d_lo.ensure((size_t)m2), d_hi.ensure((size_t)m2));
      BSN_HIP(hipGetLastError());
      BSN_HIP(hipMemcpy(S->lo.data(), d_lo.p, (size_t)m2 * 4, hipMemcpyDeviceToHost));
      BSN_HIP(hipMemcpy(S->hi.data(), d_hi.p, (size_t)m2 * 4, hipMemcpyDeviceToHost));
    }
    for (int64_t j = 0; j < m2; j++)
      if (S->lo[(size_t)j] <= S->hi[(size_t)j])
        S->bandwidth = std::max<int64_t>(S->bandwidth, std::max<int64_t>(j - S->lo[(size_t)j], S->hi[(size_t)j] - j));
    *out = S.release();
  });
}

int bsn_sfbm_ncol(const bsn_sfbm *s, int64_t *m2_out, int64_t *nnz_out, int64_t *bandwidth_out) {
  return guarded([&] {
    if (!s) fail("bsn_sfbm_ncol: NULL handle");
    if (m2_out) *m2_out = s->m2;
    if (nnz_out) *nnz_out = s->nnz;
    if (bandwidth_out) *bandwidth_out = s->bandwidth;
  });
}

int bsn_sfbm_free(bsn_sfbm *s) {
  return guarded([&] { delete s; });
}

int bsn_lassosum2(const bsn_sfbm *s, const double *beta_hat, int64_t m, const double *pf, const double *lambda,
                  const double *delta, int64_t G, const int64_t *ind_sub, double dfmax, int32_t maxiter, double tol,
                  double *beta_out, int32_t *num_iter_out, double *time_out) {
  return guarded([&] {
    if (!s) fail("bsn_lassosum2: NULL 'corr'");
    if (m < 0 || G < 0 || (m > 0 && (!beta_hat || !pf)) || (G > 0 && (!lambda || !delta || !num_iter_out)) ||
        (m > 0 && G > 0 && !beta_out))
      fail("bsn_lassosum2: arguments");
    if (!ind_sub && m != s->m2) fail("bsn_lassosum2: without 'ind_sub', 'beta_hat' needs one entry per column of 'corr'");
    if (ind_sub)
      for (int64_t j = 0; j < m; j++)
        if (ind_sub[j] < 0 || ind_sub[j] >= s->m2) fail("'ind_sub' has %lld out of range [0, %lld).", (long long)ind_sub[j],
                                                        (long long)s->m2);
    if (G == 0) return;
    require_gpu();
    const double gap0 = lassosum2_gap0(beta_hat, m);
    // as many grid points per launch as the free memory holds (dotprods + curr_beta of each, 3/4 of what is free)
    size_t free_b = 0, total_b = 0;
    BSN_HIP(hipMemGetInfo(&free_b, &total_b));
    const int64_t per_g = (s->m2 + m) * 8;
    int64_t batch = G;
    if (per_g > 0) batch = std::min<int64_t>(G, (int64_t)(free_b / 4 * 3) / per_g);
    if (batch < 1) fail("lassosum2: the state of one grid point (%lld B) does not fit the free device memory", (long long)per_g);
    int clock_khz = 0;
    int dev = 0;
    BSN_HIP(hipGetDevice(&dev));
    BSN_HIP(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, dev));
    DevBuf<double> d_bh, d_pf, d_lam, d_del, d_dots, d_curs, d_beta;
    DevBuf<int64_t> d_ind;
    DevBuf<int32_t> d_iter;
    DevBuf<uint64_t> d_ticks;
    const size_t mm = (size_t)std::max<int64_t>(m, 1);
    BSN_HIP(hipMemcpy(d_bh.ensure(mm), beta_hat, (size_t)m * 8, hipMemcpyHostToDevice));
    BSN_HIP(hipMemcpy(d_pf.ensure(mm), pf, (size_t)m * 8, hipMemcpyHostToDevice));
    if (ind_sub) BSN_HIP(hipMemcpy(d_ind.ensure(mm), ind_sub, (size_t)m * 8, hipMemcpyHostToDevice));
    BSN_HIP(hipMemcpy(d_lam.ensure((size_t)G), lambda, (size_t)G * 8, hipMemcpyHostToDevice));
    BSN_HIP(hipMemcpy(d_del.ensure((size_t)G), delta, (size_t)G * 8, hipMemcpyHostToDevice));
    d_dots.ensure((size_t)std::max<int64_t>(batch * s->m2, 1));
    d_curs.ensure((size_t)std::max<int64_t>(batch * m, 1));
    d_beta.ensure((size_t)std::max<int64_t>(G * m, 1));
    d_iter.ensure((size_t)G);
    d_ticks.ensure((size_t)G);
    for (int64_t g0 = 0; g0 < G; g0 += batch) {
      const int64_t nb = std::min<int64_t>(batch, G - g0);
      BSN_HIP(hipMemsetAsync(d_dots.p, 0, (size_t)(nb * s->m2) * 8, nullptr));
      BSN_HIP(hipMemsetAsync(d_curs.p, 0, (size_t)(nb * m) * 8, nullptr));
      k_lassosum2<<<(unsigned)nb, 64>>>(s->p.p, s->i.p, s->x.p, s->m2, d_bh.p, d_pf.p, ind_sub ? d_ind.p : nullptr, m, d_lam.p,
                                        d_del.p, g0, gap0, dfmax, maxiter, tol, d_dots.p, d_curs.p, d_beta.p, d_iter.p,
                                        d_ticks.p);
      BSN_HIP(hipGetLastError());
    }
    if (m > 0) BSN_HIP(hipMemcpy(beta_out, d_beta.p, (size_t)(G * m) * 8, hipMemcpyDeviceToHost));
    BSN_HIP(hipMemcpy(num_iter_out, d_iter.p, (size_t)G * 4, hipMemcpyDeviceToHost));
    if (time_out) {
      std::vector<uint64_t> t((size_t)G);
      BSN_HIP(hipMemcpy(t.data(), d_ticks.p, (size_t)G * 8, hipMemcpyDeviceToHost));
      for (int64_t g = 0; g < G; g++) time_out[g] = clock_khz > 0 ? (double)t[(size_t)g] / (clock_khz * 1e3) : NAN;
    }
  });
}

}  // extern "C"
