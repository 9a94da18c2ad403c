// sparse_ld.hip — a sparse LD matrix resident in HBM (bigsparser's SFBM, as R/lassosum2.R receives it through
// `corr`), snp_lassosum2's coordinate descent over it, the whole grid of (lambda, delta) in one launch, and the products
// with it: sp_prodVec, ld_scores_sfbm and sp_solve_sym (MINRES), which snp_ldsc2 and snp_ldpred2_inf run on.
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
#include <cstdlib>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "bsn_internal.hpp"
#include "gibbs_auto.hpp"
#include "gibbs_step.hpp"

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

// chains or grid points per launch: what the free memory holds, or BSN_CHAIN_BATCH=<n> of them if that is fewer (read on
// every call; the seam through which tests/test_gpu_chain_batches.py runs the batch loops of the three drivers)
int64_t chain_batch(int64_t batch) {
  const char *e = getenv("BSN_CHAIN_BATCH");
  const long long n = e ? atoll(e) : 0;
  return n >= 1 ? std::min<int64_t>(batch, n) : batch;
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

// ---- LDpred2-grid's Gibbs sampler (src/ldpred2.cpp:9-69, src/ldpred2-sampling.cpp:9-59) ---------------------------------
// One workgroup of four waves per chain; its dotprods [m2], curr_beta [m] and avg_beta [m] are in HBM.  The structure is
// k_lassosum2's: 64 coordinates are decided against the current dotprods, a coordinate whose diff is exactly 0 changes
// nothing that others read, so every coordinate up to the first with diff != 0 is decided as the sequential loop decides
// it; that one commits, its column is added to dotprods, and the decision resumes behind it.  All four waves decide (the
// same values in the same operations, so they agree without a hand-off; wave 0 alone stores curr_beta, avg_beta and the
// samples), all 256 threads add the column.  Two barriers per decision: one behind the additions, before dotprods is read
// again, and one behind those reads, before a wave that has decided starts adding (the second finds the waves together).
// gap is added in j order, avg_beta[j] touches only j, rows are distinct within a column: every element of dotprods
// receives its additions in the reference's order.  U and Z of a coordinate come from its counter alone (gibbs_step.hpp).
//
// WINDOW: the rows of dotprods that the chain can still touch, [lo[b], hi[b]] of block b (gibbs_envelope), live in LDS as
// a ring of `ring_rows` doubles (row r at r mod ring_rows).  When the block changes, the rows below the new lo go back to
// the chain's HBM vector and the rows up to the new hi come from it; reads and read-modify-writes of a move are LDS
// operations.  The same additions reach the same elements in the same order: the two paths give the same bits.
constexpr int kGibbsThreads = 256;
constexpr int kGibbsAxpy = 8;   // entries per thread and round of a column update (2 048 per round)

// WINDOW: rows wlo .. whi of the chain's dotprods are in the ring.  Before a block with the envelope [nlo, nhi] is worked
// on, the rows below nlo go back to HBM and the rows up to nhi come from it.
__device__ __forceinline__ void ring_advance(double *dot, double *ring, int32_t W, int32_t nlo, int32_t nhi, int32_t &wlo,
                                             int32_t &whi, int tid) {
  if (nlo > wlo || nhi > whi) {
    const int32_t out_end = nlo < whi + 1 ? nlo : whi + 1;    // rows wlo .. out_end - 1 leave
    for (int32_t r = wlo + tid; r < out_end; r += kGibbsThreads) dot[r] = ring[r % W];
    if (out_end > wlo) __syncthreads();   // a row that enters may take the place of one that leaves
    const int32_t in_from = nlo > whi + 1 ? nlo : whi + 1;    // rows in_from .. nhi enter
    for (int32_t r = in_from + tid; r <= nhi; r += kGibbsThreads) ring[r % W] = dot[r];
    wlo = nlo;
    whi = nhi;
    __syncthreads();
  }
}

// the end of a sweep: what is left in the ring goes back to HBM
__device__ __forceinline__ void ring_flush(double *dot, const double *ring, int32_t W, int32_t wlo, int32_t whi, int tid) {
  for (int32_t r = wlo + tid; r <= whi; r += kGibbsThreads) dot[r] = ring[r % W];
  __syncthreads();
}

// dotprods += shift * (stored entries e0 .. e1 - 1 of one column), by all threads of the workgroup: each row once
template <bool WINDOW>
__device__ __forceinline__ void add_column(const int32_t *__restrict__ I, const double *__restrict__ X, int64_t e0, int64_t e1,
                                           double shift, double *dot, double *ring, int32_t wbase, int32_t W, int tid) {
  for (int64_t eb = e0 + tid; eb < e1; eb += kGibbsThreads * kGibbsAxpy) {
    int32_t r[kGibbsAxpy];
    double xv[kGibbsAxpy], dv[kGibbsAxpy];
#pragma unroll
    for (int u = 0; u < kGibbsAxpy; u++) {
      const int64_t e = eb + kGibbsThreads * u;
      r[u] = e < e1 ? I[e] : 0;
      xv[u] = e < e1 ? X[e] : 0.0;
    }
    if (WINDOW) {
#pragma unroll
      for (int u = 0; u < kGibbsAxpy; u++)
        if (eb + kGibbsThreads * u < e1) {
          int32_t q = r[u] - wbase;
          if (q >= W) q -= W;
          ring[q] = ring[q] + xv[u] * shift;
        }
    } else {
#pragma unroll
      for (int u = 0; u < kGibbsAxpy; u++)
        if (eb + kGibbsThreads * u < e1) dv[u] = dot[r[u]];
#pragma unroll
      for (int u = 0; u < kGibbsAxpy; u++)
        if (eb + kGibbsThreads * u < e1) dot[r[u]] = dv[u] + xv[u] * shift;
    }
  }
}

struct GibbsArgs {
  const int64_t *P;
  const int32_t *I;
  const double *X;
  int64_t m2, m;
  const double *beta_hat, *n_vec;
  const int64_t *ind_sub;
  const double *h2, *p;
  const int32_t *sparse;
  const uint64_t *stream;
  const int32_t *order;     // the chain of each workgroup of the call, large p first
  const int32_t *blo, *bhi;   // WINDOW: the envelope per block of 64 positions
  int32_t ring_rows;
  int64_t g0;
  double gap0;
  int burn_in, num_iter;
  uint64_t seed;
  double *dots, *curs, *avgs;
  double *out;   // grid: beta [m x G]; sampling: sample_beta [m x num_iter] of the one chain, zeroed
  uint64_t *ticks;
};

template <bool WINDOW, bool SAMPLING>
__global__ __launch_bounds__(kGibbsThreads) void k_ldpred2_gibbs(const GibbsArgs a) {
  extern __shared__ double ring[];
  const int tid = threadIdx.x, lane = tid & 63;
  const bool writer = tid < 64;
  const int64_t m = a.m;
  const int64_t g = a.order[a.g0 + blockIdx.x];
  double *dot = a.dots + (int64_t)blockIdx.x * a.m2;   // no __restrict__: threads read what other threads stored
  double *cur = a.curs + (int64_t)blockIdx.x * m;
  double *avg = a.avgs + (int64_t)blockIdx.x * m;
  const double p = a.p[g];
  const bool sparse = a.sparse[g] != 0;
  const uint64_t stream = a.stream[g];
  const double h2_per_var = a.h2[g] / (m * p);
  const double inv_odd_p = (1 - p) / p;
  const int32_t W = a.ring_rows;
  const uint64_t t0 = wall_clock64();
  bool diverged = false;
  for (int k = -a.burn_in; k < a.num_iter && !diverged; k++) {
    double gap = 0;
    int32_t wlo = 0, whi = -1, wbase = 0;   // WINDOW: rows wlo .. whi of dot are in the ring; wbase = wlo rounded down to W
    if (WINDOW) {
      wlo = a.blo[0];
      whi = wlo - 1;
    }
    int64_t b = 0;
    for (int64_t j0 = 0; j0 < m; j0 += 64, b++) {
      if (WINDOW) {
        ring_advance(dot, ring, W, a.blo[b], a.bhi[b], wlo, whi, tid);
        wbase = wlo / W * W;
      }
      const int64_t j = j0 + lane;
      const bool in = j < m;
      int64_t j2 = 0, pa = 0, pb = 0;   // the column and its extent: loaded here, ahead of the decision
      int32_t at = 0;                   // WINDOW: where dot[j2] is in the ring
      double bh = 0, cb = 0;
      gibbs::Coord c = {};
      if (in) {
        j2 = a.ind_sub ? a.ind_sub[j] : j;
        pa = a.P[j2];
        pb = a.P[j2 + 1];
        bh = a.beta_hat[j];
        cb = cur[j];
        c = gibbs::coord(a.n_vec[j], h2_per_var, inv_odd_p, gibbs::draw(a.seed, stream, (uint32_t)(k + a.burn_in), (uint32_t)j));
        if (WINDOW) {
          at = (int32_t)j2 - wbase;
          if (at >= W) at -= W;
        }
      }
      int from = 0;   // lanes below `from` are decided
      for (;;) {
        const bool act = in && lane >= from;
        gibbs::Step s = {};
        double dj = 0, sh = 0;
        if (act) dj = WINDOW ? ring[at] : dot[j2];
        // every wave holds its values before any wave, having decided, adds a column: the waves must decide alike
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
        if (act) {
          s = gibbs::step<SAMPLING>(bh, dj, cb, c, p, sparse);
          sh = s.beta - cb;
        }
        const uint64_t moves = __ballot(act && sh != 0);
        const int f = moves ? __ffsll((unsigned long long)moves) - 1 : 64;   // the first coordinate that changes state
        const bool decided = act && lane <= f;
        if (!SAMPLING) {
          uint64_t nz = __ballot(decided && s.nonzero);
          const double sq = s.beta * s.beta;
          while (nz) {
            const int l = __ffsll((unsigned long long)nz) - 1;
            gap += lane_value(sq, l);
            nz &= nz - 1;
          }
        }
        if (writer && decided && s.drawn && k >= 0) {
          if (SAMPLING) a.out[j + (int64_t)k * m] = s.beta;
          else avg[j] += s.mean;
        }
        if (f == 64) break;
        const double shift = lane_value(sh, f);
        if (lane == f) {
          cb = s.beta;
          if (writer) cur[j] = s.beta;
        }
        add_column<WINDOW>(a.I, a.X, lane_index(pa, f), lane_index(pb, f), shift, dot, ring, wbase, W, tid);
        __syncthreads();   // the additions above, before any thread reads dotprods again
        from = f + 1;
        if (from >= 64) break;
      }
    }
    if (WINDOW) ring_flush(dot, ring, W, wlo, whi, tid);
    if (!SAMPLING && gap > a.gap0) diverged = true;
  }
  if (!SAMPLING) {
    __syncthreads();   // wave 0's avg_beta, before every thread reads it
    for (int64_t j = tid; j < m; j += kGibbsThreads) a.out[g * m + j] = diverged ? __builtin_nan("") : avg[j] / a.num_iter;
  }
  if (tid == 0) a.ticks[g] = wall_clock64() - t0;
}

// ---- LDpred2-auto (src/ldpred2-auto.cpp:57-202) ------------------------------------------------------------------------------
// k_ldpred2_gibbs's structure with the coordinate step of gibbs_auto.hpp: one workgroup per chain, 64 coordinates decided
// at a time, the first whose diff is not 0 commits.  cur_h2_est receives a term from committing coordinates only, one per
// decision, so it is added in j order; gap and ind_causal (wave 0 appends, in j order) take every decided causal
// coordinate, the three accumulators every decided coordinate.  The epilogue of a sweep runs on all 256 threads: every
// thread forms p (the same draws, the same operations), the threads stride over the bootstrap and over the sums of the
// MLE, whose partial sums meet in the fixed tree of gibbs_auto.hpp (inside each wave by lane exchange, across the four
// waves through twelve LDS doubles, kept twice so that one barrier per evaluation is enough).  The static LDS comes on
// top of the ring: 128 KiB + 192 B of the CU's 160 KiB.
struct AutoArgs {
  const int64_t *P;
  const int32_t *I;
  const double *X;
  int64_t m2, m;
  const double *beta_hat, *n_vec, *log_var;
  const int64_t *ind_sub;
  const double *p_init;
  const uint64_t *stream;
  const int32_t *order;
  const int32_t *blo, *bhi;
  int32_t ring_rows;
  int64_t g0;
  double gap0, h2_init, shrink_corr, p_lo, p_hi, alpha_lo, alpha_hi, mean_ld;
  int burn_in, num_iter, report_step, n_report, no_jump_sign, use_mle;
  uint64_t seed;
  double *dots, *curs, *avg_beta, *avg_postp, *avg_hat, *boot_a, *boot_b;   // per chain of the batch
  int32_t *causal;
  double *beta_est, *postp_est, *corr_est;   // [m x G]
  double *sample_beta;                       // [m x n_report x G], zeroed
  double *path_p, *path_h2, *path_alpha;     // [(burn_in + num_iter) x G]
  uint64_t *ticks;
};

template <bool WINDOW>
__global__ __launch_bounds__(kGibbsThreads) void k_ldpred2_auto(const AutoArgs a) {
  extern __shared__ double ring[];
  __shared__ double wsum[2][3][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool writer = tid < 64;
  const int64_t m = a.m;
  const int64_t g = a.order[a.g0 + blockIdx.x];
  double *dot = a.dots + (int64_t)blockIdx.x * a.m2;   // no __restrict__: threads read what other threads stored
  double *cur = a.curs + (int64_t)blockIdx.x * m;
  double *avg_beta = a.avg_beta + (int64_t)blockIdx.x * m;
  double *avg_postp = a.avg_postp + (int64_t)blockIdx.x * m;
  double *avg_hat = a.avg_hat + (int64_t)blockIdx.x * m;
  double *ba = a.boot_a + (int64_t)blockIdx.x * m;
  double *bb = a.boot_b + (int64_t)blockIdx.x * m;
  int32_t *causal = a.causal + (int64_t)blockIdx.x * m;
  const uint64_t stream = a.stream[g];
  const bool use_mle = a.use_mle != 0, no_jump = a.no_jump_sign != 0;
  const double shrink = a.shrink_corr;
  const int32_t W = a.ring_rows;
  const int tot = a.burn_in + a.num_iter;
  const uint64_t t0 = wall_clock64();
  double cur_h2 = 0;
  double h2 = a.h2_init < gibbs::kAutoMinH2 ? gibbs::kAutoMinH2 : a.h2_init;
  double p = gibbs::clamp_p(a.p_init[g], a.p_lo, a.p_hi);
  double alpha1 = 0, sigma2 = h2 / (m * p);
  int ind_report = 0, next_report = a.burn_in + a.report_step - 1;
  int flip = 0;
  bool diverged = false;
  int k = 0;
  for (; k < tot; k++) {
    const double inv_odd_p = (1 - p) / p;
    double gap = 0;
    int32_t nbc = 0;   // entries of ind_causal
    int32_t wlo = 0, whi = -1, wbase = 0;
    if (WINDOW) {
      wlo = a.blo[0];
      whi = wlo - 1;
    }
    int64_t b = 0;
    for (int64_t j0 = 0; j0 < m; j0 += 64, b++) {
      if (WINDOW) {
        ring_advance(dot, ring, W, a.blo[b], a.bhi[b], wlo, whi, tid);
        wbase = wlo / W * W;
      }
      const int64_t j = j0 + lane;
      const bool in = j < m;
      int64_t j2 = 0, pa = 0, pb = 0;
      int32_t at = 0;
      double bh = 0, cb = 0;
      gibbs::Coord c = {};
      if (in) {
        j2 = a.ind_sub ? a.ind_sub[j] : j;
        pa = a.P[j2];
        pb = a.P[j2 + 1];
        bh = a.beta_hat[j];
        cb = cur[j];
        c = gibbs::coord_auto(a.n_vec[j], use_mle ? a.log_var[j] : 0.0, alpha1, sigma2, inv_odd_p, use_mle,
                              gibbs::draw(a.seed, stream, (uint32_t)k, (uint32_t)j));
        if (WINDOW) {
          at = (int32_t)j2 - wbase;
          if (at >= W) at -= W;
        }
      }
      int from = 0;   // lanes below `from` are decided
      for (;;) {
        const bool act = in && lane >= from;
        gibbs::StepAuto s = {};
        double dj = 0;
        if (act) dj = WINDOW ? ring[at] : dot[j2];
        // every wave holds its values before any wave, having decided, adds a column: the waves must decide alike
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
        if (act) s = gibbs::step_auto(bh, dj, cb, c, shrink, no_jump);
        const uint64_t moves = __ballot(act && s.diff != 0);
        const int f = moves ? __ffsll((unsigned long long)moves) - 1 : 64;   // the first coordinate that changes state
        const bool decided = act && lane <= f;
        const uint64_t cz = __ballot(decided && s.causal);
        const double sq = s.beta * s.beta;
        for (uint64_t nz = cz; nz; nz &= nz - 1) gap += lane_value(sq, __ffsll((unsigned long long)nz) - 1);
        if (writer && decided) {
          if (s.causal) causal[nbc + __popcll(cz & ((1ull << lane) - 1))] = (int32_t)j;
          if (k >= a.burn_in) {
            avg_postp[j] += s.postp;
            avg_beta[j] += s.mean;
            avg_hat[j] += s.shrunk;
          }
        }
        nbc += __popcll(cz);
        if (f == 64) break;
        const double shift = lane_value(s.diff, f);
        cur_h2 += lane_value(gibbs::h2_term(s), f);
        if (lane == f) {
          cb = s.beta;
          if (writer) cur[j] = s.beta;
        }
        add_column<WINDOW>(a.I, a.X, lane_index(pa, f), lane_index(pb, f), shift, dot, ring, wbase, W, tid);
        __syncthreads();   // the additions above, before any thread reads dotprods again
        from = f + 1;
        if (from >= 64) break;
      }
    }
    if (WINDOW) ring_flush(dot, ring, W, wlo, whi, tid);
    __syncthreads();   // wave 0's curr_beta and ind_causal, before every thread reads them
    if (gap > a.gap0) {
      diverged = true;
      break;
    }
    p = gibbs::next_p(nbc, m, a.mean_ld, a.p_lo, a.p_hi, a.seed, stream, (uint32_t)k);
    h2 = cur_h2 < gibbs::kAutoMinH2 ? gibbs::kAutoMinH2 : cur_h2;
    if (use_mle) {
      if (nbc > 0) {
        for (int32_t kk = tid; kk < nbc; kk += kGibbsThreads) {
          const int32_t jj = causal[gibbs::boot_index(nbc, a.seed, stream, (uint32_t)k, (uint32_t)kk)];
          const double v = cur[jj];
          ba[kk] = a.log_var[jj];
          bb[kk] = v * v;
        }
        __syncthreads();
        const gibbs::MlePar par = gibbs::mle_solve(
            [&](double al) {
              gibbs::MleSums t = gibbs::mle_partial(ba, bb, nbc, al, tid);
              t.a = gibbs::tree_wave(t.a);
              t.S = gibbs::tree_wave(t.S);
              t.Sa = gibbs::tree_wave(t.Sa);
              double(*w)[4] = wsum[flip];
              flip ^= 1;
              if (lane == 0) {
                w[0][wave] = t.a;
                w[1][wave] = t.S;
                w[2][wave] = t.Sa;
              }
              __syncthreads();
              t.a = gibbs::tree_four(w[0][0], w[0][1], w[0][2], w[0][3]);
              t.S = gibbs::tree_four(w[1][0], w[1][1], w[1][2], w[1][3]);
              t.Sa = gibbs::tree_four(w[2][0], w[2][1], w[2][2], w[2][3]);
              return t;
            },
            nbc, a.alpha_lo, a.alpha_hi, sigma2);
        alpha1 = par.alpha1;
        sigma2 = par.sigma2;
      }
    } else {
      sigma2 = h2 / (m * p);
    }
    if (tid == 0) {
      a.path_p[g * tot + k] = p;
      a.path_h2[g * tot + k] = h2;
      a.path_alpha[g * tot + k] = use_mle ? alpha1 - 1 : __builtin_nan("");
    }
    if (k == next_report) {
      double *col = a.sample_beta + (g * a.n_report + ind_report) * m;
      for (int32_t kk = tid; kk < nbc; kk += kGibbsThreads) {
        const int32_t jj = causal[kk];
        col[jj] = cur[jj];
      }
      ind_report++;
      next_report += a.report_step;
    }
    __syncthreads();   // the reads of curr_beta and ind_causal above, before wave 0 writes them in the next sweep
  }
  const double nan = __builtin_nan("");
  for (int64_t j = tid; j < m; j += kGibbsThreads) {
    a.beta_est[g * m + j] = diverged ? nan : avg_beta[j] / a.num_iter;
    a.postp_est[g * m + j] = diverged ? nan : avg_postp[j] / a.num_iter;
    a.corr_est[g * m + j] = diverged ? nan : avg_hat[j] / a.num_iter;
  }
  for (int kk = k + tid; kk < tot; kk += kGibbsThreads) {   // the sweeps a diverged chain did not finish
    a.path_p[g * tot + kk] = nan;
    a.path_h2[g * tot + kk] = nan;
    a.path_alpha[g * tot + kk] = nan;
  }
  if (tid == 0) a.ticks[g] = wall_clock64() - t0;
}

#pragma clang fp contract(on)

// ---- products with the resident matrix: sp_prodVec, ld_scores_sfbm, sp_solve_sym ---------------------------------------
// Every sum below has a fixed order that depends on the shapes only (no floating-point atomics): lanes stride over a
// column and are combined by a butterfly, threads stride over a vector and are combined per block, and the per-block
// partial sums are added up in index order by whoever needs the total.  Two calls on the same inputs give the same bits.

constexpr int kBlock = 256;             // threads per block of every kernel below (4 waves)
constexpr int kShortLanes = 8;          // lanes that share one short column
constexpr int64_t kShortBelow = 64;     // a column with fewer stored entries is "short": 8 lanes, 8 columns to a wave
constexpr int kMaxColBlocks = 2048;     // blocks of a column kernel (waves stride over the columns) ...
constexpr int kMaxVecBlocks = 1024;     // ... and of a vector kernel: as many partial sums at the most

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the sum over the block, in every thread: butterfly inside each wave, then the four wave sums in wave order
__device__ __forceinline__ double block_sum(double v, double *lds) {
  v = wave_sum(v);
  __syncthreads();   // lds may still be read from the previous call
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// second stage of a reduction, done by every block that needs the total: thread t adds part[t], part[t + 256], ... in order
__device__ __forceinline__ double total_of(const double *__restrict__ part, int n, double *lds) {
  double a = 0;
  for (int k = threadIdx.x; k < n; k += kBlock) a += part[k];
  return block_sum(a, lds);
}

// recurrence of the solver, in device memory (two copies: an iteration reads one and writes the other)
struct SolveState {
  double beta, oldb, dbar, epsln, phibar, cs, sn;
  int32_t itn, done, first, pad;
};

__device__ __forceinline__ bool solve_idle(const SolveState *st, int maxiter) { return st->done || st->itn >= maxiter; }

// The column walk.  MODE 0: out = sum_e x_e v[i_e] (+ dg[j2] v[j2]), and the block's share of sum_j out_j v[j2] in
// part[blockIdx.x] when part is given.  MODE 1: out = sum_e x_e^2 over the rows with mask[i_e] != 0 (all rows: mask NULL).
// list [ncols] holds the output positions j served by this launch, ind [m] the column j2 of `corr` behind each (NULL:
// j2 = j); the result goes to out[j2] when `scatter`, else to out[j].
// LANES = 64: one wave per column; the lanes take the entries in aligned pairs (16-byte loads of x, 8-byte loads of i;
// a pair that straddles the column's end is loaded whole and its outside half replaced by zero).  LANES = 8: eight
// columns to a wave, one entry per lane and step.
template <int MODE, int LANES>
__global__ __launch_bounds__(kBlock, 8) void k_columns(const int64_t *__restrict__ P, const int32_t *__restrict__ I,
                                                    const double *__restrict__ X, const int32_t *__restrict__ list,
                                                    int64_t ncols, const int64_t *__restrict__ ind,
                                                    const double *__restrict__ v, const double *__restrict__ dg,
                                                    const uint8_t *__restrict__ mask, double *__restrict__ out, int scatter,
                                                    double *__restrict__ part, const SolveState *__restrict__ st,
                                                    int maxiter) {
  __shared__ double lds[4];
  if (st && solve_idle(st, maxiter)) return;
  const int lane = threadIdx.x % LANES;
  const int64_t group = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
  const int64_t ngroups = (int64_t)gridDim.x * kBlock / LANES;
  double dot = 0;
  for (int64_t c = group; c < ncols; c += ngroups) {
    const int64_t j = list[c];
    const int64_t j2 = ind ? ind[j] : j;
    const int64_t a = P[j2], b = P[j2 + 1];
    double acc0 = 0, acc1 = 0;
    if (LANES == 64) {
#pragma unroll 4
      for (int64_t e = (a & ~(int64_t)1) + 2 * lane; e < b; e += 128) {
        const bool k0 = e >= a, k1 = e + 1 < b;
        const double2 xv = *reinterpret_cast<const double2 *>(X + e);
        const int2 iv = *reinterpret_cast<const int2 *>(I + e);
        const int32_t r0 = k0 ? iv.x : 0, r1 = k1 ? iv.y : 0;
        const double x0 = k0 ? xv.x : 0.0, x1 = k1 ? xv.y : 0.0;
        if (MODE == 0) {
          acc0 += x0 * v[r0];
          acc1 += x1 * v[r1];
        } else {
          acc0 += (!mask || mask[r0]) ? x0 * x0 : 0.0;
          acc1 += (!mask || mask[r1]) ? x1 * x1 : 0.0;
        }
      }
    } else {
      for (int64_t e = a + lane; e < b; e += LANES) {
        const int32_t r = I[e];
        const double x = X[e];
        if (MODE == 0) acc0 += x * v[r];
        else acc0 += (!mask || mask[r]) ? x * x : 0.0;
      }
    }
    double s = acc0 + acc1;
#pragma unroll
    for (int o = LANES / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
      if (MODE == 0) {
        const double vj = v[j2];
        if (dg) s += dg[j2] * vj;
        dot += s * vj;
      }
      out[scatter ? j2 : j] = s;
    }
  }
  if (MODE == 0 && part) {
    const double t = block_sum(dot, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
  }
}

__global__ void k_scatter(const double *__restrict__ src, const int64_t *__restrict__ ind, int64_t m, double *__restrict__ dst) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < m) dst[ind[j]] = src[j];
}

__global__ void k_gather(const double *__restrict__ src, const int64_t *__restrict__ ind, int64_t m, double *__restrict__ dst) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < m) dst[j] = src[ind[j]];
}

__global__ void k_mask(const int64_t *__restrict__ ind, int64_t m, uint8_t *__restrict__ mask) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < m) mask[ind[j]] = 1;   // a repeated index stores the same byte twice
}

// part[blockIdx.x] = this block's share of sum (a - b)^2 (b NULL: sum a^2); diff (may be NULL) receives a - b
__global__ __launch_bounds__(kBlock) void k_sumsq(const double *__restrict__ a, const double *__restrict__ b, int64_t n,
                                                  double *__restrict__ diff, double *__restrict__ part) {
  __shared__ double lds[4];
  double s = 0;
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBlock) {
    const double d = b ? a[k] - b[k] : a[k];
    if (diff) diff[k] = d;
    s += d * d;
  }
  s = block_sum(s, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// MINRES (Paige & Saunders 1975) for (A + D) x = rhs, x being ADDED to: the first Lanczos vector from rhs, whose sum of
// squares is in part [np].  `target` is the absolute residual norm to stop at.
__global__ __launch_bounds__(kBlock) void k_solve_start(const double *__restrict__ rhs, int64_t n, const double *__restrict__ part,
                                                        int np, double target, const SolveState *prev, double *__restrict__ r1,
                                                        double *__restrict__ r2, double *__restrict__ v, double *__restrict__ w1,
                                                        double *__restrict__ w2, SolveState *st) {
  __shared__ double lds[4];
  const int itn0 = prev ? prev->itn : 0;   // read before anything is written: prev is one of st[0], st[1]
  const double beta1 = sqrt(total_of(part, np, lds));
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBlock) {
    const double r = rhs[k];
    r1[k] = r;
    r2[k] = r;
    v[k] = beta1 > 0 ? r / beta1 : 0.0;
    w1[k] = 0;
    w2[k] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    SolveState s;
    s.beta = beta1;
    s.oldb = 0;
    s.dbar = 0;
    s.epsln = 0;
    s.phibar = beta1;
    s.cs = -1;
    s.sn = 0;
    s.itn = itn0;   // a restart goes on counting
    s.done = !(beta1 > target);
    s.first = 1;
    s.pad = 0;
    st[0] = s;
    st[1] = s;
  }
}

// first half of an iteration, after t = (A + D) v and partA = the shares of v . t:
//   alfa = v . t - (beta / oldb) v . r1;  y = t - (beta / oldb) r1 - (alfa / beta) r2;  r1 <- r2;  r2 <- y;  partB = shares of y . y
// (v . r1, zero in exact arithmetic, comes from the previous iteration in partC: Paige and Saunders take alfa after the
// first subtraction)
__global__ __launch_bounds__(kBlock) void k_solve_lanczos(const double *__restrict__ t, double *__restrict__ r1, double *__restrict__ r2,
                                                          int64_t n, const double *__restrict__ partA, int nA,
                                                          const double *__restrict__ partC, int nC, const SolveState *__restrict__ st,
                                                          int maxiter, double *__restrict__ alfa_out, double *__restrict__ partB) {
  __shared__ double lds[4];
  if (solve_idle(st, maxiter)) return;
  const double beta = st->beta;
  const double c0 = st->first ? 0.0 : beta / st->oldb;
  double alfa = total_of(partA, nA, lds);
  if (!st->first) alfa -= c0 * total_of(partC, nC, lds);
  const double c1 = alfa / beta;
  double s = 0;
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBlock) {
    const double r2k = r2[k];
    const double y = (t[k] - c0 * r1[k]) - c1 * r2k;
    r1[k] = r2k;
    r2[k] = y;
    s += y * y;
  }
  s = block_sum(s, lds);
  if (threadIdx.x == 0) {
    partB[blockIdx.x] = s;
    if (blockIdx.x == 0) *alfa_out = alfa;
  }
}

// second half: the plane rotation, w and x, the next Lanczos vector v = r2 / beta and partC = the shares of v . r1.
// Every block forms the same scalars from `cur`; block 0 writes them to `next`.
__global__ __launch_bounds__(kBlock) void k_solve_update(double *__restrict__ v, const double *__restrict__ r1, const double *__restrict__ r2,
                                                         double *__restrict__ w1, double *__restrict__ w2, double *__restrict__ x, int64_t n,
                                                         const double *__restrict__ partB, int nB, const double *__restrict__ alfa_in,
                                                         const SolveState *__restrict__ cur, SolveState *__restrict__ next,
                                                         double target, int maxiter, double *__restrict__ partC) {
  __shared__ double lds[4];
  if (solve_idle(cur, maxiter)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *next = *cur;
    return;
  }
  const double betan = sqrt(total_of(partB, nB, lds));
  const double alfa = *alfa_in;
  const double oldeps = cur->epsln;
  const double delta = cur->cs * cur->dbar + cur->sn * alfa;
  const double gbar = cur->sn * cur->dbar - cur->cs * alfa;
  const double epsln = cur->sn * betan;
  const double dbar = -cur->cs * betan;
  const double gamma = fmax(sqrt(gbar * gbar + betan * betan), 2.220446049250313e-16);
  const double cs = gbar / gamma, sn = betan / gamma;
  const double phi = cs * cur->phibar, phibar = sn * cur->phibar;
  const double denom = 1.0 / gamma;
  double s = 0;
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBlock) {
    const double w2k = w2[k];
    const double wn = ((v[k] - oldeps * w1[k]) - delta * w2k) * denom;
    w1[k] = w2k;
    w2[k] = wn;
    x[k] += phi * wn;
    const double vn = betan > 0 ? r2[k] / betan : 0.0;
    v[k] = vn;
    s += vn * r1[k];
  }
  s = block_sum(s, lds);
  if (threadIdx.x == 0) {
    partC[blockIdx.x] = s;
    if (blockIdx.x == 0) {
      SolveState o;
      o.beta = betan;
      o.oldb = cur->beta;
      o.dbar = dbar;
      o.epsln = epsln;
      o.phibar = phibar;
      o.cs = cs;
      o.sn = sn;
      o.itn = cur->itn + 1;
      o.done = !(phibar > target) || !(betan > 0);
      o.first = 0;
      o.pad = 0;
      *next = o;
    }
  }
}

// which kernel serves which column: the output positions whose column has at least kShortBelow stored entries, then the rest
struct ColumnPlan {
  DevBuf<int32_t> d_list;
  int64_t n_long = 0, n_short = 0;
  int blocks_long = 0, blocks_short = 0;
  int parts() const { return blocks_long + blocks_short; }
};

void plan_columns(const bsn_sfbm *s, const int64_t *ind_sub, int64_t m, ColumnPlan *pl) {
  std::vector<int32_t> list((size_t)std::max<int64_t>(m, 1));
  int64_t nl = 0, ns = 0;
  for (int64_t j = 0; j < m; j++) {
    const int64_t j2 = ind_sub ? ind_sub[j] : j;
    if (s->hp[(size_t)j2 + 1] - s->hp[(size_t)j2] >= kShortBelow) list[(size_t)nl++] = (int32_t)j;
  }
  for (int64_t j = 0; j < m; j++) {
    const int64_t j2 = ind_sub ? ind_sub[j] : j;
    if (s->hp[(size_t)j2 + 1] - s->hp[(size_t)j2] < kShortBelow) list[(size_t)(nl + ns++)] = (int32_t)j;
  }
  pl->n_long = nl;
  pl->n_short = ns;
  pl->blocks_long = (int)std::min<int64_t>((nl + 3) / 4, kMaxColBlocks);
  pl->blocks_short = (int)std::min<int64_t>((ns + kBlock / kShortLanes - 1) / (kBlock / kShortLanes), kMaxColBlocks);
  BSN_HIP(hipMemcpy(pl->d_list.ensure(list.size()), list.data(), list.size() * 4, hipMemcpyHostToDevice));
}

// the two launches of a column walk; part (MODE 0, may be NULL) receives pl.parts() partial sums
template <int MODE>
void launch_columns(const bsn_sfbm *s, const ColumnPlan &pl, const int64_t *d_ind, const double *d_v, const double *d_dg,
                    const uint8_t *d_mask, double *d_out, int scatter, double *d_part, const SolveState *d_st, int maxiter) {
  if (pl.n_long)
    k_columns<MODE, 64><<<pl.blocks_long, kBlock>>>(s->p.p, s->i.p, s->x.p, pl.d_list.p, pl.n_long, d_ind, d_v, d_dg, d_mask,
                                                    d_out, scatter, d_part, d_st, maxiter);
  if (pl.n_short)
    k_columns<MODE, kShortLanes><<<pl.blocks_short, kBlock>>>(s->p.p, s->i.p, s->x.p, pl.d_list.p + pl.n_long, pl.n_short, d_ind,
                                                              d_v, d_dg, d_mask, d_out, scatter,
                                                              d_part ? d_part + pl.blocks_long : nullptr, d_st, maxiter);
  BSN_HIP(hipGetLastError());
}

int vec_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, kMaxVecBlocks)); }

void check_ind_sub(const bsn_sfbm *s, const int64_t *ind_sub, int64_t m, bool refuse_repeats, const char *what) {
  if (m < 0) fail("%s: 'm' is negative", what);
  if (!ind_sub) {
    if (m != s->m2) fail("%s: without 'ind_sub', the vectors need one entry per column of 'corr'", what);
    return;
  }
  std::vector<char> seen(refuse_repeats ? (size_t)s->m2 : 0, 0);
  for (int64_t j = 0; j < m; j++) {
    const int64_t j2 = ind_sub[j];
    if (j2 < 0 || j2 >= s->m2) fail("'ind_sub' has %lld out of range [0, %lld).", (long long)j2, (long long)s->m2);
    if (refuse_repeats) {
      if (seen[(size_t)j2]) fail("%s: 'ind_sub' has %lld more than once.", what, (long long)j2);
      seen[(size_t)j2] = 1;
    }
  }
}

// HIP events around the device work of one call -> s->last_ms
struct CallTimer {
  bsn_sfbm *s;
  EventMarks<2> ev;
  explicit CallTimer(bsn_sfbm *s_) : s(s_) { ev.mark(0, nullptr); }
  void stop() {
    ev.mark(1, nullptr);
    BSN_HIP(hipEventSynchronize(ev.e[1]));
    s->last_ms = ev.ms(0, 1);
  }
};

double host_total(const double *d_part, int n) {
  std::vector<double> h((size_t)n);
  BSN_HIP(hipMemcpy(h.data(), d_part, (size_t)n * 8, hipMemcpyDeviceToHost));
  double t = 0;
  for (int k = 0; k < n; k++) t += h[(size_t)k];
  return t;
}

// Both Gibbs entries: G chains of the grid (sample_out NULL), or one chain's samples.  The checks come before any device work.
void run_gibbs(const bsn_sfbm *s, const double *beta_hat, const double *n_vec, int64_t m, const int64_t *ind_sub,
               const double *h2, const double *p, const int32_t *sparse, const uint64_t *stream, int64_t G, int burn_in,
               int num_iter, uint64_t seed, double *beta_out, double *sample_out, double *seconds_out, const char *what) {
  if (!s) fail("%s: NULL 'corr'", what);
  if (m < 0 || G < 0 || G > 0x7fffffffLL || (m > 0 && (!beta_hat || !n_vec)) || (G > 0 && (!h2 || !p || !sparse)) ||
      (m > 0 && G > 0 && !(sample_out ? sample_out : beta_out)))
    fail("%s: arguments", what);
  check_ind_sub(s, ind_sub, m, true, what);
  for (int64_t g = 0; g < G; g++) {
    if (!(h2[g] > 0)) fail("'h2' should have only positive values.");
    if (!(p[g] > 0 && p[g] <= 1)) fail("'p' should be in (0, 1].");
  }
  if (burn_in < 0) fail("'burn_in' should not be negative.");
  if (num_iter < 1) fail("'num_iter' should be at least 1.");
  if (G == 0 || m == 0) return;
  require_gpu();
  const bool sampling = sample_out != nullptr;
  const double gap0 = lassosum2_gap0(beta_hat, m);   // 2 * inner_product(beta_hat, beta_hat), src/ldpred2.cpp:29-30
  // the path: the LDS window when the visiting order ascends and the envelope fits (BSN_GIBBS_NO_WINDOW=1: never)
  const gibbs::Envelope env = gibbs::gibbs_envelope(s->lo.data(), s->hi.data(), ind_sub, m);
  const bool window = gibbs::gibbs_window_fits(env) && getenv("BSN_GIBBS_NO_WINDOW") == nullptr;
  const int32_t ring_rows = window ? (int32_t)round_up(env.rows, 64) : 0;
  // large p first (R/LDpred2.R:94): the longest chains start first when there are more chains than the device takes at once
  std::vector<int32_t> order((size_t)G);
  for (int64_t g = 0; g < G; g++) order[(size_t)g] = (int32_t)g;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
    if (p[a] != p[b]) return p[a] > p[b];
    if ((sparse[a] != 0) != (sparse[b] != 0)) return sparse[a] == 0;
    return h2[a] > h2[b];
  });
  std::vector<uint64_t> st((size_t)G);
  for (int64_t g = 0; g < G; g++) st[(size_t)g] = stream ? stream[g] : (uint64_t)g;
  // as many chains per launch as the free memory holds (dotprods + curr_beta + avg_beta of each, 3/4 of what is free
  // once the result and the per-call vectors, which stay for the whole call, are taken off)
  size_t free_b = 0, total_b = 0;
  BSN_HIP(hipMemGetInfo(&free_b, &total_b));
  const size_t n_out = (size_t)m * (size_t)(sampling ? num_iter : G);
  const int64_t per_g = (s->m2 + 2 * m) * 8;
  const int64_t fixed_b = (int64_t)n_out * 8 + m * 24 + G * 48 + (int64_t)(env.lo.size() + env.hi.size()) * 4;
  const int64_t batch = chain_batch(std::min<int64_t>(G, std::max<int64_t>((int64_t)(free_b / 4 * 3) - fixed_b, 0) / per_g));
  if (batch < 1)
    fail("%s: the result (%lld B) and the state of one chain (%lld B) do not fit the free device memory", what,
         (long long)fixed_b, (long long)per_g);
  int clock_khz = 0, dev = 0;
  BSN_HIP(hipGetDevice(&dev));
  BSN_HIP(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, dev));
  DevBuf<double> d_bh, d_nv, d_h2, d_p, d_dots, d_curs, d_avgs, d_out;
  DevBuf<int64_t> d_ind;
  DevBuf<int32_t> d_sparse, d_order, d_blo, d_bhi;
  DevBuf<uint64_t> d_stream, d_ticks;
  BSN_HIP(hipMemcpy(d_bh.ensure((size_t)m), beta_hat, (size_t)m * 8, hipMemcpyHostToDevice));
  BSN_HIP(hipMemcpy(d_nv.ensure((size_t)m), n_vec, (size_t)m * 8, hipMemcpyHostToDevice));
  if (ind_sub) BSN_HIP(hipMemcpy(d_ind.ensure((size_t)m), ind_sub, (size_t)m * 8, hipMemcpyHostToDevice));
  BSN_HIP(hipMemcpy(d_h2.ensure((size_t)G), h2, (size_t)G * 8, hipMemcpyHostToDevice));
  BSN_HIP(hipMemcpy(d_p.ensure((size_t)G), p, (size_t)G * 8, hipMemcpyHostToDevice));
  BSN_HIP(hipMemcpy(d_sparse.ensure((size_t)G), sparse, (size_t)G * 4, hipMemcpyHostToDevice));
  BSN_HIP(hipMemcpy(d_order.ensure((size_t)G), order.data(), (size_t)G * 4, hipMemcpyHostToDevice));
  BSN_HIP(hipMemcpy(d_stream.ensure((size_t)G), st.data(), (size_t)G * 8, hipMemcpyHostToDevice));
  if (window) {
    BSN_HIP(hipMemcpy(d_blo.ensure(env.lo.size()), env.lo.data(), env.lo.size() * 4, hipMemcpyHostToDevice));
    BSN_HIP(hipMemcpy(d_bhi.ensure(env.hi.size()), env.hi.data(), env.hi.size() * 4, hipMemcpyHostToDevice));
  }
  d_out.ensure(n_out);
  if (sampling) BSN_HIP(hipMemsetAsync(d_out.p, 0, n_out * 8, nullptr));   // sample_beta starts as zeros
  d_dots.ensure((size_t)(batch * s->m2));
  d_curs.ensure((size_t)(batch * m));
  d_avgs.ensure((size_t)(batch * m));
  d_ticks.ensure((size_t)G);
  GibbsArgs a;
  a.P = s->p.p, a.I = s->i.p, a.X = s->x.p, a.m2 = s->m2, a.m = m;
  a.beta_hat = d_bh.p, a.n_vec = d_nv.p, a.ind_sub = ind_sub ? d_ind.p : nullptr;
  a.h2 = d_h2.p, a.p = d_p.p, a.sparse = d_sparse.p, a.stream = d_stream.p, a.order = d_order.p;
  a.blo = d_blo.p, a.bhi = d_bhi.p, a.ring_rows = ring_rows;
  a.gap0 = gap0, a.burn_in = burn_in, a.num_iter = num_iter, a.seed = seed;
  a.dots = d_dots.p, a.curs = d_curs.p, a.avgs = d_avgs.p, a.out = d_out.p, a.ticks = d_ticks.p;
  const size_t lds = (size_t)ring_rows * 8;
  auto kernel = window ? (sampling ? k_ldpred2_gibbs<true, true> : k_ldpred2_gibbs<true, false>)
                       : (sampling ? k_ldpred2_gibbs<false, true> : k_ldpred2_gibbs<false, false>);
  if (window) BSN_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (int64_t g0 = 0; g0 < G; g0 += batch) {
    const int64_t nb = std::min<int64_t>(batch, G - g0);
    BSN_HIP(hipMemsetAsync(d_dots.p, 0, (size_t)(nb * s->m2) * 8, nullptr));
    BSN_HIP(hipMemsetAsync(d_curs.p, 0, (size_t)(nb * m) * 8, nullptr));
    BSN_HIP(hipMemsetAsync(d_avgs.p, 0, (size_t)(nb * m) * 8, nullptr));
    a.g0 = g0;
    kernel<<<(unsigned)nb, kGibbsThreads, lds>>>(a);
    BSN_HIP(hipGetLastError());
  }
  BSN_HIP(hipMemcpy(sampling ? sample_out : beta_out, d_out.p, n_out * 8, hipMemcpyDeviceToHost));
  if (seconds_out) {
    std::vector<uint64_t> t((size_t)G);
    BSN_HIP(hipMemcpy(t.data(), d_ticks.p, (size_t)G * 8, hipMemcpyDeviceToHost));
    for (int64_t g = 0; g < G; g++) seconds_out[g] = clock_khz > 0 ? (double)t[(size_t)g] / (clock_khz * 1e3) : NAN;
  }
}

// bsn_ldpred2_auto: G chains of LDpred2-auto, batched as run_gibbs batches its chains.  The checks come before any device work.
void run_auto(const bsn_sfbm *s, const double *beta_hat, const double *n_vec, const double *log_var, int64_t m,
              const int64_t *ind_sub, const double *p_init, const uint64_t *stream, int64_t G, double h2_init, int burn_in,
              int num_iter, int report_step, int no_jump_sign, double shrink_corr, int use_mle, double p_lo, double p_hi,
              double alpha_lo, double alpha_hi, double mean_ld, uint64_t seed, double *beta_est, double *postp_est,
              double *corr_est, double *sample_beta, double *path_p, double *path_h2, double *path_alpha, double *seconds_out) {
  const char *what = "bsn_ldpred2_auto";
  if (!s) fail("%s: NULL 'corr'", what);
  if (m < 0 || G < 0 || G > 0x7fffffffLL || (m > 0 && (!beta_hat || !n_vec || (use_mle && !log_var))) || (G > 0 && !p_init) ||
      (m > 0 && G > 0 && (!beta_est || !postp_est || !corr_est)) || (G > 0 && (!path_p || !path_h2 || !path_alpha)))
    fail("%s: arguments", what);
  check_ind_sub(s, ind_sub, m, true, what);
  if (!(h2_init > 0)) fail("'h2_init' should have only positive values.");
  if (burn_in < 0) fail("'burn_in' should not be negative.");
  if (num_iter < 1) fail("'num_iter' should be at least 1.");
  if (report_step < 1) fail("'report_step' should be at least 1.");
  if ((int64_t)burn_in + num_iter >= (1LL << gibbs::kAutoSweepBits))
    fail("'burn_in + num_iter' should be below 2^30: the two top bits of a counter's sweep word tell its purpose.");
  if (!(p_lo > 0 && p_lo <= p_hi && p_hi <= 1)) fail("'p_bounds' should be ordered and in (0, 1].");
  if (!(alpha_lo <= alpha_hi)) fail("'alpha_bounds' should be ordered.");
  if (!(shrink_corr == shrink_corr)) fail("'shrink_corr' should not be missing.");
  if (!(mean_ld > 0)) fail("'mean_ld' should have only positive values.");
  for (int64_t g = 0; g < G; g++)
    if (!(p_init[g] == p_init[g])) fail("'vec_p_init' should not have missing values.");
  if (report_step > num_iter) report_step = num_iter + 1;   // no column is reported either way
  const int64_t n_report = num_iter / report_step;
  if (m > 0 && G > 0 && n_report > 0 && !sample_beta) fail("%s: arguments", what);
  if (G == 0) return;
  const int64_t tot = (int64_t)burn_in + num_iter;
  if (m == 0) {
    for (int64_t t = 0; t < tot * G; t++) path_p[t] = path_h2[t] = path_alpha[t] = NAN;
    return;
  }
  require_gpu();
  const double gap0 = lassosum2_gap0(beta_hat, m);   // src/ldpred2-auto.cpp:96-97
  // the path: run_gibbs's decision
  const gibbs::Envelope env = gibbs::gibbs_envelope(s->lo.data(), s->hi.data(), ind_sub, m);
  const bool window = gibbs::gibbs_window_fits(env) && getenv("BSN_GIBBS_NO_WINDOW") == nullptr;
  const int32_t ring_rows = window ? (int32_t)round_up(env.rows, 64) : 0;
  std::vector<int32_t> order((size_t)G);   // large p first (R/LDpred2.R:231)
  for (int64_t g = 0; g < G; g++) order[(size_t)g] = (int32_t)g;
  std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return p_init[x] > p_init[y]; });
  std::vector<uint64_t> st((size_t)G);
  for (int64_t g = 0; g < G; g++) st[(size_t)g] = stream ? stream[g] : (uint64_t)g;
  // as many chains per launch as the free memory holds: dotprods, curr_beta, three accumulators, the bootstrap's two
  // vectors and ind_causal of each, in 3/4 of what is free once the results and the per-call vectors are taken off
  size_t free_b = 0, total_b = 0;
  BSN_HIP(hipMemGetInfo(&free_b, &total_b));
  const size_t n_est = (size_t)m * (size_t)G, n_smp = (size_t)(m * n_report) * (size_t)G, n_path = (size_t)(tot * G);
  const int64_t per_g = (s->m2 + 6 * m) * 8 + m * 4;
  const int64_t fixed_b = (int64_t)(3 * n_est + n_smp + 3 * n_path) * 8 + m * 32 + G * 32 +
                          (int64_t)(env.lo.size() + env.hi.size()) * 4;
  const int64_t batch = chain_batch(std::min<int64_t>(G, std::max<int64_t>((int64_t)(free_b / 4 * 3) - fixed_b, 0) / per_g));
  if (batch < 1)
    fail("%s: the results (%lld B) and the state of one chain (%lld B) do not fit the free device memory", what,
         (long long)fixed_b, (long long)per_g);
  int clock_khz = 0, dev = 0;
  BSN_HIP(hipGetDevice(&dev));
  BSN_HIP(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, dev));
  DevBuf<double> d_bh, d_nv, d_lv, d_p, d_dots, d_state, d_est, d_smp, d_path;
  DevBuf<int64_t> d_ind;
  DevBuf<int32_t> d_order, d_blo, d_bhi, d_causal;
  DevBuf<uint64_t> d_stream, d_ticks;
  BSN_HIP(hipMemcpy(d_bh.ensure((size_t)m), beta_hat, (size_t)m * 8, hipMemcpyHostToDevice));
  BSN_HIP(hipMemcpy(d_nv.ensure((size_t)m), n_vec, (size_t)m * 8, hipMemcpyHostToDevice));
  if (use_mle) BSN_HIP(hipMemcpy(d_lv.ensure((size_t)m), log_var, (size_t)m * 8, hipMemcpyHostToDevice));
  if (ind_sub) BSN_HIP(hipMemcpy(d_ind.ensure((size_t)m), ind_sub, (size_t)m * 8, hipMemcpyHostToDevice));
  BSN_HIP(hipMemcpy(d_p.ensure((size_t)G), p_init, (size_t)G * 8, hipMemcpyHostToDevice));
  BSN_HIP(hipMemcpy(d_order.ensure((size_t)G), order.data(), (size_t)G * 4, hipMemcpyHostToDevice));
  BSN_HIP(hipMemcpy(d_stream.ensure((size_t)G), st.data(), (size_t)G * 8, hipMemcpyHostToDevice));
  if (window) {
    BSN_HIP(hipMemcpy(d_blo.ensure(env.lo.size()), env.lo.data(), env.lo.size() * 4, hipMemcpyHostToDevice));
    BSN_HIP(hipMemcpy(d_bhi.ensure(env.hi.size()), env.hi.data(), env.hi.size() * 4, hipMemcpyHostToDevice));
  }
  d_est.ensure(3 * n_est);
  d_path.ensure(3 * n_path);
  if (n_smp > 0) BSN_HIP(hipMemsetAsync(d_smp.ensure(n_smp), 0, n_smp * 8, nullptr));   // sample_beta starts as zeros
  d_dots.ensure((size_t)(batch * s->m2));
  d_state.ensure((size_t)(batch * m) * 6);   // curr_beta, avg_beta, avg_postp, avg_beta_hat, then the bootstrap's a and b
  d_causal.ensure((size_t)(batch * m));
  d_ticks.ensure((size_t)G);
  AutoArgs a;
  a.P = s->p.p, a.I = s->i.p, a.X = s->x.p, a.m2 = s->m2, a.m = m;
  a.beta_hat = d_bh.p, a.n_vec = d_nv.p, a.log_var = use_mle ? d_lv.p : nullptr, a.ind_sub = ind_sub ? d_ind.p : nullptr;
  a.p_init = d_p.p, a.stream = d_stream.p, a.order = d_order.p;
  a.blo = d_blo.p, a.bhi = d_bhi.p, a.ring_rows = ring_rows;
  a.gap0 = gap0, a.h2_init = h2_init, a.shrink_corr = shrink_corr, a.p_lo = p_lo, a.p_hi = p_hi;
  a.alpha_lo = alpha_lo, a.alpha_hi = alpha_hi, a.mean_ld = mean_ld;
  a.burn_in = burn_in, a.num_iter = num_iter, a.report_step = report_step, a.n_report = (int)n_report;
  a.no_jump_sign = no_jump_sign, a.use_mle = use_mle, a.seed = seed;
  const size_t bm = (size_t)(batch * m);
  a.dots = d_dots.p, a.curs = d_state.p, a.avg_beta = d_state.p + bm, a.avg_postp = d_state.p + 2 * bm;
  a.avg_hat = d_state.p + 3 * bm, a.boot_a = d_state.p + 4 * bm, a.boot_b = d_state.p + 5 * bm, a.causal = d_causal.p;
  a.beta_est = d_est.p, a.postp_est = d_est.p + n_est, a.corr_est = d_est.p + 2 * n_est, a.sample_beta = d_smp.p;
  a.path_p = d_path.p, a.path_h2 = d_path.p + n_path, a.path_alpha = d_path.p + 2 * n_path, a.ticks = d_ticks.p;
  const size_t lds = (size_t)ring_rows * 8;
  auto kernel = window ? k_ldpred2_auto<true> : k_ldpred2_auto<false>;
  if (window) BSN_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (int64_t g0 = 0; g0 < G; g0 += batch) {
    const int64_t nb = std::min<int64_t>(batch, G - g0);
    BSN_HIP(hipMemsetAsync(d_dots.p, 0, (size_t)(nb * s->m2) * 8, nullptr));
    BSN_HIP(hipMemsetAsync(d_state.p, 0, bm * 4 * 8, nullptr));   // curr_beta and the accumulators
    a.g0 = g0;
    kernel<<<(unsigned)nb, kGibbsThreads, lds>>>(a);
    BSN_HIP(hipGetLastError());
  }
  BSN_HIP(hipMemcpy(beta_est, a.beta_est, n_est * 8, hipMemcpyDeviceToHost));
  BSN_HIP(hipMemcpy(postp_est, a.postp_est, n_est * 8, hipMemcpyDeviceToHost));
  BSN_HIP(hipMemcpy(corr_est, a.corr_est, n_est * 8, hipMemcpyDeviceToHost));
  if (n_smp > 0) BSN_HIP(hipMemcpy(sample_beta, d_smp.p, n_smp * 8, hipMemcpyDeviceToHost));
  BSN_HIP(hipMemcpy(path_p, a.path_p, n_path * 8, hipMemcpyDeviceToHost));
  BSN_HIP(hipMemcpy(path_h2, a.path_h2, n_path * 8, hipMemcpyDeviceToHost));
  BSN_HIP(hipMemcpy(path_alpha, a.path_alpha, n_path * 8, hipMemcpyDeviceToHost));
  if (seconds_out) {
    std::vector<uint64_t> t((size_t)G);
    BSN_HIP(hipMemcpy(t.data(), d_ticks.p, (size_t)G * 8, hipMemcpyDeviceToHost));
    for (int64_t g = 0; g < G; g++) seconds_out[g] = clock_khz > 0 ? (double)t[(size_t)g] / (clock_khz * 1e3) : NAN;
  }
}

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
    S->hp = full_p;
    BSN_HIP(hipMemcpy(S->p.ensure((size_t)m2 + 1), full_p.data(), ((size_t)m2 + 1) * 8, hipMemcpyHostToDevice));
    // two entries of slack: the column kernels load entries in aligned pairs and may touch (never use) the pair after the last
    S->i.ensure((size_t)S->nnz + 2);
    S->x.ensure((size_t)S->nnz + 2);
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
    batch = chain_batch(batch);
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

int bsn_ldpred2_gibbs(const bsn_sfbm *s, const double *beta_hat, const double *n_vec, int64_t m, const int64_t *ind_sub,
                      const double *h2, const double *p, const int32_t *sparse, const uint64_t *stream, int64_t G, int burn_in,
                      int num_iter, uint64_t seed, double *beta_out, double *seconds_out) {
  return guarded([&] {
    run_gibbs(s, beta_hat, n_vec, m, ind_sub, h2, p, sparse, stream, G, burn_in, num_iter, seed, beta_out, nullptr, seconds_out,
              "bsn_ldpred2_gibbs");
  });
}

int bsn_ldpred2_gibbs_sampling(const bsn_sfbm *s, const double *beta_hat, const double *n_vec, int64_t m, const int64_t *ind_sub,
                               double h2, double p, int32_t sparse, uint64_t stream, int burn_in, int num_iter, uint64_t seed,
                               double *sample_out, double *seconds_out) {
  return guarded([&] {
    if (!sample_out && m > 0) fail("bsn_ldpred2_gibbs_sampling: arguments");
    run_gibbs(s, beta_hat, n_vec, m, ind_sub, &h2, &p, &sparse, &stream, 1, burn_in, num_iter, seed, nullptr, sample_out,
              seconds_out, "bsn_ldpred2_gibbs_sampling");
  });
}

int bsn_ldpred2_auto(const bsn_sfbm *s, const double *beta_hat, const double *n_vec, const double *log_var, int64_t m,
                     const int64_t *ind_sub, const double *p_init, const uint64_t *stream, int64_t G, double h2_init,
                     int burn_in, int num_iter, int report_step, int no_jump_sign, double shrink_corr, int use_mle,
                     double p_lo, double p_hi, double alpha_lo, double alpha_hi, double mean_ld, uint64_t seed,
                     double *beta_est, double *postp_est, double *corr_est, double *sample_beta,
                     double *path_p, double *path_h2, double *path_alpha, double *seconds_out) {
  return guarded([&] {
    run_auto(s, beta_hat, n_vec, log_var, m, ind_sub, p_init, stream, G, h2_init, burn_in, num_iter, report_step, no_jump_sign,
             shrink_corr, use_mle, p_lo, p_hi, alpha_lo, alpha_hi, mean_ld, seed, beta_est, postp_est, corr_est, sample_beta,
             path_p, path_h2, path_alpha, seconds_out);
  });
}

int bsn_sfbm_last_ms(const bsn_sfbm *s, double *ms_out) {
  return guarded([&] {
    if (!s || !ms_out) fail("bsn_sfbm_last_ms: NULL argument");
    *ms_out = s->last_ms;
  });
}

int bsn_sfbm_prodvec(bsn_sfbm *s, const double *x, const int64_t *ind_sub, int64_t m, double *y_out) {
  return guarded([&] {
    if (!s) fail("bsn_sfbm_prodvec: NULL 'corr'");
    check_ind_sub(s, ind_sub, m, true, "sp_prodVec");
    if (m > 0 && (!x || !y_out)) fail("bsn_sfbm_prodvec: arguments");
    if (m == 0) return;
    require_gpu();
    ColumnPlan pl;
    plan_columns(s, ind_sub, m, &pl);
    DevBuf<double> d_x, d_v, d_y;
    DevBuf<int64_t> d_ind;
    BSN_HIP(hipMemcpy(d_x.ensure((size_t)m), x, (size_t)m * 8, hipMemcpyHostToDevice));
    d_y.ensure((size_t)m);
    if (ind_sub) {
      BSN_HIP(hipMemcpy(d_ind.ensure((size_t)m), ind_sub, (size_t)m * 8, hipMemcpyHostToDevice));
      d_v.ensure((size_t)s->m2);
    }
    CallTimer timer(s);
    if (ind_sub) {
      BSN_HIP(hipMemsetAsync(d_v.p, 0, (size_t)s->m2 * 8, nullptr));
      k_scatter<<<(unsigned)((m + kBlock - 1) / kBlock), kBlock>>>(d_x.p, d_ind.p, m, d_v.p);
    }
    launch_columns<0>(s, pl, ind_sub ? d_ind.p : nullptr, ind_sub ? d_v.p : d_x.p, nullptr, nullptr, d_y.p, 0, nullptr, nullptr, 0);
    timer.stop();
    BSN_HIP(hipMemcpy(y_out, d_y.p, (size_t)m * 8, hipMemcpyDeviceToHost));
  });
}

int bsn_sfbm_ld_scores(bsn_sfbm *s, const int64_t *ind_sub, int64_t m, double *out) {
  return guarded([&] {
    if (!s) fail("bsn_sfbm_ld_scores: NULL 'corr'");
    check_ind_sub(s, ind_sub, m, false, "ld_scores_sfbm");
    if (m > 0 && !out) fail("bsn_sfbm_ld_scores: arguments");
    if (m == 0) return;
    require_gpu();
    ColumnPlan pl;
    plan_columns(s, ind_sub, m, &pl);
    DevBuf<double> d_y;
    DevBuf<int64_t> d_ind;
    DevBuf<uint8_t> d_mask;
    d_y.ensure((size_t)m);
    if (ind_sub) {
      BSN_HIP(hipMemcpy(d_ind.ensure((size_t)m), ind_sub, (size_t)m * 8, hipMemcpyHostToDevice));
      d_mask.ensure((size_t)s->m2);
    }
    CallTimer timer(s);
    if (ind_sub) {
      BSN_HIP(hipMemsetAsync(d_mask.p, 0, (size_t)s->m2, nullptr));
      k_mask<<<(unsigned)((m + kBlock - 1) / kBlock), kBlock>>>(d_ind.p, m, d_mask.p);
    }
    launch_columns<1>(s, pl, ind_sub ? d_ind.p : nullptr, nullptr, nullptr, ind_sub ? d_mask.p : nullptr, d_y.p, 0, nullptr,
                      nullptr, 0);
    timer.stop();
    BSN_HIP(hipMemcpy(out, d_y.p, (size_t)m * 8, hipMemcpyDeviceToHost));
  });
}

int bsn_sfbm_solve_sym(bsn_sfbm *s, const double *b, const double *add_to_diag, const int64_t *ind_sub, int64_t m, double tol,
                       int32_t maxiter, double *x_out, int32_t *iters_out, double *relres_out) {
  return guarded([&] {
    if (!s) fail("bsn_sfbm_solve_sym: NULL 'corr'");
    check_ind_sub(s, ind_sub, m, true, "sp_solve_sym");
    if (m > 0 && (!b || !add_to_diag || !x_out)) fail("bsn_sfbm_solve_sym: arguments");
    if (!(tol > 0) || maxiter < 1) fail("sp_solve_sym: 'tol' must be positive and 'maxiter' at least 1");
    for (int64_t j = 0; j < m; j++)
      if (!std::isfinite(b[j]) || !std::isfinite(add_to_diag[j])) fail("sp_solve_sym: 'b' and 'add_to_diag' must be finite (element %lld).", (long long)j);
    if (iters_out) *iters_out = 0;
    if (relres_out) *relres_out = 0;
    if (m == 0) return;
    require_gpu();
    const int64_t n = s->m2;   // every vector lives on the columns of `corr`, zero outside the subset
    ColumnPlan pl;
    plan_columns(s, ind_sub, m, &pl);
    const int nv = vec_blocks(n), nA = pl.parts();
    DevBuf<double> d_in, d_ws, d_part, d_alfa;
    DevBuf<int64_t> d_ind;
    DevBuf<SolveState> d_st;
    SolveState *h_st = nullptr;
    BSN_HIP(hipHostMalloc((void **)&h_st, sizeof(SolveState), hipHostMallocDefault));
    std::unique_ptr<SolveState, void (*)(SolveState *)> h_guard(h_st, [](SolveState *p) { (void)hipHostFree(p); });
    d_in.ensure((size_t)(2 * m));
    BSN_HIP(hipMemcpy(d_in.p, b, (size_t)m * 8, hipMemcpyHostToDevice));
    BSN_HIP(hipMemcpy(d_in.p + m, add_to_diag, (size_t)m * 8, hipMemcpyHostToDevice));
    if (ind_sub) BSN_HIP(hipMemcpy(d_ind.ensure((size_t)m), ind_sub, (size_t)m * 8, hipMemcpyHostToDevice));
    d_ws.ensure((size_t)(10 * n));
    double *rhs = d_ws.p, *dg = rhs + n, *r1 = dg + n, *r2 = r1 + n, *v = r2 + n, *t = v + n, *w1 = t + n, *w2 = w1 + n,
           *x = w2 + n, *bb = x + n;
    d_part.ensure((size_t)(nA + 2 * nv));
    double *partA = d_part.p, *partB = partA + nA, *partC = partB + nv;
    d_alfa.ensure(1);
    d_st.ensure(2);
    CallTimer timer(s);
    BSN_HIP(hipMemsetAsync(d_ws.p, 0, (size_t)(10 * n) * 8, nullptr));
    const unsigned gm = (unsigned)((m + kBlock - 1) / kBlock);
    if (ind_sub) {
      k_scatter<<<gm, kBlock>>>(d_in.p, d_ind.p, m, bb);
      k_scatter<<<gm, kBlock>>>(d_in.p + m, d_ind.p, m, dg);
    } else {
      BSN_HIP(hipMemcpyAsync(bb, d_in.p, (size_t)m * 8, hipMemcpyDeviceToDevice, nullptr));
      BSN_HIP(hipMemcpyAsync(dg, d_in.p + m, (size_t)m * 8, hipMemcpyDeviceToDevice, nullptr));
    }
    BSN_HIP(hipMemcpyAsync(rhs, bb, (size_t)n * 8, hipMemcpyDeviceToDevice, nullptr));
    k_sumsq<<<nv, kBlock>>>(bb, nullptr, n, nullptr, partB);
    BSN_HIP(hipGetLastError());
    const double bnorm = std::sqrt(host_total(partB, nv));
    double relres = 0;
    int32_t iters = 0;
    if (bnorm > 0) {
      const double target = tol * bnorm;
      const int64_t *ind = ind_sub ? d_ind.p : nullptr;
      constexpr int kPoll = 8;   // iterations queued between two looks at the state
      int cur = 0;
      for (bool restart = false;; restart = true) {
        // (partB holds the shares of rhs . rhs: of b . b at first, of the true residual's after a restart)
        k_solve_start<<<nv, kBlock>>>(rhs, n, partB, nv, target, restart ? d_st.p + cur : nullptr, r1, r2, v, w1, w2, d_st.p);
        BSN_HIP(hipGetLastError());
        cur = 0;
        for (;;) {
          for (int k = 0; k < kPoll; k++, cur ^= 1) {
            launch_columns<0>(s, pl, ind, v, dg, nullptr, t, 1, partA, d_st.p + cur, maxiter);
            k_solve_lanczos<<<nv, kBlock>>>(t, r1, r2, n, partA, nA, partC, nv, d_st.p + cur, maxiter, d_alfa.p, partB);
            k_solve_update<<<nv, kBlock>>>(v, r1, r2, w1, w2, x, n, partB, nv, d_alfa.p, d_st.p + cur, d_st.p + (cur ^ 1), target,
                                           maxiter, partC);
            BSN_HIP(hipGetLastError());
          }
          BSN_HIP(hipMemcpyAsync(h_st, d_st.p + cur, sizeof(SolveState), hipMemcpyDeviceToHost, nullptr));
          BSN_HIP(hipStreamSynchronize(nullptr));
          if (h_st->done || h_st->itn >= maxiter) break;
        }
        iters = h_st->itn;
        // the TRUE residual b - (A + D) x, which also is the right-hand side of a restart
        launch_columns<0>(s, pl, ind, x, dg, nullptr, t, 1, nullptr, nullptr, 0);
        k_sumsq<<<nv, kBlock>>>(bb, t, n, rhs, partB);
        BSN_HIP(hipGetLastError());
        relres = std::sqrt(host_total(partB, nv)) / bnorm;
        if (relres <= tol || iters >= maxiter || !std::isfinite(relres)) break;
      }
    }
    if (ind_sub) {
      k_gather<<<gm, kBlock>>>(x, d_ind.p, m, t);
      BSN_HIP(hipGetLastError());
    }
    timer.stop();
    BSN_HIP(hipMemcpy(x_out, ind_sub ? t : x, (size_t)m * 8, hipMemcpyDeviceToHost));
    if (iters_out) *iters_out = iters;
    if (relres_out) *relres_out = relres;
    if (!(relres <= tol))
      fail("sp_solve_sym: not converged after %d iterations: relative residual %.3e > tol = %.3e.", (int)iters, relres, tol);
  });
}

}  // extern "C"
