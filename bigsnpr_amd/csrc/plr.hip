// plr.hip — big_spLinReg / big_spLogReg (bigstatsr): elastic-net paths on individual-level data, every (alpha, fold)
// chain of the cross-model selection and averaging resident on the device for the whole call.  DESIGN.md 3.5i.
//
// The statement is plr_step.hpp's (shared with tests/native/plr_ref.cpp); this file adds the sums over the rows (fixed
// reduction trees, no float atomics) and the schedule:
//   k_plr_stats    centre and 1 / sd of every column over the training rows of every fold (exact code counts on an image)
//   k_plr_init     one workgroup per chain: intercept, residual (eta), null loss, the unpenalised columns as the first set
//   k_plr_sweep    one workgroup per live chain: the coordinate passes over its active set to their stop inside one
//                  launch, then the two losses and the masked panel m o g of the scan
//   k_plr_scan     x_j' (m o g) for every column against every live chain, one pass over the matrix
//   k_plr_flag     standardises, compares with lambda a pf_j, sets the flags (at the start: |z| / (a pf) for lambda_max)
//   k_plr_commit   one workgroup per chain: rebuilds the ascending list from the flags (ballot compaction: the sweep
//                  order is part of the result) and, when the scan added nothing, closes lambda_l: records, best model,
//                  stopping rules, next lambda
// The host loop is "sweep, scan, flag, commit, read back one record per chain"; kernel boundaries are the only
// grid-wide synchronisation, and every device loop is bounded by an argument (max_iter, |A|, n, p, C).
#include <cmath>
#include <cstring>
#include <limits>

#include "bsn_internal.hpp"
#include "plr_step.hpp"

namespace bsn {
namespace {

using namespace plr;

constexpr int kSweepThreads = 1024, kScanThreads = 256, kChainBlock = 8;

// how a column is read: KIND 0 a 2-bit image, 1 a byte image through its 256-entry table, 2 an fp64 column; the q
// covariates (columns m .. m + q - 1) are fp64 columns in every case
struct Cols {
  const uint8_t *img;
  int64_t pitch;
  const double *tab;
  const double *dense;
  int64_t ld;
  const double *cov;
  int64_t n, m;
};

template <int KIND>
struct Col {
  const uint8_t *b;
  const double *d, *tab;
  __device__ Col(const Cols &X, int64_t j) {
    b = nullptr;
    tab = X.tab;
    if (j >= X.m)
      d = X.cov + (j - X.m) * X.n;
    else if (KIND == 2)
      d = X.dense + j * X.ld;
    else {
      d = nullptr;
      b = X.img + j * X.pitch;
    }
  }
  __device__ bool image() const { return d == nullptr; }
  __device__ int code(int64_t i) const { return KIND == 0 ? (b[i >> 2] >> (2 * (int)(i & 3))) & 3 : (int)(int8_t)b[i]; }
  __device__ double raw(int64_t i) const {
    if (d) return d[i];
    if (KIND == 0) return (double)((b[i >> 2] >> (2 * (int)(i & 3))) & 3);
    return tab[b[i]];
  }
};

struct ChainState {
  double a, lam, b0, nt, nv, nullv, thresh, loss, loss_val, gs, lmax, best_val, best_b0;
  long long updates;   // coordinate updates so far (passes x active columns)
  int32_t status, l, iter_l, nA, best_l, no_change, n_done, added;
};

// what bsn_plr_last_stats reports: the last call's device time in sweeps and in scans (events around the launches of
// every turn), its turns and coordinate updates
double g_last[6] = {0, 0, 0, 0, 0, 0};

struct Args {
  Cols X;
  const double *y, *pf, *alphas;
  const int32_t *fold;
  int K, C;
  int64_t n, p;
  double *cen, *isd;          // K x p
  double *r, *eta, *w, *g;    // n x C (eta, w: logistic only)
  double *beta, *bestb, *P;   // p x C
  uint8_t *flag;              // p x C
  int32_t *list;              // p x C
  ChainState *st;
  const double *lams;         // nlambda x C
  double *o_loss, *o_lossv;
  int32_t *o_iter, *o_nb, *err;
  int family, nlambda, nlam_min, n_abort, dfmax, max_iter;
  double eps;
};

// v[k] <- the sum over the workgroup, in every thread: butterfly inside a wave, then the waves in index order
template <int N, int NT>
__device__ __forceinline__ void block_sum(double (&v)[N], double *lds) {
#pragma unroll
  for (int k = 0; k < N; k++)
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();   // the previous reduction's values are read
  if (lane == 0)
    for (int k = 0; k < N; k++) lds[wave * N + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; k++) {
    double s = 0.0;
    for (int w = 0; w < NT / 64; w++) s += lds[w * N + k];
    v[k] = s;
  }
}
template <int NT>
__device__ __forceinline__ void block_minmax(double &lo, double &hi, double *lds) {
  for (int off = 32; off > 0; off >>= 1) {
    const double l2 = __shfl_down(lo, off, 64), h2 = __shfl_down(hi, off, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) {
    lds[2 * wave] = lo;
    lds[2 * wave + 1] = hi;
  }
  __syncthreads();
  for (int w = 0; w < NT / 64; w++) {
    lo = lds[2 * w] < lo ? lds[2 * w] : lo;
    hi = lds[2 * w + 1] > hi ? lds[2 * w + 1] : hi;
  }
}

// grid (p, K): column j over the training rows of fold k
template <int KIND>
__global__ __launch_bounds__(kScanThreads) void k_plr_stats(Args A, double v_off, double v_step) {
  __shared__ double lds[4 * (kScanThreads / 64)];
  const int64_t j = blockIdx.x;
  const int k = blockIdx.y;
  const Col<KIND> col(A.X, j);
  double v[4] = {0.0, 0.0, 0.0, 0.0};   // image: (n1, n2) or (sum k, sum k^2), missing, nt; dense: sum x, -, not finite, nt
  double lo = inf(), hi = -inf();
  for (int64_t i = threadIdx.x; i < A.n; i += kScanThreads) {
    const double mi = A.fold[i] != k ? 1.0 : 0.0;
    v[3] += mi;
    if (col.image()) {
      const int c = col.code(i);
      if (KIND == 0) {
        v[0] += (c == 1) ? mi : 0.0;
        v[1] += (c == 2) ? mi : 0.0;
        v[2] += (c == 3) ? 1.0 : 0.0;
      } else if (c == -128) {
        v[2] += 1.0;
      } else {
        v[0] += mi * (double)c;
        v[1] += mi * (double)(c * c);
      }
    } else {
      const double x = col.raw(i);
      if (!(absd(x) < inf())) v[2] += 1.0;
      v[0] += mi * x;
      if (mi != 0.0) {
        lo = x < lo ? x : lo;
        hi = x > hi ? x : hi;
      }
    }
  }
  block_sum<4, kScanThreads>(v, lds);
  const double nt = v[3];
  double c, is;
  if (col.image()) {
    if (KIND == 0) {
      const double n0 = nt - v[0] - v[1];
      center_scale_sums(nt, v[0] + 2.0 * v[1], v[0] + 4.0 * v[1], c, is);
      if (n0 == nt || v[0] == nt || v[1] == nt) is = 0.0;
    } else {
      const double S1 = nt * v_off + v_step * v[0];
      const double S2 = nt * (v_off * v_off) + 2.0 * (v_off * v_step) * v[0] + (v_step * v_step) * v[1];
      center_scale_sums(nt, S1, S2, c, is);
      // no variance: nt S2 = S1^2 exactly in the integer sums of k
      if ((__int128)(long long)nt * (__int128)(long long)v[1] == (__int128)(long long)v[0] * (__int128)(long long)v[0]) is = 0.0;
    }
  } else {
    block_minmax<kScanThreads>(lo, hi, lds);
    c = v[0] / nt;
    double ss[1] = {0.0};
    for (int64_t i = threadIdx.x; i < A.n; i += kScanThreads)
      if (A.fold[i] != k) {
        const double d = col.raw(i) - c;
        ss[0] += d * d;
      }
    block_sum<1, kScanThreads>(ss, lds);
    is = inv_scale_ss(nt, ss[0]);
    if (lo == hi) is = 0.0;
  }
  if (threadIdx.x == 0) {
    A.cen[(int64_t)k * A.p + j] = c;
    A.isd[(int64_t)k * A.p + j] = is;
    if (v[2] != 0.0) *A.err = 1;
  }
}

// flags -> the ascending list; returns its length (in every thread)
__device__ int compact(const uint8_t *flag, int32_t *list, int64_t p, int *wsum) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int base = 0;
  for (int64_t j0 = 0; j0 < p; j0 += kSweepThreads) {
    const int64_t j = j0 + threadIdx.x;
    const bool f = j < p && flag[j] != 0;
    const unsigned long long bal = __ballot(f);
    __syncthreads();   // wsum of the previous turn is read
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < kSweepThreads / 64; w++) {
      off += w < wave ? wsum[w] : 0;
      tot += wsum[w];
    }
    if (f) list[base + off + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)j;
    base += tot;
  }
  return base;
}

__global__ __launch_bounds__(kSweepThreads) void k_plr_init(Args A) {
  __shared__ double lds[2 * (kSweepThreads / 64)];
  __shared__ int wsum[kSweepThreads / 64];
  const int c = blockIdx.x, k = c % A.K;
  const int64_t n = A.n, p = A.p;
  double v[2] = {0.0, 0.0};
  for (int64_t i = threadIdx.x; i < n; i += kSweepThreads) {
    const double mi = A.fold[i] != k ? 1.0 : 0.0;
    v[0] += mi;
    v[1] += mi * A.y[i];
  }
  block_sum<2, kSweepThreads>(v, lds);
  const double nt = v[0], ybar = v[1] / nt;
  const double b0 = A.family == 0 ? ybar : logit(ybar);
  double *r = A.r + n * c, *eta = A.family ? A.eta + n * c : nullptr;
  double s[1] = {0.0};
  for (int64_t i = threadIdx.x; i < n; i += kSweepThreads) {
    const double mi = A.fold[i] != k ? 1.0 : 0.0;
    if (A.family == 0) {
      const double ri = A.y[i] - ybar;
      r[i] = ri;
      s[0] += mi * (ri * ri);
    } else {
      eta[i] = b0;
      r[i] = 0.0;
      s[0] += mi * log_loss(b0, A.y[i]);
    }
  }
  block_sum<1, kSweepThreads>(s, lds);
  const double nullv = s[0] / nt;
  uint8_t *flag = A.flag + p * c;
  for (int64_t j = threadIdx.x; j < p; j += kSweepThreads) {
    flag[j] = A.pf[j] == 0.0 && A.isd[(int64_t)k * p + j] != 0.0;
    A.beta[p * c + j] = 0.0;
    A.bestb[p * c + j] = 0.0;
  }
  __syncthreads();
  const int nA = compact(flag, A.list + p * c, p, wsum);
  if (threadIdx.x == 0) {
    ChainState S;
    S.a = A.alphas[c / A.K];
    S.lam = 0.0;
    S.b0 = b0;
    S.nt = nt;
    S.nv = (double)n - nt;
    S.nullv = nullv;
    S.thresh = A.family == 0 ? A.eps * nullv : A.eps * (2.0 * nullv);
    S.loss = S.loss_val = S.gs = S.lmax = 0.0;
    S.best_val = inf();
    S.best_b0 = b0;
    S.status = kLive;
    S.l = 0;
    S.iter_l = 0;
    S.nA = nA;
    S.best_l = 0;
    S.no_change = 0;
    S.n_done = 0;
    S.added = 0;
    S.updates = 0;
    A.st[c] = S;
  }
}

// One workgroup per live chain; a thread owns the rows threadIdx.x + 1024 t in every loop, so the residual needs no
// barrier of its own between a column's dot and its axpy; the coefficients do (thread 0 stores them): one per pass.
template <int KIND, int FAM>
__global__ __launch_bounds__(kSweepThreads) void k_plr_sweep(Args A) {
  __shared__ double lds[3 * (kSweepThreads / 64)];
  const int c = blockIdx.x, k = c % A.K;
  const ChainState S = A.st[c];
  if (S.status != kLive) return;
  const int64_t n = A.n, p = A.p;
  const double nt = S.nt, a = S.a, lam = S.lam;
  double *r = A.r + n * c, *g = A.g + n * c;
  double *eta = FAM ? A.eta + n * c : nullptr, *w = FAM ? A.w + n * c : nullptr;
  double *beta = A.beta + p * c;
  const int32_t *list = A.list + p * c;
  const double *cen = A.cen + (int64_t)k * p, *isd = A.isd + (int64_t)k * p;
  int iter = S.iter_l;
  double b0 = S.b0;
  while (iter < A.max_iter) {
    double maxupd = 0.0;
    if (FAM == 1) {
      double v[2] = {0.0, 0.0};
      for (int64_t i = threadIdx.x; i < n; i += kSweepThreads) {
        double wi, si, ri;
        log_map(eta[i], A.y[i], wi, si, ri);
        w[i] = wi;
        r[i] = ri;
        if (A.fold[i] != k) {
          v[0] += wi;
          v[1] += wi * ri;
        }
      }
      block_sum<2, kSweepThreads>(v, lds);
      const double d = v[1] / v[0];
      b0 = b0 + d;
      for (int64_t i = threadIdx.x; i < n; i += kSweepThreads) {
        r[i] = r[i] - d;
        eta[i] = eta[i] + d;
      }
      maxupd = d * d * (v[0] / nt);
    }
    for (int idx = 0; idx < S.nA; idx++) {
      const int64_t j = list[idx];
      const Col<KIND> col(A.X, j);
      const double cj = cen[j], is = isd[j], bj = beta[j], pfj = A.pf[j];
      double shift, vj = 1.0;
      if (FAM == 0) {
        double v[1] = {0.0};
        for (int64_t i = threadIdx.x; i < n; i += kSweepThreads)
          if (A.fold[i] != k) v[0] += xt(col.raw(i), cj, is) * r[i];
        block_sum<1, kSweepThreads>(v, lds);
        shift = lin_coef(v[0] / nt + bj, lam, a, pfj) - bj;
      } else {
        double v[2] = {0.0, 0.0};
        for (int64_t i = threadIdx.x; i < n; i += kSweepThreads)
          if (A.fold[i] != k) {
            const double t = xt(col.raw(i), cj, is), wi = w[i];
            v[0] += wi * (t * t);
            v[1] += wi * (t * r[i]);
          }
        block_sum<2, kSweepThreads>(v, lds);
        vj = v[0] / nt;
        shift = log_coef(v[1] / nt + vj * bj, vj, lam, a, pfj) - bj;
      }
      if (shift != 0.0) {
        for (int64_t i = threadIdx.x; i < n; i += kSweepThreads) {
          const double t = shift * xt(col.raw(i), cj, is);
          r[i] = r[i] - t;
          if (FAM == 1) eta[i] = eta[i] + t;
        }
        if (threadIdx.x == 0) beta[j] = bj + shift;
        const double up = shift * shift * vj;
        maxupd = up > maxupd ? up : maxupd;
      }
    }
    iter++;
    // thread 0's stores of beta[j] are read by every thread in the next pass: with a single active column of the
    // linear family no reduction (and so no barrier) lies between the two
    __syncthreads();
    if (maxupd < S.thresh) break;
  }
  // the two losses and the masked panel of the scan
  double v[3] = {0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < n; i += kSweepThreads) {
    const bool tr = A.fold[i] != k;
    double li, gi;
    if (FAM == 0) {
      li = r[i] * r[i];
      gi = tr ? r[i] : 0.0;
    } else {
      li = log_loss(eta[i], A.y[i]);
      gi = tr ? log_grad(eta[i], A.y[i]) : 0.0;
    }
    v[0] += tr ? li : 0.0;
    v[1] += tr ? 0.0 : li;
    g[i] = gi;
    v[2] += gi;
  }
  block_sum<3, kSweepThreads>(v, lds);
  if (threadIdx.x == 0) {
    ChainState *o = A.st + c;
    o->loss = v[0] / nt;
    o->loss_val = v[1] / S.nv;
    o->gs = v[2];
    o->iter_l = iter;
    o->b0 = b0;
    o->updates = S.updates + (long long)(iter - S.iter_l) * S.nA;
  }
}

// P[j, c] = sum_i x_ij g_ic for every live chain; the columns are read once per block of kChainBlock chains
template <int KIND>
__global__ __launch_bounds__(kScanThreads) void k_plr_scan(Args A) {
  __shared__ double lds[kChainBlock * (kScanThreads / 64)];
  const int64_t j = blockIdx.x, n = A.n;
  const Col<KIND> col(A.X, j);
  for (int c0 = 0; c0 < A.C; c0 += kChainBlock) {
    bool live[kChainBlock], any = false;
#pragma unroll
    for (int u = 0; u < kChainBlock; u++) {
      live[u] = c0 + u < A.C && A.st[c0 + u].status == kLive;
      any |= live[u];
    }
    if (!any) continue;
    double acc[kChainBlock];
#pragma unroll
    for (int u = 0; u < kChainBlock; u++) acc[u] = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kScanThreads) {
      const double x = col.raw(i);
#pragma unroll
      for (int u = 0; u < kChainBlock; u++)
        if (live[u]) acc[u] += x * A.g[i + n * (c0 + u)];
    }
    block_sum<kChainBlock, kScanThreads>(acc, lds);
    if (threadIdx.x == 0)
#pragma unroll
      for (int u = 0; u < kChainBlock; u++)
        if (live[u]) A.P[j + A.p * (c0 + u)] = acc[u];
  }
}

// grid (ceil(p / 256), C).  start = 1: P <- |z| / (a pf) of the columns that may enter (0 elsewhere), for lambda_max
__global__ void k_plr_flag(Args A, int start) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int c = blockIdx.y;
  if (j >= A.p) return;
  const ChainState *S = A.st + c;
  if (S->status != kLive) return;
  const int k = c % A.K;
  const int64_t o = j + A.p * c;
  const double is = A.isd[(int64_t)k * A.p + j];
  const bool open = is != 0.0 && A.flag[o] == 0;
  const double z = open ? (A.P[o] - A.cen[(int64_t)k * A.p + j] * S->gs) * is / S->nt : 0.0;
  if (start)
    A.P[o] = open ? absd(z) / (S->a * A.pf[j]) : 0.0;
  else if (open && enters(z, S->lam, S->a, A.pf[j]))
    A.flag[o] = 1;
}

__global__ __launch_bounds__(kSweepThreads) void k_plr_lmax(Args A) {
  __shared__ double lds[2 * (kSweepThreads / 64)];
  const int c = blockIdx.x;
  double lo = 0.0, hi = 0.0;
  for (int64_t j = threadIdx.x; j < A.p; j += kSweepThreads) {
    const double t = A.P[j + A.p * c];
    hi = t > hi ? t : hi;
  }
  block_minmax<kSweepThreads>(lo, hi, lds);
  if (threadIdx.x == 0) A.st[c].lmax = hi;
}

// start = 1: closes lambda_0 (the unpenalised fit) once the grid is known
__global__ __launch_bounds__(kSweepThreads) void k_plr_commit(Args A, int start) {
  __shared__ double lds[kSweepThreads / 64];
  __shared__ int wsum[kSweepThreads / 64];
  const int c = blockIdx.x;
  const ChainState S = A.st[c];
  if (S.status != kLive) return;
  const int64_t p = A.p;
  int32_t *list = A.list + p * c;
  const int nA = start ? S.nA : compact(A.flag + p * c, list, p, wsum);
  const int added = nA - S.nA;
  __syncthreads();   // the list is complete (and S was read by every thread)
  if (!(start || added == 0 || S.iter_l >= A.max_iter)) {
    if (threadIdx.x == 0) {
      A.st[c].nA = nA;
      A.st[c].added = added;
    }
    return;
  }
  const double *beta = A.beta + p * c;
  double cnt[1] = {0.0};
  for (int idx = threadIdx.x; idx < nA; idx += kSweepThreads) cnt[0] += beta[list[idx]] != 0.0 ? 1.0 : 0.0;
  block_sum<1, kSweepThreads>(cnt, lds);
  const int nnz = (int)cnt[0], l = S.l;
  Book b{S.best_val, S.best_l, S.no_change};
  bool improved;
  const int st = book(b, l, S.loss_val, A.family == 1 ? S.loss / S.nullv : 1.0, nnz, A.nlambda, A.nlam_min, A.n_abort,
                      A.dfmax, improved);
  if (improved)   // (a coefficient outside the set is 0 in both: the set only grows)
    for (int idx = threadIdx.x; idx < nA; idx += kSweepThreads) A.bestb[p * c + list[idx]] = beta[list[idx]];
  if (threadIdx.x == 0) {
    const int64_t o = l + (int64_t)A.nlambda * c;
    A.o_loss[o] = S.loss;
    A.o_lossv[o] = S.loss_val;
    A.o_iter[o] = S.iter_l;
    A.o_nb[o] = nnz;
    ChainState *t = A.st + c;
    t->nA = nA;
    t->added = added;
    t->best_val = b.best_val;
    t->best_l = b.best_l;
    t->no_change = b.no_change;
    if (improved) t->best_b0 = S.b0;
    t->status = st;
    t->n_done = l + 1;
    if (st == kLive) {
      t->l = l + 1;
      t->lam = A.lams[o + 1];
      t->iter_l = 0;
    }
  }
}

struct Outputs {
  double *intercept, *beta, *lambda, *loss, *loss_val;
  int32_t *iter, *nb_active, *n_done, *best, *status;
};

template <int KIND>
void launch_sweep(const Args &A) {
  if (A.family == 0)
    hipLaunchKernelGGL((k_plr_sweep<KIND, 0>), dim3((unsigned)A.C), dim3(kSweepThreads), 0, 0, A);
  else
    hipLaunchKernelGGL((k_plr_sweep<KIND, 1>), dim3((unsigned)A.C), dim3(kSweepThreads), 0, 0, A);
  BSN_HIP(hipGetLastError());
}

template <int KIND>
void launch_scan(const Args &A, int start) {
  hipLaunchKernelGGL(k_plr_scan<KIND>, dim3((unsigned)A.p), dim3(kScanThreads), 0, 0, A);
  BSN_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_plr_flag, dim3((unsigned)((A.p + 255) / 256), (unsigned)A.C), dim3(256), 0, 0, A, start);
  BSN_HIP(hipGetLastError());
}

// X: the columns on the device (X.cov is filled here).  All work goes to the null stream.
template <int KIND>
void run(Cols X, double v_off, double v_step, int64_t n, int64_t m, const double *y, const double *covar, int64_t q,
         const double *pf, const int32_t *fold, int K, const double *alphas, int n_alpha, const bsn_plr_options *opt,
         const Outputs &out, const char *what) {
  const int64_t p = m + q;
  const int C = K * n_alpha, NL = opt->nlambda;
  // what the chains hold beside the matrix
  const double need = (double)n * C * 8.0 * (opt->family ? 4 : 2) + (double)p * C * (3 * 8.0 + 1 + 4) +
                      (double)K * p * 16.0 + (double)n * q * 8.0 + (double)NL * C * 32.0;
  size_t fr = 0, tot = 0;
  BSN_HIP(hipMemGetInfo(&fr, &tot));
  if (need > 0.9 * ((double)fr + (double)dev_cache_held()))
    fail("%s: the state of the %d chains (%.2f GB) does not fit the device memory that is free beside the matrix (%.2f GB); "
         "use fewer alphas or folds per call", what, C, need / 1e9, ((double)fr + (double)dev_cache_held()) / 1e9);
  DevBuf<double> d_y, d_cov, d_pf, d_al, d_cen, d_isd, d_r, d_eta, d_w, d_g, d_beta, d_bestb, d_P, d_lams, d_ol, d_olv;
  DevBuf<int32_t> d_fold, d_list, d_oi, d_onb, d_err;
  DevBuf<uint8_t> d_flag;
  DevBuf<ChainState> d_st;
  auto up = [](void *d, const void *h, size_t bytes) { BSN_HIP(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice)); };
  up(d_y.ensure((size_t)n), y, (size_t)n * 8);
  if (q) up(d_cov.ensure((size_t)n * q), covar, (size_t)n * q * 8);
  up(d_pf.ensure((size_t)p), pf, (size_t)p * 8);
  up(d_al.ensure((size_t)n_alpha), alphas, (size_t)n_alpha * 8);
  up(d_fold.ensure((size_t)n), fold, (size_t)n * 4);
  X.cov = d_cov.p;
  X.n = n;
  X.m = m;
  Args A{};
  A.X = X;
  A.y = d_y.p;
  A.pf = d_pf.p;
  A.alphas = d_al.p;
  A.fold = d_fold.p;
  A.K = K;
  A.C = C;
  A.n = n;
  A.p = p;
  A.cen = d_cen.ensure((size_t)K * p);
  A.isd = d_isd.ensure((size_t)K * p);
  A.r = d_r.ensure((size_t)n * C);
  A.g = d_g.ensure((size_t)n * C);
  if (opt->family) {
    A.eta = d_eta.ensure((size_t)n * C);
    A.w = d_w.ensure((size_t)n * C);
  }
  A.beta = d_beta.ensure((size_t)p * C);
  A.bestb = d_bestb.ensure((size_t)p * C);
  A.P = d_P.ensure((size_t)p * C);
  A.flag = d_flag.ensure((size_t)p * C);
  A.list = d_list.ensure((size_t)p * C);
  A.st = d_st.ensure((size_t)C);
  A.lams = d_lams.ensure((size_t)NL * C);
  A.o_loss = d_ol.ensure((size_t)NL * C);
  A.o_lossv = d_olv.ensure((size_t)NL * C);
  A.o_iter = d_oi.ensure((size_t)NL * C);
  A.o_nb = d_onb.ensure((size_t)NL * C);
  A.err = d_err.ensure(1);
  A.family = opt->family;
  A.nlambda = NL;
  A.nlam_min = opt->nlam_min;
  A.n_abort = opt->n_abort;
  A.dfmax = opt->dfmax;
  A.max_iter = opt->max_iter;
  A.eps = opt->eps;
  BSN_HIP(hipMemset(A.err, 0, 4));
  BSN_HIP(hipMemset(A.o_loss, 0xff, (size_t)NL * C * 8));    // (all-ones bytes: a NaN where a chain did not get to)
  BSN_HIP(hipMemset(A.o_lossv, 0xff, (size_t)NL * C * 8));
  BSN_HIP(hipMemset(A.o_iter, 0, (size_t)NL * C * 4));
  BSN_HIP(hipMemset(A.o_nb, 0, (size_t)NL * C * 4));
  BSN_HIP(hipMemset(A.P, 0, (size_t)p * C * 8));

  EventMarks<4> ev;
  double ms_sweep = 0, ms_scan = 0;
  ev.mark(3, 0);
  hipLaunchKernelGGL(k_plr_stats<KIND>, dim3((unsigned)p, (unsigned)K), dim3(kScanThreads), 0, 0, A, v_off, v_step);
  BSN_HIP(hipGetLastError());
  int32_t err = 0;
  BSN_HIP(hipMemcpy(&err, A.err, 4, hipMemcpyDeviceToHost));
  if (err)
    fail("You can't have missing values in 'X'.\nImpute them first (snp_fastImputeSimple) or leave their columns out of "
         "'ind.col'.");
  hipLaunchKernelGGL(k_plr_init, dim3((unsigned)C), dim3(kSweepThreads), 0, 0, A);
  BSN_HIP(hipGetLastError());
  // the unpenalised fit, lambda_max, the grid
  launch_sweep<KIND>(A);
  launch_scan<KIND>(A, 1);
  hipLaunchKernelGGL(k_plr_lmax, dim3((unsigned)C), dim3(kSweepThreads), 0, 0, A);
  BSN_HIP(hipGetLastError());
  std::vector<ChainState> st((size_t)C);
  BSN_HIP(hipMemcpy(st.data(), A.st, (size_t)C * sizeof(ChainState), hipMemcpyDeviceToHost));
  for (int c = 0; c < C; c++) {
    if (!(st[(size_t)c].nt >= 1.0 && st[(size_t)c].nv >= 1.0))
      fail("%s: fold %d of 'ind.sets' leaves no training or no validation row.", what, c % K);
    for (int l = 0; l < NL; l++) out.lambda[l + (int64_t)NL * c] = lambda_at(st[(size_t)c].lmax, opt->lambda_min_ratio, l, NL);
  }
  up(d_lams.p, out.lambda, (size_t)NL * C * 8);
  hipLaunchKernelGGL(k_plr_commit, dim3((unsigned)C), dim3(kSweepThreads), 0, 0, A, 1);
  BSN_HIP(hipGetLastError());
  // every turn closes a lambda or grows an active set (or uses up max_iter): at most NL (p + 2) turns per chain
  const int64_t max_turns = (int64_t)NL * (p + 2) + 2;
  ev.mark(0, 0);
  BSN_HIP(hipEventSynchronize(ev.e[0]));
  const double ms_start = ev.ms(3, 0);
  int64_t turn = 0;
  for (;; turn++) {
    BSN_HIP(hipMemcpy(st.data(), A.st, (size_t)C * sizeof(ChainState), hipMemcpyDeviceToHost));
    if (turn > 0) {   // (the copy waited for the turn's kernels)
      ms_sweep += ev.ms(0, 1);
      ms_scan += ev.ms(1, 2);
    }
    bool any = false;
    for (int c = 0; c < C; c++) any |= st[(size_t)c].status == kLive;
    if (!any) break;
    if (turn >= max_turns) fail("%s: internal: the chains did not end", what);
    ev.mark(0, 0);
    launch_sweep<KIND>(A);
    ev.mark(1, 0);
    launch_scan<KIND>(A, 0);
    hipLaunchKernelGGL(k_plr_commit, dim3((unsigned)C), dim3(kSweepThreads), 0, 0, A, 0);
    BSN_HIP(hipGetLastError());
    ev.mark(2, 0);
  }
  long long updates = 0;
  for (int c = 0; c < C; c++) updates += st[(size_t)c].updates;
  g_last[0] = ms_sweep;
  g_last[1] = ms_scan;
  g_last[2] = (double)turn;
  g_last[3] = (double)updates;
  g_last[4] = ms_start;
  g_last[5] = ms_start + ms_sweep + ms_scan;
  // the best model of every chain on the original scale
  std::vector<double> bb((size_t)p * C), cen((size_t)K * p), isd((size_t)K * p);
  BSN_HIP(hipMemcpy(bb.data(), A.bestb, bb.size() * 8, hipMemcpyDeviceToHost));
  BSN_HIP(hipMemcpy(cen.data(), A.cen, cen.size() * 8, hipMemcpyDeviceToHost));
  BSN_HIP(hipMemcpy(isd.data(), A.isd, isd.size() * 8, hipMemcpyDeviceToHost));
  BSN_HIP(hipMemcpy(out.loss, A.o_loss, (size_t)NL * C * 8, hipMemcpyDeviceToHost));
  BSN_HIP(hipMemcpy(out.loss_val, A.o_lossv, (size_t)NL * C * 8, hipMemcpyDeviceToHost));
  BSN_HIP(hipMemcpy(out.iter, A.o_iter, (size_t)NL * C * 4, hipMemcpyDeviceToHost));
  BSN_HIP(hipMemcpy(out.nb_active, A.o_nb, (size_t)NL * C * 4, hipMemcpyDeviceToHost));
  for (int c = 0; c < C; c++) {
#pragma clang fp contract(off)
    const int k = c % K;
    double b = st[(size_t)c].best_b0;
    for (int64_t j = 0; j < p; j++) {
      const double bj = bb[(size_t)(p * c + j)] * isd[(size_t)(k * p + j)];
      out.beta[p * c + j] = bj;
      b = b - cen[(size_t)(k * p + j)] * bj;
    }
    out.intercept[c] = b;
    out.n_done[c] = st[(size_t)c].n_done;
    out.best[c] = st[(size_t)c].best_l;
    out.status[c] = st[(size_t)c].status;
  }
}

void check_args(const char *what, int64_t n, int64_t m, int64_t q, const double *y, const double *covar, const double *pf,
                const int32_t *fold, int K, const double *alphas, int n_alpha, const bsn_plr_options *opt) {
  if (!opt || !y || !pf || !fold || !alphas) fail("%s: a required argument is NULL", what);
  if (n <= 0 || m <= 0) fail("'ind.row' and 'ind.col' can't be empty.");
  if (q < 0 || (q > 0 && !covar)) fail("%s: 'covar.train' is missing", what);
  if (m + q >= ((int64_t)1 << 31) - 1 || n >= ((int64_t)1 << 31) - 1) fail("%s: more than 2^31 - 2 rows or columns", what);
  if (K < 2) fail("%s: 'K' must be at least 2.", what);
  if (n_alpha < 1 || (int64_t)K * n_alpha > 65535) fail("%s: between 1 and 65535 chains (alphas x folds) per call", what);
  if (opt->family != 0 && opt->family != 1) fail("%s: family must be 0 (linear) or 1 (logistic)", what);
  if (opt->nlambda < 2 || opt->max_iter < 1 || opt->n_abort < 1 || opt->dfmax < 1 || opt->nlam_min < 0)
    fail("%s: 'nlambda' >= 2, 'max.iter' >= 1, 'n.abort' >= 1, 'dfmax' >= 1, 'nlam.min' >= 0 are required", what);
  if (!(opt->eps > 0) || !(opt->lambda_min_ratio > 0 && opt->lambda_min_ratio <= 1))
    fail("%s: 'eps' > 0 and 0 < 'lambda.min.ratio' <= 1 are required", what);
  for (int a = 0; a < n_alpha; a++)
    if (!(alphas[a] > 0 && alphas[a] <= 1)) fail("%s: 'alphas' must be in (0, 1].", what);
  for (int64_t j = 0; j < m + q; j++)
    if (!(pf[j] >= 0) || std::isinf(pf[j])) fail("%s: penalty factors must be finite and non-negative.", what);
  for (int64_t i = 0; i < n; i++) {
    if (fold[i] < 0 || fold[i] >= K) fail("%s: 'ind.sets' must hold fold ids in 0 .. K - 1.", what);
    if (!std::isfinite(y[i])) fail("You can't have missing values in 'y.train'.");
    if (opt->family == 1 && y[i] != 0.0 && y[i] != 1.0) fail("'y01.train' should be composed of 0s and 1s.");
  }
  for (int64_t t = 0; t < n * q; t++)
    if (!std::isfinite(covar[t])) fail("You can't have missing values in 'covar.train'.");
}

}  // namespace
}  // namespace bsn

using namespace bsn;

extern "C" {

int bsn_bed_sp_reg(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const double *y,
                   const double *covar, int64_t q, const double *pf, const int32_t *fold, int32_t K, const double *alphas,
                   int32_t n_alpha, const bsn_plr_options *opt, double *intercept, double *beta, double *lambda,
                   double *loss, double *loss_val, int32_t *iter, int32_t *nb_active, int32_t *n_done, int32_t *best,
                   int32_t *status) {
  return guarded([&] {
    const char *what = opt && opt->family ? "big_spLogReg" : "big_spLinReg";
    if (!bed) fail("%s: no handle", what);
    refuse_generic(bed, what);
    require_resident(bed, what);
    check_args(what, n, m, q, y, covar, pf, fold, K, alphas, n_alpha, opt);
    BSN_HIP(hipSetDevice(bed->device));
    // a selection that is not the whole image is compacted once into a private copy in its own code width
    bool whole = n == bed->n && m == bed->m;
    for (int64_t i = 0; whole && ind_row && i < n; i++) whole = ind_row[i] == i;
    for (int64_t j = 0; whole && ind_col && j < m; j++) whole = ind_col[j] == j;
    std::unique_ptr<bsn_bed, void (*)(bsn_bed *)> sub(nullptr, bed_free);
    bsn_bed *im = bed;
    if (!whole) {
      sub.reset(image_gather(bed, ind_row, n, ind_col, m));
      im = sub.get();
    }
    BSN_HIP(hipStreamSynchronize(bed->stream));
    BSN_HIP(hipStreamSynchronize(im->stream));
    DevBuf<double> d_tab;
    Cols X{};
    X.img = im->d_img;
    X.pitch = im->pitch;
    const Outputs out{intercept, beta, lambda, loss, loss_val, iter, nb_active, n_done, best, status};
    if (im->bits == 2) {
      run<0>(X, 0.0, 1.0, n, m, y, covar, q, pf, fold, K, alphas, n_alpha, opt, out, what);
    } else {
      double tab[256];
      for (int b = 0; b < 256; b++) {
#pragma clang fp contract(off)
        const int k = (int8_t)(uint8_t)b;
        tab[b] = k == -128 ? std::numeric_limits<double>::quiet_NaN() : im->v_off + im->v_step * (double)k;
      }
      BSN_HIP(hipMemcpy(d_tab.ensure(256), tab, sizeof tab, hipMemcpyHostToDevice));
      X.tab = d_tab.p;
      run<1>(X, im->v_off, im->v_step, n, m, y, covar, q, pf, fold, K, alphas, n_alpha, opt, out, what);
    }
    BSN_HIP(hipDeviceSynchronize());
  });
}

int bsn_dense_sp_reg(const void *Xh, int type, int64_t ld, int64_t n, int64_t m, const double *y, const double *covar,
                     int64_t q, const double *pf, const int32_t *fold, int32_t K, const double *alphas, int32_t n_alpha,
                     const bsn_plr_options *opt, double *intercept, double *beta, double *lambda, double *loss,
                     double *loss_val, int32_t *iter, int32_t *nb_active, int32_t *n_done, int32_t *best, int32_t *status) {
  return guarded([&] {
    const char *what = opt && opt->family ? "big_spLogReg" : "big_spLinReg";
    require_gpu();
    if (!Xh) fail("%s: no matrix", what);
    if (type != 4 && type != 7) fail("%s: type must be 4 (float) or 7 (double)", what);
    if (ld < n) fail("%s: the leading dimension is smaller than the number of rows", what);
    check_args(what, n, m, q, y, covar, pf, fold, K, alphas, n_alpha, opt);
    // uploaded once as fp64 columns
    std::vector<double> h((size_t)n * m);
    for (int64_t j = 0; j < m; j++)
      for (int64_t i = 0; i < n; i++) {
        const double x = type == 7 ? ((const double *)Xh)[i + j * ld] : (double)((const float *)Xh)[i + j * ld];
        if (!std::isfinite(x))
          fail("You can't have missing values in 'X'.\nImpute them first (snp_fastImputeSimple) or leave their columns "
               "out of 'ind.col'.");
        h[(size_t)(i + j * n)] = x;
      }
    DevBuf<double> d_X;
    BSN_HIP(hipMemcpy(d_X.ensure(h.size()), h.data(), h.size() * 8, hipMemcpyHostToDevice));
    Cols X{};
    X.dense = d_X.p;
    X.ld = n;
    const Outputs out{intercept, beta, lambda, loss, loss_val, iter, nb_active, n_done, best, status};
    run<2>(X, 0.0, 1.0, n, m, y, covar, q, pf, fold, K, alphas, n_alpha, opt, out, what);
    BSN_HIP(hipDeviceSynchronize());
  });
}

/* the last call of this process: out[0] ms in sweeps, [1] ms in scans (scan, flag, commit), [2] turns of the host loop,
 * [3] coordinate updates (passes x active columns, all chains), [4] ms before the first turn (statistics, start fit,
 * lambda_max), [5] their sum; device time from events */
int bsn_plr_last_stats(double *out) {
  return guarded([&] {
    if (!out) fail("bsn_plr_last_stats: no output");
    for (int i = 0; i < 6; i++) out[i] = g_last[i];
  });
}

}  // extern "C"
