// knn.hip — knn_parallel / prob_dist / LOF: the exact k nearest neighbours of every query among the data points, all pairs
// in fp64 on the vector pipe, and the two outlier statistics of bigutilsr over the self-mode table (bsn_knn, bsn_prob_dist,
// bsn_lof, bsn_knn_last_stats).
//
// The outlier-sample step of the reference's PCA workflow (vignettes/bedpca.Rmd: bigutilsr::prob_dist(obj.svd$u)) between
// two bed_autoSVD calls.  At 400 000 x 20 scores a tree search degenerates to brute force; brute force is what runs here.
//
//     k_knn_pack     a column-major matrix -> point-major rows of P = p rounded up to 4 coordinates, zero padded; flags a
//                    non-finite value (NaN breaks the total order of the candidates)
//     k_knn_scan<P, QL>  one lane per query (two where they fit: a coordinate read from LDS then serves two pairs), its
//                    coordinates in registers; the data points of a slab go through LDS in tiles
//                    of 32 and every lane reads them by broadcast; the sorted list of k (squared distance, index) pairs of
//                    every query lives in LDS (indexed dynamically there, never in registers) and its last place is
//                    mirrored in two registers, so a candidate that does not make the list costs one compare
//     k_knn_merge    the k smallest of the S sorted partial lists of a query, by the same total order (S > 1 only)
//     k_knn_sqrt     distances from squared distances
//     k_knn_m2 / k_knn_mean_nn / k_knn_lrd / k_knn_lof   the gathers of the two statistics, sums in the stated order
// The squared distance is the difference form sum (q - x)^2, not the Gram form |q|^2 + |x|^2 - 2 q.x on the f64 MFMA: no
// cancellation between near neighbours, and bit-reproducible against the CPU statement, which an index output needs.  The
// vendor's specification puts the f64 vector and matrix peaks at the same 78.6 TFLOP/s, so the price would be the extra
// subtraction per coordinate; nobody has measured this here (tools/probe_knn.py is the probe).
// The rule (distance, order, self mode, statistics) is knn_step.hpp, the geometry knn_plan.hpp; both are shared with the
// CPU statement (tests/native/knn_ref.cpp).  No atomics on values, no order that depends on the schedule: two calls return
// the same bytes, and so does every slab count.  DESIGN.md 3.5r.
#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <vector>

#include "bsn_internal.hpp"
#include "knn_plan.hpp"
#include "knn_step.hpp"

namespace bsn {
namespace {

// device milliseconds of the last call of this process (bsn_knn_last_stats): packing, scan, merge, what follows the table
// (square roots, statistics, without the download); then the slab count and the query block the call ran with
double g_last[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

// A (rows x p, column-major, leading dimension ld) -> out (rows x P, point-major), coordinates p .. P - 1 zero.  A zero
// coordinate on both sides leaves a squared distance as it is, bit for bit: fma(0, 0, acc) == acc (knn_step.hpp, step).
__global__ __launch_bounds__(256) void k_knn_pack(const double *__restrict__ A, int64_t rows, int64_t ld, int p, int P,
                                                  double *__restrict__ out, int *__restrict__ flag) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;   // e = d * rows + i: the reads are contiguous
  if (e >= rows * P) return;
  const int64_t d = e / rows, i = e - d * rows;
  double v = 0.0;
  if (d < p) {
    v = A[i + d * ld];
    if (!(fabs(v) <= DBL_MAX)) atomicOr(flag, 1);
  }
  out[i * P + d] = v;
}

// Workgroup (b, s) = blockIdx.x = b + nqb * s: queries b * qb .. of the block, data points lo .. hi - 1 of slab s.  A lane
// holds QL queries — the block's queries tid, tid + blockDim.x, ... (qb = QL * blockDim.x) — so that a data coordinate read
// from LDS serves QL pairs.  List of query qi to out[(s * k + t) * nq + qi], t = 0 .. k - 1: with S = 1 that is the n x k
// column-major table.  LDS: the tile (kTile x P doubles), then the lists (k x qb doubles, k x qb int32; place t of the
// block's query l at t * qb + l).
template <int P, int QL>
__global__ __launch_bounds__(256) void k_knn_scan(const double *__restrict__ X, const double *__restrict__ Q, int64_t n, int64_t nq,
                                                  int self, int k, int S, int64_t nqb, double *__restrict__ out_d2,
                                                  int32_t *__restrict__ out_idx) {
  extern __shared__ double s_mem[];
  const int nt = blockDim.x, tid = threadIdx.x, qb = QL * nt;
  double *s_tile = s_mem;
  double *s_d2 = s_mem + knn::kTile * P;
  int32_t *s_idx = (int32_t *)(s_mem + knn::kTile * P + (size_t)k * qb);
  const int64_t b = blockIdx.x % nqb;
  const int s = (int)(blockIdx.x / nqb);
  const int64_t lo = n * (int64_t)s / S, hi = n * (int64_t)(s + 1) / S;   // knn::Plan::lo

  int64_t qi[QL], me[QL];
  bool valid[QL];
  double q[QL][P];
  double wd[QL];   // the last place of each list
  int32_t wi[QL];
#pragma unroll
  for (int c = 0; c < QL; c++) {
    const int l = tid + c * nt;
    qi[c] = b * qb + l;
    valid[c] = qi[c] < nq;
    me[c] = self ? qi[c] : -1;
    const double *qp = Q + (valid[c] ? qi[c] : 0) * P;
#pragma unroll
    for (int d = 0; d < P; d++) q[c][d] = qp[d];
    for (int t = 0; t < k; t++) {
      s_d2[t * qb + l] = knn::no_dist2();
      s_idx[t * qb + l] = knn::kNoIndex;
    }
    wd[c] = knn::no_dist2();
    wi[c] = knn::kNoIndex;
  }

  for (int64_t j0 = lo; j0 < hi; j0 += knn::kTile) {
    const int64_t cnt = hi - j0 < knn::kTile ? hi - j0 : knn::kTile;
    __syncthreads();   // the previous tile has been read
    for (int e = tid; e < knn::kTile * P; e += nt) s_tile[e] = e < cnt * P ? X[j0 * P + e] : 0.0;
    __syncthreads();
    // U data points at a time: QL x U independent chains of fused multiply-adds, each in the order of the statement (two
    // points where the queries alone take more than half of the registers)
    constexpr int U = P * QL <= 32 ? 4 : 2;
    for (int jj = 0; jj < knn::kTile; jj += U) {
      if (jj >= cnt) break;
      const double *x = s_tile + jj * P;
      double a[QL][U];
#pragma unroll
      for (int c = 0; c < QL; c++)
#pragma unroll
        for (int u = 0; u < U; u++) a[c][u] = 0.0;
#pragma unroll
      for (int d = 0; d < P; d++) {
#pragma unroll
        for (int u = 0; u < U; u++) {
          const double xv = x[u * P + d];
#pragma unroll
          for (int c = 0; c < QL; c++) a[c][u] = knn::step(q[c][d], xv, a[c][u]);
        }
      }
#pragma unroll
      for (int c = 0; c < QL; c++) {
        const int l = tid + c * nt;
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int64_t j = j0 + jj + u;
          if (valid[c] && jj + u < cnt && j != me[c] && knn::before(a[c][u], (int32_t)j, wd[c], wi[c])) {
            knn::offer(s_d2 + l, s_idx + l, qb, k, a[c][u], (int32_t)j);
            wd[c] = s_d2[(k - 1) * qb + l];
            wi[c] = s_idx[(k - 1) * qb + l];
          }
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < QL; c++) {
    if (!valid[c]) continue;
    const int l = tid + c * nt;
    for (int t = 0; t < k; t++) {
      out_d2[((int64_t)s * k + t) * nq + qi[c]] = s_d2[t * qb + l];
      out_idx[((int64_t)s * k + t) * nq + qi[c]] = s_idx[t * qb + l];
    }
  }
}

// The k smallest of the S partial lists of every query.  A partial list is sorted, so its first candidate that stays out
// ends it.  LDS: the lists as in the scan.
__global__ __launch_bounds__(256) void k_knn_merge(const double *__restrict__ part_d2, const int32_t *__restrict__ part_idx, int64_t nq,
                                                   int k, int S, double *__restrict__ out_d2, int32_t *__restrict__ out_idx) {
  extern __shared__ double s_mem[];
  const int qb = blockDim.x, tid = threadIdx.x;
  double *s_d2 = s_mem + tid;
  int32_t *s_idx = (int32_t *)(s_mem + (size_t)k * qb) + tid;
  const int64_t qi = (int64_t)blockIdx.x * qb + tid;
  if (qi >= nq) return;
  for (int t = 0; t < k; t++) {
    s_d2[t * qb] = knn::no_dist2();
    s_idx[t * qb] = knn::kNoIndex;
  }
  for (int s = 0; s < S; s++)
    for (int t = 0; t < k; t++) {
      const int64_t at = ((int64_t)s * k + t) * nq + qi;
      if (!knn::offer(s_d2, s_idx, qb, k, part_d2[at], part_idx[at])) break;
    }
  for (int t = 0; t < k; t++) {
    out_d2[(int64_t)t * nq + qi] = s_d2[t * qb];
    out_idx[(int64_t)t * nq + qi] = s_idx[t * qb];
  }
}

__global__ __launch_bounds__(256) void k_knn_sqrt(const double *__restrict__ d2, int64_t count, double *__restrict__ dist) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < count) dist[e] = knn::sqrt_rn(d2[e]);
}

__global__ __launch_bounds__(256) void k_knn_m2(const double *__restrict__ d2, int64_t n, int k, double *__restrict__ m2,
                                                double *__restrict__ dist_self) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double m = knn::mean_d2(d2, n, i, k);
  m2[i] = m;
  dist_self[i] = knn::sqrt_rn(m);
}

__global__ __launch_bounds__(256) void k_knn_mean_nn(const double *__restrict__ v, const int32_t *__restrict__ nn, int64_t n, int k,
                                                     double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = knn::mean_over_nn(v, nn, n, i, k);
}

__global__ __launch_bounds__(256) void k_knn_lrd(const double *__restrict__ dist, const int32_t *__restrict__ nn, int64_t n, int kk,
                                                 double *__restrict__ lrd) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) lrd[i] = knn::lrd(dist, nn, n, i, kk);
}

__global__ __launch_bounds__(256) void k_knn_lof(const double *__restrict__ lrd, const int32_t *__restrict__ nn, int64_t n, int kk,
                                                 double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = knn::lof(lrd, nn, n, i, kk);
}

using ScanFn = void (*)(const double *, const double *, int64_t, int64_t, int, int, int, int64_t, double *, int32_t *);
// Queries per lane: two where both fit the registers (P <= 32) and the block is 256 queries (k <= 16: two waves of 128
// lanes).  Measured at 400 000 x 20 (profiles/knn_scan_ab.txt): two per lane take the scan from 558 to 414 ms at k = 5, but
// from 810 to 1 030 ms at k = 30, where the block of 128 queries becomes a single wave — so one per lane stays there.
int queries_per_lane(int P, int qb) { return P <= 32 && qb >= 256 ? 2 : 1; }
ScanFn scan_of(int P, int QL) {
  if (QL == 2) switch (P) {
      case 4: return k_knn_scan<4, 2>;
      case 8: return k_knn_scan<8, 2>;
      case 12: return k_knn_scan<12, 2>;
      case 16: return k_knn_scan<16, 2>;
      case 20: return k_knn_scan<20, 2>;
      case 24: return k_knn_scan<24, 2>;
      case 28: return k_knn_scan<28, 2>;
      case 32: return k_knn_scan<32, 2>;
    }
  if (QL == 1) switch (P) {
      case 4: return k_knn_scan<4, 1>;
      case 8: return k_knn_scan<8, 1>;
      case 12: return k_knn_scan<12, 1>;
      case 16: return k_knn_scan<16, 1>;
      case 20: return k_knn_scan<20, 1>;
      case 24: return k_knn_scan<24, 1>;
      case 28: return k_knn_scan<28, 1>;
      case 32: return k_knn_scan<32, 1>;
      case 36: return k_knn_scan<36, 1>;
      case 40: return k_knn_scan<40, 1>;
      case 44: return k_knn_scan<44, 1>;
      case 48: return k_knn_scan<48, 1>;
      case 52: return k_knn_scan<52, 1>;
      case 56: return k_knn_scan<56, 1>;
      case 60: return k_knn_scan<60, 1>;
      case 64: return k_knn_scan<64, 1>;
    }
  fail("knn: no scan kernel for %d coordinates, %d queries per lane", P, QL);
}

unsigned blocks256(int64_t count) { return (unsigned)((count + 255) / 256); }

// the table of the k nearest neighbours on the device: squared distances and indices, nq x k column-major
struct Table {
  DevBuf<double> d2;
  DevBuf<int32_t> idx;
  int64_t nq = 0;
  int k = 0;
};

int cu_count() {
  int dev = 0, ncu = 0;
  BSN_HIP(hipGetDevice(&dev));
  BSN_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  return ncu > 0 ? ncu : 256;
}

// d_query == NULL: self mode (the data is its own query; the candidate with the query's own index is left out, by index).
// Marks ev 0 .. 3: start, packed, scanned, merged.
void knn_table(const char *who, const double *d_data, int64_t n, int64_t ld, const double *d_query, int64_t nq, int64_t ldq, int32_t p,
               int32_t k, Table &T, EventMarks<5> &ev) {
  const bool self = d_query == nullptr;
  if (!d_data) fail("%s: null argument", who);
  if (p < 1 || p > knn::kMaxP) fail("%s: 'p' (the number of columns) should be in range [1, %d] (got %d).", who, knn::kMaxP, (int)p);
  if (k < 1 || k > knn::kMaxK) fail("%s: 'k' should be in range [1, %d] (got %d).", who, knn::kMaxK, (int)k);
  if (self) nq = n, ldq = ld;
  if (n < 1 || nq < 1) fail("%s: no point", who);
  if (n >= ((int64_t)1 << 31) || nq >= ((int64_t)1 << 31)) fail("%s: 2^31 points or more (the indices are int32)", who);
  if (ld < n || ldq < nq) fail("%s: Incompatibility between dimensions (leading dimension).", who);
  if (self ? k > n - 1 : k > n)
    fail("%s: 'k' should be at most %lld here (%s; got %d).", who, (long long)(self ? n - 1 : n),
         self ? "the number of points minus one: a point is not its own neighbour" : "the number of data points", (int)k);

  const int P = knn::padded_p(p);
  const char *env = getenv("BSN_KNN_SLABS");
  const knn::Plan plan = knn::plan(n, nq, k, cu_count(), env ? atoll(env) : 0);
  const int S = plan.S;
  const double bytes = (double)(self ? n : n + nq) * P * 8.0 + (double)nq * k * knn::kListBytes * 3.0 + (double)plan.partial_bytes(nq, k);
  size_t free_b = 0, total_b = 0;
  BSN_HIP(hipMemGetInfo(&free_b, &total_b));
  if ((double)(free_b + dev_cache_held()) < bytes + 256e6)
    fail("%s: no room for the workspace (%.1f GB for it, %.1f GB free)", who, bytes / 1e9, (double)free_b / 1e9);

  hipStream_t st = nullptr;
  DevBuf<double> d_X, d_Q, d_part_d2;
  DevBuf<int32_t> d_part_idx;
  DevBuf<int> d_flag;
  d_flag.ensure(2);
  BSN_HIP(hipMemsetAsync(d_flag.p, 0, 8, st));
  ev.mark(0, st);
  d_X.ensure((size_t)n * P);
  hipLaunchKernelGGL(k_knn_pack, dim3(blocks256(n * P)), dim3(256), 0, st, d_data, n, ld, (int)p, P, d_X.p, d_flag.p);
  BSN_HIP(hipGetLastError());
  if (!self) {
    d_Q.ensure((size_t)nq * P);
    hipLaunchKernelGGL(k_knn_pack, dim3(blocks256(nq * P)), dim3(256), 0, st, d_query, nq, ldq, (int)p, P, d_Q.p, d_flag.p + 1);
    BSN_HIP(hipGetLastError());
  }
  ev.mark(1, st);
  int flag[2] = {0, 0};
  BSN_HIP(hipMemcpy(flag, d_flag.p, 8, hipMemcpyDeviceToHost));
  if (flag[0]) fail("%s: non-finite value (NA, NaN or Inf) in 'data'", who);
  if (flag[1]) fail("%s: non-finite value (NA, NaN or Inf) in 'query'", who);

  T.nq = nq;
  T.k = k;
  T.d2.ensure((size_t)nq * k);
  T.idx.ensure((size_t)nq * k);
  double *scan_d2 = T.d2.p;
  int32_t *scan_idx = T.idx.p;
  if (S > 1) {
    scan_d2 = d_part_d2.ensure((size_t)nq * k * S);
    scan_idx = d_part_idx.ensure((size_t)nq * k * S);
  }
  const size_t lds_lists = (size_t)plan.qb * k * knn::kListBytes;
  const size_t lds_scan = (size_t)knn::kTile * P * 8 + lds_lists;
  if (lds_scan > (size_t)knn::kLdsBytes) fail("%s: the lists of a query block do not fit the LDS", who);
  if (plan.nqb * S >= ((int64_t)1 << 31)) fail("%s: too many workgroups (%lld query blocks x %d slabs)", who, (long long)plan.nqb, S);
  const int QL = queries_per_lane(P, plan.qb);
  hipLaunchKernelGGL(scan_of(P, QL), dim3((unsigned)(plan.nqb * S)), dim3(plan.qb / QL), lds_scan, st, d_X.p, self ? d_X.p : d_Q.p, n, nq,
                     self ? 1 : 0, (int)k, S, plan.nqb, scan_d2, scan_idx);
  BSN_HIP(hipGetLastError());
  ev.mark(2, st);
  if (S > 1) {
    hipLaunchKernelGGL(k_knn_merge, dim3((unsigned)plan.nqb), dim3(plan.qb), lds_lists, st, scan_d2, scan_idx, nq, (int)k, S, T.d2.p,
                       T.idx.p);
    BSN_HIP(hipGetLastError());
  }
  ev.mark(3, st);
  g_last[4] = (double)S;
  g_last[5] = (double)plan.qb;
}

// after the call's last kernel: waits, then files the times
void file_times(EventMarks<5> &ev) {
  ev.mark(4, nullptr);
  BSN_HIP(hipStreamSynchronize(nullptr));
  for (int q = 0; q < 4; q++) g_last[q] = ev.ms(q, q + 1);
}

void knn_entry(const double *d_data, int64_t n, int64_t ld, const double *d_query, int64_t nq, int64_t ldq, int32_t p, int32_t k,
               int32_t *idx_out, double *dist_out) {
  if (!idx_out || !dist_out) fail("knn_parallel: null argument");
  Table T;
  EventMarks<5> ev;
  knn_table("knn_parallel", d_data, n, ld, d_query, nq, ldq, p, k, T, ev);
  const int64_t count = T.nq * T.k;
  DevBuf<double> d_dist;
  d_dist.ensure((size_t)count);
  hipLaunchKernelGGL(k_knn_sqrt, dim3(blocks256(count)), dim3(256), 0, nullptr, T.d2.p, count, d_dist.p);
  BSN_HIP(hipGetLastError());
  file_times(ev);
  BSN_HIP(hipMemcpy(idx_out, T.idx.p, (size_t)count * 4, hipMemcpyDeviceToHost));
  BSN_HIP(hipMemcpy(dist_out, d_dist.p, (size_t)count * 8, hipMemcpyDeviceToHost));
}

void prob_dist_entry(const double *d_U, int64_t n, int64_t ld, int32_t p, int32_t kNN, double *dist_self_out, double *dist_nn_out) {
  if (!dist_self_out || !dist_nn_out) fail("prob_dist: null argument");
  Table T;
  EventMarks<5> ev;
  knn_table("prob_dist", d_U, n, ld, nullptr, 0, 0, p, kNN, T, ev);
  DevBuf<double> d_m2, d_self, d_nn;
  d_m2.ensure((size_t)n);
  d_self.ensure((size_t)n);
  d_nn.ensure((size_t)n);
  hipLaunchKernelGGL(k_knn_m2, dim3(blocks256(n)), dim3(256), 0, nullptr, T.d2.p, n, (int)kNN, d_m2.p, d_self.p);
  BSN_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_knn_mean_nn, dim3(blocks256(n)), dim3(256), 0, nullptr, d_m2.p, T.idx.p, n, (int)kNN, d_nn.p);
  BSN_HIP(hipGetLastError());
  file_times(ev);
  BSN_HIP(hipMemcpy(dist_self_out, d_self.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  BSN_HIP(hipMemcpy(dist_nn_out, d_nn.p, (size_t)n * 8, hipMemcpyDeviceToHost));
}

void lof_entry(const double *d_U, int64_t n, int64_t ld, int32_t p, const int32_t *seq_k, int32_t nk, double *lof_out) {
  if (!seq_k || nk < 1 || !lof_out) fail("LOF: 'seq_k' is empty");
  int32_t kmax = 0;
  for (int c = 0; c < nk; c++) {
    if (seq_k[c] < 1 || seq_k[c] > knn::kMaxK) fail("LOF: 'k' should be in range [1, %d] (got %d).", knn::kMaxK, (int)seq_k[c]);
    kmax = std::max(kmax, seq_k[c]);
  }
  Table T;
  EventMarks<5> ev;
  knn_table("LOF", d_U, n, ld, nullptr, 0, 0, p, kmax, T, ev);
  const int64_t count = n * kmax;
  DevBuf<double> d_dist, d_lrd, d_lof;
  d_dist.ensure((size_t)count);
  d_lrd.ensure((size_t)n);
  d_lof.ensure((size_t)n * nk);
  hipLaunchKernelGGL(k_knn_sqrt, dim3(blocks256(count)), dim3(256), 0, nullptr, T.d2.p, count, d_dist.p);
  BSN_HIP(hipGetLastError());
  for (int c = 0; c < nk; c++) {
    hipLaunchKernelGGL(k_knn_lrd, dim3(blocks256(n)), dim3(256), 0, nullptr, d_dist.p, T.idx.p, n, (int)seq_k[c], d_lrd.p);
    BSN_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_knn_lof, dim3(blocks256(n)), dim3(256), 0, nullptr, d_lrd.p, T.idx.p, n, (int)seq_k[c], d_lof.p + (size_t)c * n);
    BSN_HIP(hipGetLastError());
  }
  file_times(ev);
  BSN_HIP(hipMemcpy(lof_out, d_lof.p, (size_t)n * nk * 8, hipMemcpyDeviceToHost));
}

}  // namespace
}  // namespace bsn

extern "C" {

int bsn_knn(const double *d_data, int64_t n, int64_t ld, const double *d_query, int64_t nq, int64_t ldq, int32_t p, int32_t k,
            int32_t *idx_out, double *dist_out) {
  return bsn::guarded([&] {
    bsn::require_gpu();
    bsn::knn_entry(d_data, n, ld, d_query, nq, ldq, p, k, idx_out, dist_out);
  });
}

int bsn_prob_dist(const double *d_U, int64_t n, int64_t ld, int32_t p, int32_t kNN, double *dist_self_out, double *dist_nn_out) {
  return bsn::guarded([&] {
    bsn::require_gpu();
    bsn::prob_dist_entry(d_U, n, ld, p, kNN, dist_self_out, dist_nn_out);
  });
}

int bsn_lof(const double *d_U, int64_t n, int64_t ld, int32_t p, const int32_t *seq_k, int32_t nk, double *lof_out) {
  return bsn::guarded([&] {
    bsn::require_gpu();
    bsn::lof_entry(d_U, n, ld, p, seq_k, nk, lof_out);
  });
}

int bsn_knn_last_stats(double *out) {
  return bsn::guarded([&] {
    for (int q = 0; q < 6; q++) out[q] = bsn::g_last[q];
  });
}

}  // extern "C"
