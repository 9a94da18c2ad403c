// auc.hip — scoring a grid of models on the device: bsn_bed_prodmat (big_prodMat), bsn_auc (AUC of K score columns, and
// snp_grid_AUC's sums over chromosomes), bsn_auc_boot / bsn_auc_boot_draws (AUCBoot) and bsn_pcor_moments (pcor).  The rule
// — the keys, the exact integer form of the AUC, the resample rule — is stated in auc_step.hpp, shared with the CPU
// statement (tests/native/auc_ref.cpp).  DESIGN.md 3.5t.
//
// AUC of a batch of columns:
//   k_auc_keys<T>   one thread per (row, column): the fp64 sum of the column's members (one member for AUC, one per
//                   chromosome for snp_grid_AUC, ascending), its order-preserving key, the row as the value; a NaN folds
//                   its column into an atomic minimum ("first NaN column").
//   rocprim         segmented_radix_sort_pairs over the batch, one segment per column (radix_sort_pairs for one column).
//   k_auc_groups    one workgroup per column walks the sorted keys in tiles: heads of tie groups, their running count (the
//                   group id) by a workgroup prefix sum, code[row] = 2 gid + y[row], and one integer atomic per row on
//                   hist[code].  Atomics make a tie group that straddles a tile no special case.
//   k_auc_eval      one workgroup per column: twoU = sum_g c1_g (2 sum_{h<g} c0_h + c0_g) by a prefix sum over the groups.
// AUCBoot, the hot path (nboot x n draws per column):
//   k_auc_boot      a workgroup takes replicates r, r + grid, ...: it generates the replicate's draws (one Philox block
//                   per four draws), adds 1 to hist[code[row]] of ITS histogram in global memory (2 G counters, L2 atomics;
//                   the order of additions is immaterial: integers), evaluates it with the prefix sum of k_auc_eval and
//                   leaves it zeroed for its next replicate.  One form: the histogram of a continuous score has G = n
//                   groups, 8 n bytes, which fits LDS for n <= 8192 only.
// pcor: k_pcor_qtx (a = Q'x) and k_pcor_resid (e = x - Q a; e'e, e'r_y) over row slabs of auc::kPcorSlabRows rows, the
// per-slab sums added in ascending slab order by k_pcor_sum: no atomics, the same bits in every run.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>
#include <climits>
#include <cstring>
#include <limits>

#include "auc_step.hpp"
#include "bsn_internal.hpp"

namespace bsn {
namespace {

// device milliseconds of the last call of this process (bsn_auc_last_ms): key pass, sort, group + evaluation kernels,
// bootstrap kernel, pcor passes
double g_last_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};

constexpr int kThreads = 256;
constexpr int kItems = 8;                       // sorted positions (or groups) of one thread in one tile
constexpr int kTile = kThreads * kItems;
constexpr int kBootMaxGroups = 1024;            // workgroups of one bootstrap launch, at most
constexpr int64_t kBootLaunchDraws = (int64_t)1 << 32;
constexpr int64_t kMaxBatch = 65535;            // gridDim.y

// BSN_AUC_BATCH=<n>: at most n columns per sort batch and n replicates per bootstrap launch (read on every call)
int64_t batch_cap() {
  const char *e = getenv("BSN_AUC_BATCH");
  if (!e || !*e) return kMaxBatch;
  const long long v = atoll(e);
  if (v < 1) fail("BSN_AUC_BATCH should be a positive number (got '%s')", e);
  return std::min<int64_t>(v, kMaxBatch);
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// exclusive prefix sum of one uint32 per thread over the workgroup; *total: the sum.  sh: kThreads words.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *sh, uint32_t *total) {
  const int tid = (int)threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int off = 1; off < kThreads; off <<= 1) {
    const uint32_t t = tid >= off ? sh[tid - off] : 0u;
    __syncthreads();
    sh[tid] += t;
    __syncthreads();
  }
  const uint32_t incl = sh[tid];
  *total = sh[kThreads - 1];
  __syncthreads();
  return incl - v;
}

template <class T>
__global__ __launch_bounds__(kThreads) void k_auc_keys(const T *__restrict__ x, int64_t ld, int64_t sum_stride, int nsum,
                                                       const int32_t *__restrict__ rows, uint32_t n, int col0,
                                                       uint64_t *__restrict__ keys, uint32_t *__restrict__ vals, int *first_nan) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int j = (int)blockIdx.y;
  const T *p = x + (rows ? (int64_t)rows[i] : (int64_t)i) + (int64_t)j * ld;
  double s = (double)p[0];
  for (int c = 1; c < nsum; c++) s += (double)p[(int64_t)c * sum_stride];
  if (auc::is_nan(s)) atomicMin(first_nan, col0 + j);
  keys[(size_t)j * n + i] = auc::order_key(s);
  vals[(size_t)j * n + i] = i;
}

// column j of the batch: keys and rows sorted by key -> code[row] = 2 gid + y[row], hist[code] += 1, ngroups[j] = G
__global__ __launch_bounds__(kThreads) void k_auc_groups(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                         const uint8_t *__restrict__ y, uint32_t n, uint32_t *__restrict__ code,
                                                         uint32_t *__restrict__ hist, uint32_t *__restrict__ ngroups) {
  __shared__ uint32_t sh[kThreads];
  const int tid = (int)threadIdx.x;
  const size_t j = blockIdx.x;
  keys += j * n, vals += j * n, code += j * n, hist += j * 2 * (size_t)n;
  uint32_t carry = 0;   // groups that began before this tile
  for (uint32_t t0 = 0; t0 < n; t0 += kTile) {
    const uint32_t lo = t0 + (uint32_t)tid * kItems;
    uint32_t head[kItems], cnt = 0;
#pragma unroll
    for (int k = 0; k < kItems; k++) {
      const uint32_t p = lo + k;
      head[k] = p < n && (p == 0 || keys[p] != keys[p - 1]) ? 1u : 0u;
      cnt += head[k];
    }
    uint32_t total;
    uint32_t g = carry + block_excl_scan(cnt, sh, &total);   // groups begun before this thread's first position
#pragma unroll
    for (int k = 0; k < kItems; k++) {
      const uint32_t p = lo + k;
      g += head[k];
      if (p < n) {
        const uint32_t row = vals[p], c = 2u * (g - 1u) + (uint32_t)y[row];
        code[row] = c;
        atomicAdd(&hist[c], 1u);
      }
    }
    carry += total;
  }
  if (tid == 0) ngroups[j] = carry;
}

// twoU, n1, n0 of one histogram by a prefix sum over its G groups; the whole workgroup calls it, thread 0 gets the result.
// kLive: the histogram was written by atomics of THIS kernel — read it past the L1 with device-scope loads — and is left
// zeroed for the workgroup's next replicate.
template <bool kLive>
__device__ __forceinline__ void eval_groups(uint32_t *hist, uint32_t G, uint32_t *sh, unsigned long long *sh64, uint64_t out[3]) {
  const int tid = (int)threadIdx.x;
  unsigned long long *pairs = (unsigned long long *)hist;   // (c0, c1) of group g: the low and the high word of pairs[g]
  uint64_t u = 0, c1s = 0;
  uint32_t carry = 0;   // controls of the groups before this tile (< 2^31)
  for (uint32_t g0 = 0; g0 < G; g0 += kTile) {
    const uint32_t lo = g0 + (uint32_t)tid * kItems;
    uint32_t c0[kItems], c1[kItems], mine = 0;
#pragma unroll
    for (int k = 0; k < kItems; k++) {
      const uint32_t g = lo + k;
      unsigned long long w = 0;
      if (g < G) {
        if (kLive) {
          w = __hip_atomic_load(&pairs[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(&pairs[g], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          w = pairs[g];
        }
      }
      c0[k] = (uint32_t)w, c1[k] = (uint32_t)(w >> 32);
      mine += c0[k];
    }
    uint32_t total;
    uint64_t before = (uint64_t)carry + block_excl_scan(mine, sh, &total);
#pragma unroll
    for (int k = 0; k < kItems; k++) {
      u += auc::group_term(before, c0[k], c1[k]);
      before += c0[k];
      c1s += c1[k];
    }
    carry += total;
  }
  // sums of u and c1s over the workgroup (integers: any order)
  sh64[tid] = u, sh64[kThreads + tid] = c1s;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) sh64[tid] += sh64[tid + s], sh64[kThreads + tid] += sh64[kThreads + tid + s];
    __syncthreads();
  }
  if (tid == 0) out[0] = sh64[0], out[1] = sh64[kThreads], out[2] = carry;
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void k_auc_eval(uint32_t *__restrict__ hist, const uint32_t *__restrict__ ngroups, uint32_t n,
                                                       uint64_t *__restrict__ out) {
  __shared__ uint32_t sh[kThreads];
  __shared__ unsigned long long sh64[2 * kThreads];
  uint64_t r[3];
  eval_groups<false>(hist + (size_t)blockIdx.x * 2 * n, ngroups[blockIdx.x], sh, sh64, r);
  if (threadIdx.x == 0) out[3 * blockIdx.x] = r[0], out[3 * blockIdx.x + 1] = r[1], out[3 * blockIdx.x + 2] = r[2];
}

// replicates b0 .. b0 + nb - 1 of one column; scratch: gridDim.x histograms of 2 G counters, zero on entry and on exit
__global__ __launch_bounds__(kThreads) void k_auc_boot(const uint32_t *__restrict__ code, uint32_t n, uint32_t G, uint64_t seed,
                                                       uint32_t b0, uint32_t nb, uint32_t *__restrict__ scratch,
                                                       uint64_t *__restrict__ out) {
  __shared__ uint32_t sh[kThreads];
  __shared__ unsigned long long sh64[2 * kThreads];
  uint32_t *hist = scratch + (size_t)blockIdx.x * 2 * G;
  const uint32_t nq = (n + 3u) / 4u;
  for (uint32_t r = blockIdx.x; r < nb; r += gridDim.x) {
    const uint32_t b = b0 + r;
    for (uint32_t q = threadIdx.x; q < nq; q += kThreads) {
      const gibbs::Philox o = auc::draw_words(q, b, seed);
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (4u * q + k < n) atomicAdd(&hist[code[auc::row_of_word(o.v[k], n)]], 1u);
    }
    // every atomic of the workgroup has reached the L2 before any wave reads the histogram
    __threadfence();
    __syncthreads();
    uint64_t res[3];
    eval_groups<true>(hist, G, sh, sh64, res);
    if (threadIdx.x == 0) out[3 * (size_t)r] = res[0], out[3 * (size_t)r + 1] = res[1], out[3 * (size_t)r + 2] = res[2];
    // ... and every zero before the next replicate's atomics
    __threadfence();
    __syncthreads();
  }
}

__global__ void k_auc_draws(uint32_t n, uint32_t b, uint64_t seed, int32_t *__restrict__ rows) {
  const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
  if (t < n) rows[t] = (int32_t)auc::draw_row(t, b, seed, n);
}

__global__ void k_fill_nan(double *__restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) p[i] = __longlong_as_double(0x7ff8000000000000ll);
}

// ---- pcor -------------------------------------------------------------------------------------------------------------------
// sum of v over the workgroup in a fixed tree (thread 0 gets it); sh: kThreads doubles
__device__ __forceinline__ double block_sum(double v, double *sh) {
  const int tid = (int)threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// partial[(slab * K + col) * 32 + q] = sum over the slab's rows of Q[i, q] x[i, col]
template <class T>
__global__ __launch_bounds__(kThreads) void k_pcor_qtx(const T *__restrict__ x, int64_t ld, int64_t n, const double *__restrict__ Q, int p,
                                                       double *__restrict__ partial) {
  __shared__ double sh[kThreads];
  const int64_t lo = (int64_t)blockIdx.x * auc::kPcorSlabRows, hi = min(n, lo + auc::kPcorSlabRows);
  const T *xc = x + (int64_t)blockIdx.y * ld;
  double acc[32];
#pragma unroll
  for (int q = 0; q < 32; q++) acc[q] = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
    const double v = (double)xc[i];
#pragma unroll
    for (int q = 0; q < 32; q++)
      if (q < p) acc[q] += Q[i + (int64_t)q * n] * v;
  }
  double *dst = partial + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 32;
#pragma unroll
  for (int q = 0; q < 32; q++) {
    if (q < p) {
      const double s = block_sum(acc[q], sh);
      if (threadIdx.x == 0) dst[q] = s;
    }
  }
}

// out[col * width + q] = sum over the slabs, ascending, of partial[(slab * K + col) * width + q]
__global__ void k_pcor_sum(const double *__restrict__ partial, int64_t nslab, int64_t K, int width, int used, double *__restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= K * width) return;
  const int q = (int)(idx % width);
  double s = 0.0;
  if (q < used)
    for (int64_t sl = 0; sl < nslab; sl++) s += partial[(size_t)sl * K * width + idx];
  out[idx] = s;
}

// e = x - Q a; partial[(slab * K + col) * 2] = sum e^2, [.. + 1] = sum e r_y
template <class T>
__global__ __launch_bounds__(kThreads) void k_pcor_resid(const T *__restrict__ x, int64_t ld, int64_t n, const double *__restrict__ Q, int p,
                                                         const double *__restrict__ a, const double *__restrict__ ry,
                                                         double *__restrict__ partial) {
  __shared__ double sh[kThreads];
  __shared__ double sa[32];
  const int64_t lo = (int64_t)blockIdx.x * auc::kPcorSlabRows, hi = min(n, lo + auc::kPcorSlabRows);
  const T *xc = x + (int64_t)blockIdx.y * ld;
  if (threadIdx.x < 32) sa[threadIdx.x] = (int)threadIdx.x < p ? a[(size_t)blockIdx.y * 32 + threadIdx.x] : 0.0;
  __syncthreads();
  double ee = 0.0, er = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
    double e = (double)xc[i];
    for (int q = 0; q < p; q++) e -= Q[i + (int64_t)q * n] * sa[q];
    ee += e * e;
    er += e * ry[i];
  }
  double *dst = partial + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 2;
  const double s0 = block_sum(ee, sh), s1 = block_sum(er, sh);
  if (threadIdx.x == 0) dst[0] = s0, dst[1] = s1;
}

// ---- host side --------------------------------------------------------------------------------------------------------------
size_t free_bytes() {
  size_t free_b = 0, total_b = 0;
  BSN_HIP(hipMemGetInfo(&free_b, &total_b));
  return free_b + dev_cache_held();
}

struct Scores {
  const void *pred;
  int f32, on_device;
  int64_t ld, n_src, K;   // K result columns over K * nsum input columns of n_src rows
  int64_t nsum;           // members of one result column: input columns j, j + K, j + 2 K, ...
  size_t esize() const { return f32 ? 4 : 8; }
};

void check_scores(const Scores &s, const char *who) {
  if (!s.pred) fail("%s: no scores", who);
  if (s.K < 1 || s.nsum < 1) fail("%s: 'pred' should have at least one column.", who);
  if (s.n_src < 1) fail("%s: 'pred' should have at least one row.", who);
  if (s.n_src > auc::kMaxRows) fail("%s: 2^31 rows or more (the row indices are 32-bit)", who);
  if (s.ld < s.n_src) fail("%s: Incompatibility between dimensions (leading dimension).", who);
}

// the selected rows' classes; refuses a value other than 0 / 1 and a single class
void check_target(const uint8_t *target, int64_t n, const char *who, int64_t *n1_out) {
  if (!target) fail("%s: no target", who);
  int64_t n1 = 0;
  for (int64_t i = 0; i < n; i++) {
    if (target[i] > 1) fail("%s: 'target' should hold 0 and 1 only (row %lld holds %d).", who, (long long)i, (int)target[i]);
    n1 += target[i];
  }
  if (n1 == 0 || n1 == n) fail("%s: 'target' should hold both classes (it holds %lld cases and %lld controls).", who, (long long)n1,
                              (long long)(n - n1));
  *n1_out = n1;
}

// columns [j0, j0 + kb) of every member, on the device: the caller's own memory for a device matrix, a staged copy for a
// host matrix (member c of batch column j at column c * kb + j of the copy, leading dimension n_src)
const void *stage(const Scores &s, int64_t j0, int64_t kb, DevBuf<char> &buf, int64_t *ld, int64_t *sum_stride) {
  if (s.on_device) {
    *ld = s.ld, *sum_stride = s.K * s.ld;
    return (const char *)s.pred + (size_t)j0 * s.ld * s.esize();
  }
  const size_t w = (size_t)s.n_src * s.esize();
  buf.ensure(w * kb * s.nsum);
  for (int64_t c = 0; c < s.nsum; c++)
    BSN_HIP(hipMemcpy2D(buf.p + (size_t)c * kb * w, w, (const char *)s.pred + (size_t)(c * s.K + j0) * s.ld * s.esize(), (size_t)s.ld * s.esize(),
                        w, (size_t)kb, hipMemcpyHostToDevice));
  *ld = s.n_src, *sum_stride = kb * s.n_src;
  return buf.p;
}

// (twoU, n1, n0) of every result column into counts (3 K words).  keep_code / keep_groups: the codes 2 gid + y of every
// column (n x K) and its number of tie groups stay for the bootstrap.
void auc_columns(const Scores &s, const int64_t *ind_row, int64_t n, const uint8_t *target, const char *who, uint64_t *counts,
                 DevBuf<uint32_t> *keep_code, std::vector<uint32_t> *keep_groups) {
  check_scores(s, who);
  if (n < 1) fail("%s: no row selected", who);
  if (n > auc::kMaxRows) fail("%s: 2^31 rows or more (the row indices are 32-bit)", who);
  int64_t n1 = 0;
  check_target(target, n, who, &n1);
  std::vector<int32_t> rows;
  if (ind_row) {
    rows.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
      if (ind_row[i] < 0 || ind_row[i] >= s.n_src) fail("%s: 'ind_row' out of bounds (%lld of %lld rows).", who, (long long)ind_row[i], (long long)s.n_src);
      rows[(size_t)i] = (int32_t)ind_row[i];
    }
  } else if (n != s.n_src) {
    fail("%s: Incompatibility between dimensions.\n'pred' and 'target' should have the same length.", who);
  }
  const int64_t cap = batch_cap();
  require_gpu();
  for (double &v : g_last_ms) v = 0.0;

  hipStream_t st = nullptr;
  DevBuf<uint8_t> d_y;
  DevBuf<int32_t> d_rows;
  DevBuf<int> d_flag;
  BSN_HIP(hipMemcpy(d_y.ensure((size_t)n), target, (size_t)n, hipMemcpyHostToDevice));
  if (ind_row) BSN_HIP(hipMemcpy(d_rows.ensure((size_t)n), rows.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  if (keep_code) keep_code->ensure((size_t)n * s.K);
  if (keep_groups) keep_groups->assign((size_t)s.K, 0u);

  // one column's workspace: keys in + out (16 n), rows in + out (8 n), codes (4 n), histogram (8 n), the sort's own
  // temporary storage (about one more copy of keys and rows) and, for a host matrix, the staged members
  const double per_col = 48.0 * (double)n + (s.on_device ? 0.0 : (double)s.n_src * s.esize() * s.nsum);
  const double room = (double)free_bytes() - 256e6;
  int64_t kb_max = std::min<int64_t>({s.K, cap, (int64_t)(0xffffffffull / (uint64_t)n)});
  if (room < per_col) fail("%s: no room for one column's workspace (%.3f GB for it, %.3f GB free)", who, per_col / 1e9, std::max(room, 0.0) / 1e9);
  kb_max = std::max<int64_t>(1, std::min<int64_t>(kb_max, (int64_t)(room / per_col)));

  DevBuf<char> d_stage, d_tmp;
  DevBuf<uint64_t> d_keys, d_keys2, d_out;
  DevBuf<uint32_t> d_vals, d_vals2, d_code, d_hist, d_ng, d_off;
  std::vector<uint32_t> off((size_t)kb_max + 1), ng((size_t)kb_max);
  for (int64_t j = 0; j <= kb_max; j++) off[(size_t)j] = (uint32_t)(j * n);
  BSN_HIP(hipMemcpy(d_off.ensure(off.size()), off.data(), off.size() * 4, hipMemcpyHostToDevice));
  d_flag.ensure(1);
  EventMarks<4> ev;
  for (int64_t j0 = 0; j0 < s.K; j0 += kb_max) {
    const int64_t kb = std::min(kb_max, s.K - j0);
    const size_t cells = (size_t)kb * n;
    int64_t ld = 0, sum_stride = 0;
    const void *x = stage(s, j0, kb, d_stage, &ld, &sum_stride);
    d_keys.ensure(cells), d_keys2.ensure(cells), d_vals.ensure(cells), d_vals2.ensure(cells);
    uint32_t *code = keep_code ? keep_code->p + (size_t)j0 * n : d_code.ensure(cells);
    d_hist.ensure(2 * cells), d_ng.ensure((size_t)kb), d_out.ensure((size_t)3 * kb);
    const int none = INT_MAX;
    BSN_HIP(hipMemcpyAsync(d_flag.p, &none, 4, hipMemcpyHostToDevice, st));
    BSN_HIP(hipMemsetAsync(d_hist.p, 0, 2 * cells * 4, st));
    ev.mark(0, st);
    const dim3 grid(blocks_of(n, kThreads), (unsigned)kb);
    if (s.f32)
      hipLaunchKernelGGL(k_auc_keys<float>, grid, dim3(kThreads), 0, st, (const float *)x, ld, sum_stride, (int)s.nsum,
                         ind_row ? d_rows.p : nullptr, (uint32_t)n, (int)j0, d_keys.p, d_vals.p, d_flag.p);
    else
      hipLaunchKernelGGL(k_auc_keys<double>, grid, dim3(kThreads), 0, st, (const double *)x, ld, sum_stride, (int)s.nsum,
                         ind_row ? d_rows.p : nullptr, (uint32_t)n, (int)j0, d_keys.p, d_vals.p, d_flag.p);
    BSN_HIP(hipGetLastError());
    ev.mark(1, st);
    size_t tmp = 0;
    if (kb == 1) {
      BSN_HIP(rocprim::radix_sort_pairs(nullptr, tmp, d_keys.p, d_keys2.p, d_vals.p, d_vals2.p, (size_t)n, 0, 64, st));
      d_tmp.ensure(std::max<size_t>(tmp, 1));
      BSN_HIP(rocprim::radix_sort_pairs((void *)d_tmp.p, tmp, d_keys.p, d_keys2.p, d_vals.p, d_vals2.p, (size_t)n, 0, 64, st));
    } else {
      BSN_HIP(rocprim::segmented_radix_sort_pairs(nullptr, tmp, d_keys.p, d_keys2.p, d_vals.p, d_vals2.p, (unsigned)cells, (unsigned)kb,
                                                  d_off.p, d_off.p + 1, 0, 64, st));
      d_tmp.ensure(std::max<size_t>(tmp, 1));
      BSN_HIP(rocprim::segmented_radix_sort_pairs((void *)d_tmp.p, tmp, d_keys.p, d_keys2.p, d_vals.p, d_vals2.p, (unsigned)cells,
                                                  (unsigned)kb, d_off.p, d_off.p + 1, 0, 64, st));
    }
    ev.mark(2, st);
    hipLaunchKernelGGL(k_auc_groups, dim3((unsigned)kb), dim3(kThreads), 0, st, d_keys2.p, d_vals2.p, d_y.p, (uint32_t)n, code, d_hist.p,
                       d_ng.p);
    BSN_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_auc_eval, dim3((unsigned)kb), dim3(kThreads), 0, st, d_hist.p, d_ng.p, (uint32_t)n, d_out.p);
    BSN_HIP(hipGetLastError());
    ev.mark(3, st);
    int flag = 0;
    BSN_HIP(hipMemcpy(&flag, d_flag.p, 4, hipMemcpyDeviceToHost));   // (synchronises the null stream)
    if (flag != INT_MAX) fail("%s: missing value (NaN) in 'pred', first in column %d.", who, flag);
    BSN_HIP(hipMemcpy(counts + 3 * j0, d_out.p, (size_t)3 * kb * 8, hipMemcpyDeviceToHost));
    if (keep_groups) BSN_HIP(hipMemcpy(keep_groups->data() + j0, d_ng.p, (size_t)kb * 4, hipMemcpyDeviceToHost));
    g_last_ms[0] += ev.ms(0, 1), g_last_ms[1] += ev.ms(1, 2), g_last_ms[2] += ev.ms(2, 3);
  }
  for (int64_t j = 0; j < s.K; j++)
    if (counts[3 * j + 1] != (uint64_t)n1 || counts[3 * j + 2] != (uint64_t)(n - n1))
      fail("%s: internal error: the class counts of column %lld do not add up", who, (long long)j);
}

void auc_entry(const Scores &s, const int64_t *ind_row, int64_t n, const uint8_t *target, double *auc_out) {
  if (!auc_out) fail("AUC: no result buffer");
  std::vector<uint64_t> counts((size_t)3 * std::max<int64_t>(s.K, 1));
  auc_columns(s, ind_row, n, target, "AUC", counts.data(), nullptr, nullptr);
  for (int64_t j = 0; j < s.K; j++) auc_out[j] = auc::value(counts[3 * j], counts[3 * j + 1], counts[3 * j + 2]);
}

void boot_entry(const Scores &s, const uint8_t *target, int64_t nboot, uint64_t seed, double *rep_out) {
  const char *who = "AUCBoot";
  if (!rep_out) fail("%s: no result buffer", who);
  if (nboot < 1 || nboot > ((int64_t)1 << 31) - 1) fail("%s: 'nboot' should be between 1 and 2^31 - 1.", who);
  const int64_t n = s.n_src;
  std::vector<uint64_t> counts((size_t)3 * std::max<int64_t>(s.K, 1));
  DevBuf<uint32_t> d_code;
  std::vector<uint32_t> groups;
  auc_columns(s, nullptr, n, target, who, counts.data(), &d_code, &groups);

  hipStream_t st = nullptr;
  const int64_t cap = batch_cap();
  const uint32_t gmax = *std::max_element(groups.begin(), groups.end());
  const double per_group = 8.0 * (double)gmax, room = (double)free_bytes() - 256e6;
  if (room < per_group) fail("%s: no room for one replicate's histogram (%.3f GB for it, %.3f GB free)", who, per_group / 1e9, std::max(room, 0.0) / 1e9);
  const int64_t wg_max = std::max<int64_t>(1, std::min<int64_t>({(int64_t)kBootMaxGroups, nboot, cap, (int64_t)(room / per_group)}));
  // replicates of one launch: at most 2^32 draws, so that no launch occupies the device for long whatever nboot is
  const int64_t launch = std::min<int64_t>({nboot, cap, std::max<int64_t>(wg_max, kBootLaunchDraws / n)});
  DevBuf<uint32_t> d_scratch;
  DevBuf<uint64_t> d_out;
  d_scratch.ensure((size_t)wg_max * 2 * gmax);
  d_out.ensure((size_t)3 * launch);
  BSN_HIP(hipMemsetAsync(d_scratch.p, 0, (size_t)wg_max * 2 * gmax * 4, st));
  std::vector<uint64_t> out((size_t)3 * launch);
  EventMarks<2> ev;
  for (int64_t j = 0; j < s.K; j++)
    for (int64_t b0 = 0; b0 < nboot; b0 += launch) {
      const int64_t nb = std::min(launch, nboot - b0);
      ev.mark(0, st);
      hipLaunchKernelGGL(k_auc_boot, dim3((unsigned)std::min(wg_max, nb)), dim3(kThreads), 0, st, d_code.p + (size_t)j * n, (uint32_t)n,
                         groups[(size_t)j], seed, (uint32_t)b0, (uint32_t)nb, d_scratch.p, d_out.p);
      BSN_HIP(hipGetLastError());
      ev.mark(1, st);
      BSN_HIP(hipMemcpy(out.data(), d_out.p, (size_t)3 * nb * 8, hipMemcpyDeviceToHost));
      g_last_ms[3] += ev.ms(0, 1);
      for (int64_t r = 0; r < nb; r++) {
        if (out[3 * r + 1] + out[3 * r + 2] != (uint64_t)n) fail("%s: internal error: a replicate's draws do not add up", who);
        rep_out[(size_t)j * nboot + b0 + r] = auc::value(out[3 * r], out[3 * r + 1], out[3 * r + 2]);
      }
    }
}

void draws_entry(int64_t n, int64_t b, uint64_t seed, int32_t *rows_out) {
  if (n < 1 || n > auc::kMaxRows) fail("AUCBoot: the number of rows should be between 1 and 2^31 - 1.");
  if (b < 0 || b > ((int64_t)1 << 31) - 1) fail("AUCBoot: the replicate should be between 0 and 2^31 - 1.");
  if (!rows_out) fail("AUCBoot: no result buffer");
  require_gpu();
  DevBuf<int32_t> d_rows;
  d_rows.ensure((size_t)n);
  hipLaunchKernelGGL(k_auc_draws, dim3(blocks_of(n, kThreads)), dim3(kThreads), 0, nullptr, (uint32_t)n, (uint32_t)b, seed, d_rows.p);
  BSN_HIP(hipGetLastError());
  BSN_HIP(hipMemcpy(rows_out, d_rows.p, (size_t)n * 4, hipMemcpyDeviceToHost));
}

void pcor_entry(const Scores &s, const double *Q, int64_t p, const double *ry, double *ee_out, double *ery_out) {
  const char *who = "pcor";
  check_scores(s, who);
  if (!Q || !ry || !ee_out || !ery_out) fail("%s: no buffer", who);
  if (p < 1 || p > auc::kMaxCovar) fail("%s: [1, z] should have at most %d columns (got %lld).", who, auc::kMaxCovar, (long long)p);
  if (s.K > kMaxBatch) fail("%s: at most %lld columns per call.", who, (long long)kMaxBatch);
  const int64_t n = s.n_src, K = s.K, nslab = (n + auc::kPcorSlabRows - 1) / auc::kPcorSlabRows;
  require_gpu();
  for (double &v : g_last_ms) v = 0.0;
  const double bytes = (s.on_device ? 0.0 : (double)n * K * s.esize()) + (double)n * (p + 1) * 8 + (double)nslab * K * 34 * 8 + (double)K * 34 * 8;
  const double room = (double)free_bytes() - 256e6;
  if (room < bytes) fail("%s: no room for the workspace (%.3f GB for it, %.3f GB free)", who, bytes / 1e9, std::max(room, 0.0) / 1e9);
  hipStream_t st = nullptr;
  DevBuf<char> d_stage;
  DevBuf<double> d_Q, d_ry, d_part, d_a, d_res;
  int64_t ld = 0, unused = 0;
  const void *x = stage(s, 0, K, d_stage, &ld, &unused);
  BSN_HIP(hipMemcpy(d_Q.ensure((size_t)n * p), Q, (size_t)n * p * 8, hipMemcpyHostToDevice));
  BSN_HIP(hipMemcpy(d_ry.ensure((size_t)n), ry, (size_t)n * 8, hipMemcpyHostToDevice));
  d_part.ensure((size_t)nslab * K * 32), d_a.ensure((size_t)K * 32), d_res.ensure((size_t)K * 2);
  const dim3 grid((unsigned)nslab, (unsigned)K);
  EventMarks<2> ev;
  ev.mark(0, st);
  if (s.f32)
    hipLaunchKernelGGL(k_pcor_qtx<float>, grid, dim3(kThreads), 0, st, (const float *)x, ld, n, d_Q.p, (int)p, d_part.p);
  else
    hipLaunchKernelGGL(k_pcor_qtx<double>, grid, dim3(kThreads), 0, st, (const double *)x, ld, n, d_Q.p, (int)p, d_part.p);
  BSN_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_pcor_sum, dim3(blocks_of(K * 32, kThreads)), dim3(kThreads), 0, st, d_part.p, nslab, K, 32, (int)p, d_a.p);
  BSN_HIP(hipGetLastError());
  if (s.f32)
    hipLaunchKernelGGL(k_pcor_resid<float>, grid, dim3(kThreads), 0, st, (const float *)x, ld, n, d_Q.p, (int)p, d_a.p, d_ry.p, d_part.p);
  else
    hipLaunchKernelGGL(k_pcor_resid<double>, grid, dim3(kThreads), 0, st, (const double *)x, ld, n, d_Q.p, (int)p, d_a.p, d_ry.p, d_part.p);
  BSN_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_pcor_sum, dim3(blocks_of(K * 2, kThreads)), dim3(kThreads), 0, st, d_part.p, nslab, K, 2, 2, d_res.p);
  BSN_HIP(hipGetLastError());
  ev.mark(1, st);
  std::vector<double> res((size_t)K * 2);
  BSN_HIP(hipMemcpy(res.data(), d_res.p, (size_t)K * 16, hipMemcpyDeviceToHost));
  g_last_ms[4] = ev.ms(0, 1);
  for (int64_t j = 0; j < K; j++) ee_out[j] = res[(size_t)2 * j], ery_out[j] = res[(size_t)2 * j + 1];
}

// big_prodMat: what bsn_bed_prod_and_rowsumssq does without the row norms; the result stays on the device when asked
void prodmat(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const double *center, const double *scale,
             const double *A, int64_t K, double *XV, double *d_XV_out) {
  if (!bed) fail("big_prodMat: no handle");
  if (K <= 0) fail("'A.col' must have at least one column.");
  if (K > INT_MAX) fail("big_prodMat: too many columns.");
  if (!A || (!XV && !d_XV_out)) fail("big_prodMat: no buffer");
  // a NaN column of A (a grid point that diverged) is a NaN column of the result; the product itself sees zeros there
  // (A is copied only when such a column exists)
  std::vector<double> V;
  std::vector<char> bad((size_t)K, 0);
  bool any_bad = false;
  for (int64_t k = 0; k < K; k++) {
    const double *col = A + (size_t)k * m;
    int nan = 0;
    for (int64_t j = 0; j < m; j++) nan |= col[j] != col[j];
    bad[(size_t)k] = (char)nan;
    any_bad |= nan != 0;
  }
  if (any_bad) {
    V.assign(A, A + (size_t)m * K);
    for (int64_t k = 0; k < K; k++)
      if (bad[(size_t)k]) std::fill(V.begin() + (size_t)k * m, V.begin() + (size_t)(k + 1) * m, 0.0);
  }
  bsn_op op;
  fill_op(&op, bed, ind_row, n, ind_col, m, center, scale);
  op.slices = 7;
  DevBuf<double> d_V, d_own;
  copy_h2d(bed, d_V.ensure((size_t)m * K), any_bad ? V.data() : A, (size_t)m * K * 8);
  double *d_XV = d_XV_out ? d_XV_out : d_own.ensure((size_t)n * K);
  op_prod(&op, d_V.p, m, (int)K, d_XV, n);
  for (int64_t k = 0; k < K; k++)
    if (bad[(size_t)k] && n > 0) {
      hipLaunchKernelGGL(k_fill_nan, dim3(blocks_of(n, kThreads)), dim3(kThreads), 0, bed->stream, d_XV + (size_t)k * n, n);
      BSN_HIP(hipGetLastError());
    }
  if (XV) copy_d2h(bed, XV, d_XV, (size_t)n * K * 8);
  BSN_HIP(hipStreamSynchronize(bed->stream));
}

Scores scores_of(const void *pred, int32_t is_f32, int32_t on_device, int64_t ld, int64_t n_src, int64_t K, int64_t nsum) {
  Scores s{};
  s.pred = pred, s.f32 = is_f32 != 0, s.on_device = on_device != 0, s.ld = ld, s.n_src = n_src, s.K = K, s.nsum = nsum;
  return s;
}

}  // namespace
}  // namespace bsn

extern "C" {

int bsn_bed_prodmat(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const double *center,
                    const double *scale, const double *A, int64_t K, double *XV, double *d_XV) {
  return bsn::guarded([&] { bsn::prodmat(bed, ind_row, n, ind_col, m, center, scale, A, K, XV, d_XV); });
}

int bsn_auc(const void *pred, int32_t is_f32, int32_t on_device, int64_t ld, int64_t n_src, int64_t K, int64_t n_sum,
            const int64_t *ind_row, int64_t n, const uint8_t *target, double *auc_out) {
  return bsn::guarded([&] { bsn::auc_entry(bsn::scores_of(pred, is_f32, on_device, ld, n_src, K, n_sum), ind_row, n, target, auc_out); });
}

int bsn_auc_boot(const void *pred, int32_t is_f32, int32_t on_device, int64_t ld, int64_t n, int64_t K, const uint8_t *target,
                 int64_t nboot, uint64_t seed, double *replicates_out) {
  return bsn::guarded([&] { bsn::boot_entry(bsn::scores_of(pred, is_f32, on_device, ld, n, K, 1), target, nboot, seed, replicates_out); });
}

int bsn_auc_boot_draws(int64_t n, int64_t b, uint64_t seed, int32_t *rows_out) {
  return bsn::guarded([&] { bsn::draws_entry(n, b, seed, rows_out); });
}

int bsn_pcor_moments(const void *x, int32_t is_f32, int32_t on_device, int64_t ld, int64_t n, int64_t K, const double *Q, int64_t p,
                     const double *ry, double *ee_out, double *ery_out) {
  return bsn::guarded([&] { bsn::pcor_entry(bsn::scores_of(x, is_f32, on_device, ld, n, K, 1), Q, p, ry, ee_out, ery_out); });
}

int bsn_auc_last_ms(double *ms_out) {
  return bsn::guarded([&] {
    for (int k = 0; k < 5; k++) ms_out[k] = bsn::g_last_ms[k];
  });
}

}  // extern "C"
