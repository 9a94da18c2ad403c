// ldsplit.hip — snp_ldsplit (R/split-LD.R, src/split-LD.cpp of the reference) over the resident sparse LD matrix: the
// split of a chromosome into K = 1 .. max_K blocks that minimises the sum of r^2 outside the blocks (and, among equal
// sums, the sum of squared block sizes), by the reference's dynamic program.  DESIGN.md section 3.5e.
//
//   suffix sums   one thread per column walks the part below its diagonal from the end and writes the running sum l next
//                 to each stored entry (ldsplit_step.hpp: take_entry).  L(c, row) is then the value at the first stored
//                 entry of column c with index >= row (binary search), 0 when there is none.
//   E             one thread per last variant `col`: e += L(row, col + 1) for row = col, col - 1, ... in fp64, in that
//                 order; from the min_size-th term on every partial sum is kept as a float, E[t * m + col] being the block
//                 col - min_size + 1 - t .. col.  len[col] of them exist (the position window, max_cost and max_size stop
//                 the walk).
//   levels        level k, row r: the minimum, in the order of ldsplit_step.hpp (better), over t of
//                 (E[t, col] + C1(col + 1, k - 1), size^2 + C2(col + 1, k - 1)) with col = r + min_size - 1 + t.  One
//                 launch per level; a workgroup holds kRowTile rows, one per lane, and its kSplit waves share the t range
//                 (wave w takes t = w, w + kSplit, ...), so that for one t the lanes of a wave read neighbouring floats
//                 of E; the kSplit partial minima of a row meet in LDS.  The order is associative and commutative: the
//                 grouping changes no bit.  The host reads C1(0, k) after each level and decides the early stop.
//   epilogue      one thread per K follows best_ind from row 0 (all_last, the sum of squared sizes); the stored entries
//                 beyond their column's block are counted in integers, one thread per (column, K).
//
// Every loop has a trip count bounded by its arguments; no workgroup waits for another.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "bsn_internal.hpp"
#include "ldsplit_step.hpp"

namespace bsn {
namespace {

constexpr int kThreads = 256;   // threads per block of the per-column and per-K kernels
constexpr int kRowTile = 64;    // rows of a level per workgroup: one per lane of a wave
constexpr int kSplit = 8;       // waves of that workgroup: each takes every kSplit-th t of its rows

#pragma clang fp contract(off)

// the first position e in [a, b) with I[e] >= row (b when there is none); rows ascend within a column
__device__ __forceinline__ int64_t first_at_least(const int32_t *__restrict__ I, int64_t a, int64_t b, int64_t row) {
  while (a < b) {
    const int64_t mid = a + ((b - a) >> 1);
    if (I[mid] < row) a = mid + 1; else b = mid;
  }
  return a;
}

// where column c stores its diagonal: -1 when it does not, -2 when the stored value is 0
__global__ void k_diag(const int64_t *__restrict__ P, const int32_t *__restrict__ I, const double *__restrict__ X, int64_t m,
                       int64_t *__restrict__ diag) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m) return;
  const int64_t b = P[c + 1];
  const int64_t e = first_at_least(I, P[c], b, c);
  diag[c] = (e < b && I[e] == c) ? (X[e] == 0 ? -2 : e) : -1;
}

// S[e] = the running sum of column c once every stored entry below the diagonal from the last one up to e has been taken
__global__ void k_suffix(const int64_t *__restrict__ P, const double *__restrict__ X, const int64_t *__restrict__ diag, int64_t m,
                         double thr_r2, double max_r2, double *__restrict__ S) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m) return;
  const int64_t a = diag[c] + 1;
  double l = 0;
  for (int64_t e = P[c + 1] - 1; e >= a; e--) {
    l = ldsplit::take_entry(l, X[e], thr_r2, max_r2);
    S[e] = l;
  }
}

__global__ void k_E(const int64_t *__restrict__ P, const int32_t *__restrict__ I, const double *__restrict__ S,
                    const int64_t *__restrict__ diag, const double *__restrict__ pos, int64_t m, int32_t min_size,
                    int32_t max_size, double max_cost, float *__restrict__ E, int32_t *__restrict__ len) {
  const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= m) return;
  const double pos_min = (pos ? pos[col] : 0.0) - 1;
  double e = 0;
  int32_t count = 0, n = 0;
  for (int64_t row = col; row >= 0; row--) {   // at most max_size turns: every turn that does not leave adds 1 to count
    if ((pos ? pos[row] : 0.0) < pos_min) break;
    if (col + 1 < m) {   // L(., m) is 0
      const int64_t b = P[row + 1];
      const int64_t at = first_at_least(I, diag[row] + 1, b, col + 1);
      if (at < b) e = e + S[at];
    }
    if (e > max_cost) break;
    count++;
    if (count >= min_size) {
      E[(int64_t)(count - min_size) * m + col] = ldsplit::keep(e);
      n++;
      if (count == max_size) break;
    }
  }
  len[col] = n;
}

__global__ void k_fill(double *__restrict__ a, int64_t n, double v) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) a[k] = v;
}

// one block only: the rows m - max_size .. m - min_size whose position is within 1 of the last variant's.  Every row of
// the level is written (C1 and best_ind of the others keep +Inf and NA).
__global__ void k_level0(const double *__restrict__ pos, int64_t m, int32_t min_size, int32_t max_size, double *__restrict__ C1,
                         double *__restrict__ C2, int32_t *__restrict__ best) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= m) return;
  const int64_t size = m - row;
  const double pos_min = (pos ? pos[m - 1] : 0.0) - 1;
  // pos ascends: the reference's walk from size = min_size upwards leaves at the first row outside the window
  const bool in = size >= min_size && size <= max_size && !((pos ? pos[row] : 0.0) < pos_min);
  C2[row] = in ? (double)size * (double)size : ldsplit::inf();
  if (in) {
    C1[row] = 0;
    best[row] = (int32_t)m;
  }
}

__global__ __launch_bounds__(kRowTile * kSplit) void k_level(const float *__restrict__ E, const int32_t *__restrict__ len,
                                                             const double *__restrict__ C1p, const double *__restrict__ C2p,
                                                             int64_t m, int32_t min_size, int32_t W, double *__restrict__ C1,
                                                             double *__restrict__ C2, int32_t *__restrict__ best) {
  __shared__ double s1[kSplit][kRowTile], s2[kSplit][kRowTile];
  __shared__ int32_t sc[kSplit][kRowTile];
  const int lane = threadIdx.x % kRowTile, wave = threadIdx.x / kRowTile;
  const int64_t row = (int64_t)blockIdx.x * kRowTile + lane;
  ldsplit::Cand b = ldsplit::none();
  if (row < m) {
    const int64_t left = m - row - min_size + 1;   // col < m
    const int32_t t_end = left < W ? (int32_t)(left < 0 ? 0 : left) : W;
    for (int32_t t = wave; t < t_end; t += kSplit) {
      const int64_t col = row + min_size - 1 + t;
      if (t < len[col]) {
        const bool last = col + 1 == m;   // C(m, .) = +Inf: a block that ends at the last variant exists at level 0 only
        const ldsplit::Cand c = ldsplit::candidate(E[(int64_t)t * m + col], last ? ldsplit::inf() : C1p[col + 1],
                                                   last ? ldsplit::inf() : C2p[col + 1], (int32_t)row, (int32_t)col);
        if (ldsplit::better(c, b)) b = c;
      }
    }
  }
  s1[wave][lane] = b.c1;
  s2[wave][lane] = b.c2;
  sc[wave][lane] = b.col;
  __syncthreads();
  if (wave == 0 && row < m) {
    for (int w = 1; w < kSplit; w++) {
      const ldsplit::Cand c = {s1[w][lane], s2[w][lane], sc[w][lane]};
      if (ldsplit::better(c, b)) b = c;
    }
    C1[row] = b.c1;
    C2[row] = b.c2;
    best[row] = b.col < 0 ? -1 : b.col + 1;
  }
}

// thread kk: K = kk + 1 blocks.  all_last [max_K x max_K], row kk: the first row of the next block after each of the K
// blocks (the reference's 1-based last index), the rest -1; cost2 = the sum of squared sizes (+Inf when not reported)
__global__ void k_paths(const double *__restrict__ C1, const int32_t *__restrict__ best, int64_t m, int32_t max_K, int32_t levels,
                        double max_cost, double *__restrict__ cost, double *__restrict__ cost2, int32_t *__restrict__ ok,
                        int32_t *__restrict__ all_last) {
  const int32_t kk = blockIdx.x * blockDim.x + threadIdx.x;
  if (kk >= max_K) return;
  int32_t *mine = all_last + (int64_t)kk * max_K;
  for (int32_t b = 0; b < max_K; b++) mine[b] = -1;
  const double c = C1[(int64_t)kk * m];
  cost[kk] = c;
  bool good = kk < levels && ldsplit::reported(c, best[(int64_t)kk * m], max_cost);
  double sq = 0;
  if (good) {
    int64_t j = 0;
    for (int32_t k = kk; k >= 0; k--) {
      const int64_t nj = best[j + (int64_t)k * m];
      if (nj <= j || nj > m || (k > 0 && nj == m)) {   // cannot happen on a table the levels wrote; keeps the walk inside it
        good = false;
        break;
      }
      mine[kk - k] = (int32_t)nj;
      const double size = (double)(nj - j);
      sq = sq + size * size;
      j = nj;
    }
  }
  if (!good)
    for (int32_t b = 0; b <= kk; b++) mine[b] = -1;
  ok[kk] = good ? 1 : 0;
  cost2[kk] = good ? sq : ldsplit::inf();
}

#pragma clang fp contract(on)

// kk = k0 + blockIdx.y; one thread per column j: the stored entries below the diagonal whose row lies beyond j's block
__global__ __launch_bounds__(kThreads) void k_outside(const int64_t *__restrict__ P, const int32_t *__restrict__ I,
                                                      const int64_t *__restrict__ diag, int64_t m, int32_t max_K,
                                                      int32_t k0, const int32_t *__restrict__ ok, const int32_t *__restrict__ all_last,
                                                      unsigned long long *__restrict__ outside) {
  const int32_t kk = k0 + (int32_t)blockIdx.y;
  if (!ok[kk]) return;
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  unsigned long long n = 0;
  if (j < m) {
    const int32_t *mine = all_last + (int64_t)kk * max_K;
    int32_t a = 0, b = kk + 1;   // the first block end > j (the last one is m)
    while (a < b) {
      const int32_t mid = a + ((b - a) >> 1);
      if (mine[mid] <= j) a = mid + 1; else b = mid;
    }
    const int64_t limit = a <= kk ? mine[a] : m;
    const int64_t e1 = P[j + 1];
    n = (unsigned long long)(e1 - first_at_least(I, diag[j] + 1, e1, limit));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(outside + kk, n);
}

unsigned blocks_for(int64_t n, int per) { return (unsigned)std::max<int64_t>((n + per - 1) / per, 1); }

}  // namespace
}  // namespace bsn

using namespace bsn;

extern "C" {

int bsn_sfbm_ldsplit(const bsn_sfbm *s, double thr_r2, double max_r2, int32_t min_size, int32_t max_size, int32_t max_K,
                     double max_cost, const double *pos_scaled, double *C_out, int32_t *best_ind_out, double *cost_out,
                     double *cost2_out, double *perc_kept_out, int32_t *n_block_ok_out, int32_t *all_last_out,
                     int32_t *levels_run_out, double *seconds_out) {
  return guarded([&] {
    if (!s) fail("bsn_sfbm_ldsplit: NULL 'corr'");
    const int64_t m = s->m2;
    if (m < 1) fail("snp_ldsplit: 'corr' has no column.");
    if (min_size < 1) fail("snp_ldsplit: 'min_size' must be at least 1 (got %d).", (int)min_size);
    if (max_size < min_size) fail("snp_ldsplit: 'max_size' (%d) must be at least 'min_size' (%d).", (int)max_size, (int)min_size);
    if (max_size > m) fail("snp_ldsplit: 'max_size' (%d) must be at most ncol(corr) = %lld.", (int)max_size, (long long)m);
    if (max_K < 1) fail("snp_ldsplit: 'max_K' must be at least 1 (got %d).", (int)max_K);
    if (std::isnan(thr_r2) || std::isnan(max_r2) || std::isnan(max_cost)) fail("snp_ldsplit: 'thr_r2', 'max_r2' and 'max_cost' must not be NaN.");
    if (pos_scaled)
      for (int64_t j = 0; j + 1 < m; j++)
        if (!(pos_scaled[j + 1] >= pos_scaled[j]))
          fail("snp_ldsplit: 'pos_scaled' must be ascending (positions %lld and %lld).", (long long)j, (long long)j + 1);
    if (pos_scaled && std::isnan(pos_scaled[0])) fail("snp_ldsplit: 'pos_scaled' must be ascending (position 0 is NaN).");
    require_gpu();

    // the diagonal of every column: stored and not 0 (the first kernel; nothing of the recurrence is allocated yet)
    DevBuf<int64_t> d_diag;
    std::vector<int64_t> diag((size_t)m);
    k_diag<<<blocks_for(m, kThreads), kThreads>>>(s->p.p, s->i.p, s->x.p, m, d_diag.ensure((size_t)m));
    BSN_HIP(hipGetLastError());
    BSN_HIP(hipMemcpy(diag.data(), d_diag.p, (size_t)m * 8, hipMemcpyDeviceToHost));
    int64_t nnz_lower = 0;
    for (int64_t c = 0; c < m; c++) {
      if (diag[(size_t)c] == -1) fail("snp_ldsplit: 'corr' must store its diagonal: column %lld has none.", (long long)c);
      if (diag[(size_t)c] == -2) fail("snp_ldsplit: the diagonal of 'corr' must not be 0: column %lld.", (long long)c);
      nnz_lower += s->hp[(size_t)c + 1] - diag[(size_t)c];
    }

    const int64_t W = (int64_t)max_size - min_size + 1;
    const double need = 4.0 * m * W + 8.0 * m * max_K + 4.0 * m * max_K + 16.0 * m + 8.0 * (double)s->nnz + 4.0 * m + 8.0 * m +
                        4.0 * max_K * (double)max_K + 64.0 * max_K;
    size_t free_b = 0, total_b = 0;
    BSN_HIP(hipMemGetInfo(&free_b, &total_b));
    const double have = (double)free_b + (double)dev_cache_held();
    if (need > 0.95 * have)
      fail("snp_ldsplit: the tables (E: %.0f B, C: %.0f B, best_ind: %.0f B, suffix sums: %.0f B) do not fit the free device "
           "memory (%.0f B).", 4.0 * m * W, 8.0 * m * max_K, 4.0 * m * max_K, 8.0 * (double)s->nnz, have);

    DevBuf<double> d_S, d_pos, d_C1, d_C2, d_cost, d_cost2;
    DevBuf<float> d_E;
    DevBuf<int32_t> d_len, d_best, d_ok, d_last;
    DevBuf<unsigned long long> d_out;
    d_S.ensure((size_t)std::max<int64_t>(s->nnz, 1));
    d_E.ensure((size_t)(m * W));
    d_len.ensure((size_t)m);
    d_C1.ensure((size_t)(m * max_K));
    d_C2.ensure((size_t)(2 * m));
    d_best.ensure((size_t)(m * max_K));
    d_cost.ensure((size_t)max_K);
    d_cost2.ensure((size_t)max_K);
    d_ok.ensure((size_t)max_K);
    d_last.ensure((size_t)max_K * (size_t)max_K);
    d_out.ensure((size_t)max_K);
    if (pos_scaled) BSN_HIP(hipMemcpy(d_pos.ensure((size_t)m), pos_scaled, (size_t)m * 8, hipMemcpyHostToDevice));
    const double *pos = pos_scaled ? d_pos.p : nullptr;

    EventMarks<4> ev;
    ev.mark(0, nullptr);
    k_suffix<<<blocks_for(m, kThreads), kThreads>>>(s->p.p, s->x.p, d_diag.p, m, thr_r2, max_r2, d_S.p);
    BSN_HIP(hipGetLastError());
    k_E<<<blocks_for(m, kThreads), kThreads>>>(s->p.p, s->i.p, d_S.p, d_diag.p, pos, m, min_size, max_size, max_cost, d_E.p,
                                               d_len.p);
    BSN_HIP(hipGetLastError());
    ev.mark(1, nullptr);

    k_fill<<<blocks_for(m * max_K, kThreads), kThreads>>>(d_C1.p, m * max_K, std::numeric_limits<double>::infinity());
    BSN_HIP(hipGetLastError());
    BSN_HIP(hipMemsetAsync(d_best.p, 0xff, (size_t)(m * max_K) * 4, nullptr));   // -1: NA
    k_level0<<<blocks_for(m, kThreads), kThreads>>>(pos, m, min_size, max_size, d_C1.p, d_C2.p, d_best.p);
    BSN_HIP(hipGetLastError());
    int32_t levels = max_K;
    double c_prev = 0;
    if (max_K > 1) BSN_HIP(hipMemcpy(&c_prev, d_C1.p, 8, hipMemcpyDeviceToHost));
    for (int32_t k = 1; k < max_K; k++) {
      k_level<<<blocks_for(m, kRowTile), kRowTile * kSplit>>>(d_E.p, d_len.p, d_C1.p + (int64_t)(k - 1) * m,
                                                              d_C2.p + (int64_t)((k - 1) & 1) * m, m, min_size, (int32_t)W,
                                                              d_C1.p + (int64_t)k * m, d_C2.p + (int64_t)(k & 1) * m,
                                                              d_best.p + (int64_t)k * m);
      BSN_HIP(hipGetLastError());
      double c_k = 0;
      BSN_HIP(hipMemcpy(&c_k, d_C1.p + (int64_t)k * m, 8, hipMemcpyDeviceToHost));
      if (ldsplit::stop_after(c_k, c_prev, max_cost)) {
        levels = k + 1;
        break;
      }
      c_prev = c_k;
    }
    ev.mark(2, nullptr);

    BSN_HIP(hipMemsetAsync(d_out.p, 0, (size_t)max_K * 8, nullptr));
    k_paths<<<blocks_for(max_K, kThreads), kThreads>>>(d_C1.p, d_best.p, m, max_K, levels, max_cost, d_cost.p, d_cost2.p, d_ok.p,
                                                       d_last.p);
    BSN_HIP(hipGetLastError());
    if (perc_kept_out) {
      // the grid's y extent holds 65 535 at the most
      for (int32_t k0 = 0; k0 < max_K; k0 += 32768) {
        const int32_t nk = std::min<int32_t>(32768, max_K - k0);
        k_outside<<<dim3(blocks_for(m, kThreads), (unsigned)nk), kThreads>>>(s->p.p, s->i.p, d_diag.p, m, max_K, k0, d_ok.p,
                                                                             d_last.p, d_out.p);
        BSN_HIP(hipGetLastError());
      }
    }
    ev.mark(3, nullptr);
    BSN_HIP(hipEventSynchronize(ev.e[3]));

    std::vector<int32_t> ok((size_t)max_K);
    BSN_HIP(hipMemcpy(ok.data(), d_ok.p, (size_t)max_K * 4, hipMemcpyDeviceToHost));
    if (C_out) BSN_HIP(hipMemcpy(C_out, d_C1.p, (size_t)(m * max_K) * 8, hipMemcpyDeviceToHost));
    if (best_ind_out) BSN_HIP(hipMemcpy(best_ind_out, d_best.p, (size_t)(m * max_K) * 4, hipMemcpyDeviceToHost));
    if (cost_out) BSN_HIP(hipMemcpy(cost_out, d_cost.p, (size_t)max_K * 8, hipMemcpyDeviceToHost));
    if (cost2_out) BSN_HIP(hipMemcpy(cost2_out, d_cost2.p, (size_t)max_K * 8, hipMemcpyDeviceToHost));
    if (all_last_out) BSN_HIP(hipMemcpy(all_last_out, d_last.p, (size_t)max_K * (size_t)max_K * 4, hipMemcpyDeviceToHost));
    if (n_block_ok_out) std::copy(ok.begin(), ok.end(), n_block_ok_out);
    if (perc_kept_out) {
      std::vector<unsigned long long> out((size_t)max_K);
      BSN_HIP(hipMemcpy(out.data(), d_out.p, (size_t)max_K * 8, hipMemcpyDeviceToHost));
      const double count_all = 2.0 * (double)nnz_lower - (double)m;   // the diagonal once
      for (int32_t kk = 0; kk < max_K; kk++)
        perc_kept_out[kk] = ok[(size_t)kk] ? (count_all - 2.0 * (double)out[(size_t)kk]) / count_all : -1.0;
    }
    if (levels_run_out) *levels_run_out = levels;
    if (seconds_out)
      for (int q = 0; q < 3; q++) seconds_out[q] = ev.ms(q, q + 1) * 1e-3;
  });
}

}  // extern "C"
