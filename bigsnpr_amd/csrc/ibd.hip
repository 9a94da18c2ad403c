// ibd.hip — bed_ibd / bed_ibdQC: the method-of-moments IBD table of every pair of samples, on the device (bsn_bed_ibd,
// bsn_ibd_fetch, bsn_ibd_free, bsn_ibd_last_ms).
//
// Replaces the PLINK 1.9 run of snp_plinkIBDQC (R/external-software.R of the reference: --genome in a child process).  The
// IBS0 / IBS1 / IBS2 counts of a pair follow from the five counts k_king_pairs leaves in its stash (IBS0; HET1HOM2 +
// HET2HOM1; the rest of NSNP), so the pair kernel, its operand, its batches and its two-product path are bed_king's,
// through the shared walk (king_walk.hpp).  New here:
//
//     k_ibd_moments   the five allele-frequency terms of every variant from the counts of the frequency samples, summed per
//                     leaf of 256 variants in ascending order
//     k_ibd_means     the leaves summed in ascending order, divided by the number of used variants
//     k_ibd_count     rows of the table per (sample i, column tile b), the estimate evaluated from the stash's integers
//     k_ibd_write     every segment writes its rows behind its offset (k_king_scan gives the offsets)
// The statement (terms, order of the sums, estimate, filter) is ibd_step.hpp, shared with the CPU statement.  No float
// atomics, no order that depends on the schedule: two calls return the same bytes.  DESIGN.md 3.5p.
#include <algorithm>
#include <memory>
#include <vector>

#include "bsn_internal.hpp"
#include "ibd_step.hpp"
#include "king_walk.hpp"

struct bsn_ibd {
  bsn_bed *bed = nullptr;   // the handle whose staging buffers serve the download
  int64_t count = 0, cap = 0;
  int64_t n_used = 0;
  double E[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  std::unique_ptr<bsn::DevBuf<int32_t>> d_i1, d_i2, d_ibs;   // count, count, 3 x count (row k at 3 k)
  std::unique_ptr<bsn::DevBuf<double>> d_est;                // 5 x count (row k at 5 k: Z0, Z1, Z2, PI_HAT, DST)
};

namespace bsn {
namespace {

using namespace kingwalk;

constexpr double kRowBytes = 60.0;   // I1, I2, three counts, five doubles

// device milliseconds of the last call of this process (bsn_ibd_last_ms): the operand, the per-sample totals of the
// complete-data path, the pair kernel, the compaction (as bsn_king_last_ms), then the counting pass of the frequency
// samples and the moment kernels
double g_last_ms[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

// One workgroup per leaf, one thread per variant: the terms go to LDS, threads 0 .. 4 add one term each over the leaf in
// ascending order (an unused variant adds 0), thread 5 counts the used variants.  table[4 j + c]: the count of code c.
__global__ __launch_bounds__(ibd::kLeaf) void k_ibd_moments(const int32_t *__restrict__ table, int64_t m, double *__restrict__ leaf_sum,
                                                            int32_t *__restrict__ leaf_used) {
  __shared__ double s_a[5][ibd::kLeaf];
  __shared__ int32_t s_used[ibd::kLeaf];
  const int tid = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * ibd::kLeaf + tid;
  double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  bool used = false;
  if (j < m) {
    const int4 c = *(const int4 *)(table + 4 * j);
    used = ibd::terms(c.x, c.y, c.z, a);
  }
#pragma unroll
  for (int k = 0; k < 5; k++) s_a[k][tid] = a[k];
  s_used[tid] = used ? 1 : 0;
  __syncthreads();
  if (tid < 5) {
    double sum = 0.0;
    for (int v = 0; v < ibd::kLeaf; v++) sum += s_a[tid][v];
    leaf_sum[5 * (int64_t)blockIdx.x + tid] = sum;
  } else if (tid == 5) {
    int32_t u = 0;
    for (int v = 0; v < ibd::kLeaf; v++) u += s_used[v];
    leaf_used[blockIdx.x] = u;
  }
}

// out[0 .. 4] = E, out[5] = n_used (as a double: exact below 2^53).  One workgroup; threads 0 .. 4 add one term each over
// the leaves in ascending order.
__global__ __launch_bounds__(64) void k_ibd_means(const double *__restrict__ leaf_sum, const int32_t *__restrict__ leaf_used,
                                                  int64_t nleaf, double *__restrict__ out) {
  __shared__ double s_sum[5];
  __shared__ int64_t s_n;
  const int tid = threadIdx.x;
  if (tid < 5) {
    double sum = 0.0;
    for (int64_t l = 0; l < nleaf; l++) sum += leaf_sum[5 * l + tid];
    s_sum[tid] = sum;
  } else if (tid == 5) {
    int64_t u = 0;
    for (int64_t l = 0; l < nleaf; l++) u += leaf_used[l];
    s_n = u;
  }
  __syncthreads();
  if (tid == 0) {
    const double sum[5] = {s_sum[0], s_sum[1], s_sum[2], s_sum[3], s_sum[4]};
    const ibd::Moments E = ibd::means(sum, s_n);
    out[0] = E.e00;
    out[1] = E.e01;
    out[2] = E.e02;
    out[3] = E.e11;
    out[4] = E.e12;
    out[5] = (double)s_n;
  }
}

struct Ibs {
  int32_t ibs0, ibs1, ibs2;
};
__device__ __forceinline__ Ibs ibs_of(const int32_t *__restrict__ st_cnt, size_t slot, int e) {
  const int32_t *c = st_cnt + slot * kStashCnt + e;
  Ibs s;
  s.ibs0 = c[2 * KT * KT];
  s.ibs1 = c[3 * KT * KT] + c[4 * KT * KT];
  s.ibs2 = c[0] - s.ibs0 - s.ibs1;
  return s;
}

// is the lane's pair of the segment (king_walk.hpp) a row of the table?  The estimate comes back for the writer.
__device__ __forceinline__ bool seg_row(const Batch &B, const ibd::Moments &E, const int32_t *__restrict__ st_cnt, int64_t seg, int lane,
                                        int64_t &i, int64_t &j, Ibs &s, ibd::Estimate &est) {
  size_t slot;
  int e;
  if (!seg_pair(B, seg, lane, i, j, slot, e)) return false;
  s = ibs_of(st_cnt, slot, e);
  est = ibd::estimate(s.ibs0, s.ibs1, s.ibs2, E);
  return !B.filter || ibd::passes(est.pi_hat, B.thr);
}

__global__ __launch_bounds__(256) void k_ibd_count(Batch B, ibd::Moments E, const int32_t *__restrict__ st_cnt, int64_t nseg,
                                                   int32_t *__restrict__ cnt) {
  const int64_t seg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const int lane = threadIdx.x & 63;
  int64_t i, j;
  Ibs s;
  ibd::Estimate est;
  const bool keep = seg_row(B, E, st_cnt, seg, lane, i, j, s, est);
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) cnt[seg] = __popcll(bal);
}

__global__ __launch_bounds__(256) void k_ibd_write(Batch B, ibd::Moments E, const int32_t *__restrict__ st_cnt, int64_t nseg,
                                                   const int64_t *__restrict__ off, int64_t base, int32_t *__restrict__ i1,
                                                   int32_t *__restrict__ i2, int32_t *__restrict__ ibs, double *__restrict__ est_out) {
  const int64_t seg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const int lane = threadIdx.x & 63;
  int64_t i, j;
  Ibs s;
  ibd::Estimate est;
  const bool keep = seg_row(B, E, st_cnt, seg, lane, i, j, s, est);
  const unsigned long long bal = __ballot(keep);
  if (!keep) return;
  const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
  const int64_t k = base + off[seg] + rank;
  i1[k] = (int32_t)i;
  i2[k] = (int32_t)j;
  ibs[3 * k] = s.ibs0;
  ibs[3 * k + 1] = s.ibs1;
  ibs[3 * k + 2] = s.ibs2;
  est_out[5 * k] = est.z0;
  est_out[5 * k + 1] = est.z1;
  est_out[5 * k + 2] = est.z2;
  est_out[5 * k + 3] = est.pi_hat;
  est_out[5 * k + 4] = est.dst;
}

// the rows of bed_ibd's table
struct IbdSink final : PairSink {
  bsn_ibd *K;
  ibd::Moments E;
  IbdSink(bsn_ibd *k, const ibd::Moments &e) : K(k), E(e) {}
  void reserve(int64_t need, int64_t keep, hipStream_t st) override {
    if (need <= K->cap) return;
    const int64_t cap = std::max<int64_t>(std::max<int64_t>(need, 2 * K->cap), 1 << 16);
    const double bytes = kRowBytes * (double)cap;
    size_t free_b = 0, total_b = 0;
    BSN_HIP(hipMemGetInfo(&free_b, &total_b));
    if ((double)(free_b + dev_cache_held()) < bytes + 256e6)
      fail("bed_ibd: a table of %lld rows does not fit in device memory (%.1f GB for it, %.1f GB free); raise 'pi.hat' or "
           "select fewer samples",
           (long long)need, bytes / 1e9, (double)free_b / 1e9);
    auto n_i1 = std::make_unique<DevBuf<int32_t>>(), n_i2 = std::make_unique<DevBuf<int32_t>>(), n_ibs = std::make_unique<DevBuf<int32_t>>();
    auto n_est = std::make_unique<DevBuf<double>>();
    n_i1->ensure((size_t)cap);
    n_i2->ensure((size_t)cap);
    n_ibs->ensure((size_t)3 * cap);
    n_est->ensure((size_t)5 * cap);
    if (keep > 0) {
      BSN_HIP(hipMemcpyAsync(n_i1->p, K->d_i1->p, (size_t)keep * 4, hipMemcpyDeviceToDevice, st));
      BSN_HIP(hipMemcpyAsync(n_i2->p, K->d_i2->p, (size_t)keep * 4, hipMemcpyDeviceToDevice, st));
      BSN_HIP(hipMemcpyAsync(n_ibs->p, K->d_ibs->p, (size_t)keep * 12, hipMemcpyDeviceToDevice, st));
      BSN_HIP(hipMemcpyAsync(n_est->p, K->d_est->p, (size_t)keep * 40, hipMemcpyDeviceToDevice, st));
      BSN_HIP(hipStreamSynchronize(st));
    }
    K->d_i1 = std::move(n_i1);
    K->d_i2 = std::move(n_i2);
    K->d_ibs = std::move(n_ibs);
    K->d_est = std::move(n_est);
    K->cap = cap;
  }
  void count(const Batch &B, const int32_t *st_cnt, const double *, int64_t nseg, int32_t *cnt, hipStream_t st) override {
    hipLaunchKernelGGL(k_ibd_count, dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, st, B, E, st_cnt, nseg, cnt);
    BSN_HIP(hipGetLastError());
  }
  void write(const Batch &B, const int32_t *st_cnt, const double *, int64_t nseg, const int64_t *off, int64_t base,
             hipStream_t st) override {
    hipLaunchKernelGGL(k_ibd_write, dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, st, B, E, st_cnt, nseg, off, base, K->d_i1->p,
                       K->d_i2->p, K->d_ibs->p, K->d_est->p);
    BSN_HIP(hipGetLastError());
  }
};

void bed_ibd(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const uint8_t *freq_mask,
             double min_pi_hat, int filter, int64_t *count_out, bsn_ibd **out) {
  if (!bed || !count_out || !out) fail("bed_ibd: null argument");
  pairs_check(bed, n, m, "bed_ibd");
  if (!(min_pi_hat >= 0.0 && min_pi_hat <= 1.0)) fail("bed_ibd: 'pi.hat' should be in range [0, 1] (got %g).", min_pi_hat);
  std::vector<int32_t> group((size_t)n, 0);
  int64_t n_freq = n;
  if (freq_mask) {
    n_freq = 0;
    for (int64_t i = 0; i < n; i++) {
      group[(size_t)i] = freq_mask[i] ? 0 : -1;
      n_freq += freq_mask[i] ? 1 : 0;
    }
  }
  if (n_freq == 0) fail("bed_ibd: the frequency mask selects no sample (no founder among 'ind.row'?)");
  for (double &v : g_last_ms) v = 0.0;

  // ---- the moments: the counts of the frequency samples (the grouped counting pass, one group), the terms, their means
  BSN_HIP(hipSetDevice(bed->device));
  hipStream_t st = bed->stream;
  DevBuf<int32_t> d_table, d_leaf_used;
  DevBuf<double> d_leaf_sum, d_E;
  double ms3[3] = {0.0, 0.0, 0.0};
  group_counts_device(bed, ind_row, n, group.data(), 1, ind_col, m, d_table, ms3);
  g_last_ms[4] = ms3[0] + ms3[1] + ms3[2];
  const int64_t nleaf = (m + ibd::kLeaf - 1) / ibd::kLeaf;
  d_leaf_sum.ensure((size_t)5 * nleaf);
  d_leaf_used.ensure((size_t)nleaf);
  d_E.ensure(6);
  EventMarks<2> ev;
  ev.mark(0, st);
  hipLaunchKernelGGL(k_ibd_moments, dim3((unsigned)nleaf), dim3(ibd::kLeaf), 0, st, d_table.p, m, d_leaf_sum.p, d_leaf_used.p);
  BSN_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_ibd_means, dim3(1), dim3(64), 0, st, d_leaf_sum.p, d_leaf_used.p, nleaf, d_E.p);
  BSN_HIP(hipGetLastError());
  ev.mark(1, st);
  double e6[6];
  copy_d2h(bed, e6, d_E.p, sizeof(e6));
  BSN_HIP(hipStreamSynchronize(st));
  g_last_ms[5] = ev.ms(0, 1);
  if (e6[5] == 0.0) fail("bed_ibd: no variant with both alleles and more than 3 called alleles among the founders");

  std::unique_ptr<bsn_ibd> K(new bsn_ibd());
  K->bed = bed;
  K->n_used = (int64_t)e6[5];
  for (int k = 0; k < 5; k++) K->E[k] = e6[k];
  K->d_i1 = std::make_unique<DevBuf<int32_t>>();
  K->d_i2 = std::make_unique<DevBuf<int32_t>>();
  K->d_ibs = std::make_unique<DevBuf<int32_t>>();
  K->d_est = std::make_unique<DevBuf<double>>();
  const ibd::Moments E = {e6[0], e6[1], e6[2], e6[3], e6[4]};
  IbdSink sink(K.get(), E);
  double ms[4] = {0.0, 0.0, 0.0, 0.0};
  K->count = pairs_walk(bed, ind_row, n, ind_col, m, min_pi_hat, filter, "bed_ibd", sink, ms);
  for (int q = 0; q < 4; q++) g_last_ms[q] = ms[q];
  *count_out = K->count;
  *out = K.release();
}

}  // namespace
}  // namespace bsn

extern "C" {

int bsn_bed_ibd(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const uint8_t *freq_mask,
                double min_pi_hat, int filter, int64_t *count, bsn_ibd **out) {
  return bsn::guarded([&] { bsn::bed_ibd(bed, ind_row, n, ind_col, m, freq_mask, min_pi_hat, filter, count, out); });
}

int bsn_ibd_fetch(bsn_ibd *k, int32_t *i1, int32_t *i2, int32_t *ibs, double *est, double *E, int64_t *n_used) {
  return bsn::guarded([&] {
    if (E)
      for (int q = 0; q < 5; q++) E[q] = k->E[q];
    if (n_used) *n_used = k->n_used;
    if (k->count <= 0) return;
    BSN_HIP(hipSetDevice(k->bed->device));
    bsn::copy_d2h(k->bed, i1, k->d_i1->p, (size_t)k->count * 4);
    bsn::copy_d2h(k->bed, i2, k->d_i2->p, (size_t)k->count * 4);
    bsn::copy_d2h(k->bed, ibs, k->d_ibs->p, (size_t)k->count * 12);
    bsn::copy_d2h(k->bed, est, k->d_est->p, (size_t)k->count * 40);
  });
}

int bsn_ibd_free(bsn_ibd *k) {
  return bsn::guarded([&] { delete k; });
}

int bsn_ibd_last_ms(double *ms_out) {
  return bsn::guarded([&] {
    for (int q = 0; q < 6; q++) ms_out[q] = bsn::g_last_ms[q];
  });
}

}  // extern "C"
