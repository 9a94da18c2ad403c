// fastimpute.hip — snp_fastImpute on the device (bsn_fast_impute): for every variant with a missing and an observed call,
// ten rounds of depth-4 boosted trees on the 2-bit codes of its predictors, trained on a draw of its observed samples,
// validated on the others, and the calls of the final margin written at its missing positions of a NEW 2-bit image.
//
// Replaces the loop of R/impute.R:29-160 (one xgboost model per variant, each seeing the calls imputed before it) by one
// independent model per variant that reads the source image.  The statement lives in fastimpute_step.hpp, shared with
// the CPU statement (tests/native/fastimpute_ref.cpp).  DESIGN.md 3.5q.
#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>
#include <vector>

#include "bsn_internal.hpp"
#include "fastimpute_step.hpp"

namespace bsn {
namespace {

// what decides when a loop of the kernels below goes round again, and which kernel runs (tests/test_gpu_fastimpute.py
// reads these lines and picks its shapes from them)
constexpr int kBoostThreads = 512;                     // a workgroup per target; a lane takes a byte of four samples
constexpr int64_t kTurnSamples = 4 * kBoostThreads;    // samples per workgroup turn
constexpr int kFeatTurn = 8;                           // predictors whose histograms are built in one pass over the samples
constexpr int64_t kGridTargets = 1024;                 // workgroups at most; a workgroup strides over the targets beyond
constexpr int64_t kLdsSamples = 8192;                  // per-sample state in LDS up to this many samples, in global scratch beyond
constexpr int64_t kBytesMaxCols = 65535;               // FBM bytes: variants per launch (gridDim.y)
constexpr int64_t kBytesChunkMiB = 256;                // FBM bytes: size of a column chunk
constexpr int64_t kBytesGroups = 1024;                 // FBM bytes: workgroups over the samples of a variant, a stride for the rest

constexpr int kStateBytes = 18;   // per sample: margin (8), gq (4), hq (4), node (1), role and call (1)
constexpr int kPad = 3;           // role of a field past sample n - 1
static_assert(kLdsSamples % kTurnSamples == 0 && kLdsSamples * kStateBytes <= 150 * 1024, "the state of kLdsSamples samples beside 8 KiB of histograms");

// device milliseconds of the last call of this process (bsn_fast_impute_last_ms): boosting kernel, image copy, FBM bytes
double g_last_ms[3] = {0.0, 0.0, 0.0};

extern __shared__ __attribute__((aligned(16))) uint8_t fimp_lds[];

// ---- one workgroup per target ---------------------------------------------------------------------------------------------
// Per-sample state (margin, quantised gradient and hessian, node, role) in LDS (LDS) or in this workgroup's slice of
// `scratch`.  Per level and turn of kFeatTurn predictors, one pass over the samples adds (gq, hq) into the 64-bit LDS
// histograms [predictor][node of the level][code 1, 2, missing]; code 0, the common one, is the node's sums minus the
// three.  Integer sums: the order in which lanes arrive does not matter.  Then a thread per (predictor, node) scans the
// six candidates and a thread per node merges the predictors in ascending position, which is the tie rule.
// valid: 2 x ntargets (errors on the validation samples, their number).
template <bool LDS>
__global__ __launch_bounds__(kBoostThreads) void k_fimp_boost(const uint8_t *__restrict__ src, uint8_t *dst, int64_t pitch,
                                                              int64_t n, const int32_t *__restrict__ targets, int64_t ntargets,
                                                              const int64_t *__restrict__ pred_off,
                                                              const int32_t *__restrict__ pred_idx, double p_train, uint64_t seed,
                                                              uint8_t *scratch, int64_t scratch_stride, int32_t *valid) {
  __shared__ unsigned long long hist[kFeatTurn][fimp::kLevelNodes][4][2];
  __shared__ fimp::Best bestf[kFeatTurn][fimp::kLevelNodes];
  __shared__ fimp::Best best[fimp::kLevelNodes];
  __shared__ unsigned long long nodeG[fimp::kNodes], nodeH[fimp::kNodes];
  __shared__ int32_t tfeat[fimp::kNodes], tthr[fimp::kNodes], tdir[fimp::kNodes];
  __shared__ double tw[fimp::kNodes];
  __shared__ int32_t cnt[8];   // training samples, their calls 1 and 2; observed samples, their calls 1 and 2; validation errors, samples

  const int tid = threadIdx.x;
  const int64_t nb = (n + 3) / 4, n4 = 4 * nb;
  uint8_t *base = LDS ? fimp_lds : scratch + (int64_t)blockIdx.x * scratch_stride;
  double *margin = (double *)base;
  int32_t *gq = (int32_t *)(base + 8 * n4);
  int32_t *hq = (int32_t *)(base + 12 * n4);
  uint8_t *node = base + 16 * n4;
  uint8_t *role = base + 17 * n4;   // role | code << 2

  for (int64_t tix = blockIdx.x; tix < ntargets; tix += gridDim.x) {
    const int64_t j = targets[tix];
    const int32_t *P = pred_idx + pred_off[j];
    const int64_t np = pred_off[j + 1] - pred_off[j];
    const uint8_t *row = src + j * pitch;

    // ---- roles and the starting margin
    if (tid < 8) cnt[tid] = 0;
    __syncthreads();
    {
      int32_t c[6] = {0, 0, 0, 0, 0, 0};
      for (int64_t b = tid; b < nb; b += kBoostThreads) {
        const uint32_t x = row[b];
        for (int e = 0; e < 4; e++) {
          const int64_t i = 4 * b + e;
          const int code = (int)((x >> (2 * e)) & 3u);
          int r = kPad;
          if (i < n) {
            r = code == 3 ? fimp::kFill : fimp::draws_train(seed, (uint64_t)i, (uint64_t)j, p_train) ? fimp::kTrain : fimp::kValid;
            if (code != 3) c[3]++, c[4] += code == 1, c[5] += code == 2;
            if (r == fimp::kTrain) c[0]++, c[1] += code == 1, c[2] += code == 2;
          }
          role[i] = (uint8_t)(r | (code << 2));
        }
      }
      for (int q = 0; q < 6; q++)
        if (c[q]) atomicAdd(&cnt[q], c[q]);
    }
    __syncthreads();
    const bool all_train = cnt[0] == 0;   // nobody drew a training role: every observed sample trains, nobody validates
    const double m0 = all_train ? fimp::start_margin(cnt[4], cnt[5], cnt[3]) : fimp::start_margin(cnt[1], cnt[2], cnt[0]);
    for (int64_t b = tid; b < nb; b += kBoostThreads)
      for (int e = 0; e < 4; e++) {
        const int64_t i = 4 * b + e;
        margin[i] = m0;
        if (all_train && (role[i] & 3) == fimp::kValid) role[i] = (uint8_t)((role[i] & ~3) | fimp::kTrain);
      }

    for (int round = 0; round < fimp::kRounds; round++) {
      __syncthreads();
      if (tid < fimp::kNodes) {
        tfeat[tid] = tid == 0 ? -1 : -2;   // -1: a leaf so far, -2: absent
        tthr[tid] = tdir[tid] = 0;
        nodeG[tid] = nodeH[tid] = 0ull;
        tw[tid] = 0.0;
      }
      __syncthreads();
      // ---- gradients of the training samples, the root's sums
      {
        int64_t sg = 0, sh = 0;
        for (int64_t b = tid; b < nb; b += kBoostThreads)
          for (int e = 0; e < 4; e++) {
            const int64_t i = 4 * b + e;
            node[i] = 0;
            const int r = role[i];
            if ((r & 3) != fimp::kTrain) continue;
            int32_t g, h;
            fimp::grad(margin[i], r >> 2, &g, &h);
            gq[i] = g;
            hq[i] = h;
            sg += g;
            sh += h;
          }
        atomicAdd(&nodeG[0], (unsigned long long)sg);
        atomicAdd(&nodeH[0], (unsigned long long)sh);
      }
      __syncthreads();

      for (int level = 0; level < fimp::kMaxDepth; level++) {
        const int first = (1 << level) - 1, nn = 1 << level;
        if (tid < nn) best[tid] = fimp::no_split();
        for (int64_t f0 = 0; f0 < np; f0 += kFeatTurn) {
          const int nf = (int)(np - f0 < kFeatTurn ? np - f0 : kFeatTurn);
          for (int q = tid; q < kFeatTurn * fimp::kLevelNodes * 8; q += kBoostThreads) (&hist[0][0][0][0])[q] = 0ull;
          __syncthreads();
          for (int64_t b = tid; b < nb; b += kBoostThreads) {
            int k[4];
            bool any = false;
            for (int e = 0; e < 4; e++) {
              const int64_t i = 4 * b + e;
              k[e] = (role[i] & 3) == fimp::kTrain ? (int)node[i] - first : -1;
              any = any || k[e] >= 0;
            }
            if (!any) continue;
            for (int f = 0; f < nf; f++) {
              const uint32_t x = src[(int64_t)P[f0 + f] * pitch + b];
              for (int e = 0; e < 4; e++) {
                const int c = (int)((x >> (2 * e)) & 3u);
                if (k[e] < 0 || c == 0) continue;
                const int64_t i = 4 * b + e;
                atomicAdd(&hist[f][k[e]][c][0], (unsigned long long)(int64_t)gq[i]);
                atomicAdd(&hist[f][k[e]][c][1], (unsigned long long)(int64_t)hq[i]);
              }
            }
          }
          __syncthreads();
          if (tid < nf * nn) {
            const int f = tid / nn, kk = tid % nn, id = first + kk;
            fimp::Best b = fimp::no_split();
            if (tfeat[id] == -1) {
              int64_t gc[4], hc[4];
              const int64_t G = (int64_t)nodeG[id], H = (int64_t)nodeH[id];
              gc[0] = G, hc[0] = H;
              for (int c = 1; c < 4; c++) {
                gc[c] = (int64_t)hist[f][kk][c][0];
                hc[c] = (int64_t)hist[f][kk][c][1];
                gc[0] -= gc[c];
                hc[0] -= hc[c];
              }
              fimp::scan_feature(gc, hc, G, H, (int32_t)(f0 + f), &b);
            }
            bestf[f][kk] = b;
          }
          __syncthreads();
          if (tid < nn)
            for (int f = 0; f < nf; f++)
              if (fimp::better(bestf[f][tid], best[tid])) best[tid] = bestf[f][tid];
          __syncthreads();
        }
        // ---- split or leaf
        __syncthreads();
        if (tid < nn) {
          const int id = first + tid;
          if (tfeat[id] == -1) {
            const fimp::Best b = best[tid];
            if (b.feat >= 0) {
              tfeat[id] = b.feat, tthr[id] = b.t, tdir[id] = b.dir;
              tfeat[2 * id + 1] = tfeat[2 * id + 2] = -1;
              nodeG[2 * id + 1] = (unsigned long long)b.GL;
              nodeH[2 * id + 1] = (unsigned long long)b.HL;
              nodeG[2 * id + 2] = nodeG[id] - (unsigned long long)b.GL;
              nodeH[2 * id + 2] = nodeH[id] - (unsigned long long)b.HL;
            } else {
              tw[id] = fimp::leaf_weight((int64_t)nodeG[id], (int64_t)nodeH[id]);
            }
          }
        }
        __syncthreads();
        // ---- every sample of a node that split moves to a child
        for (int64_t b = tid; b < nb; b += kBoostThreads)
          for (int e = 0; e < 4; e++) {
            const int64_t i = 4 * b + e;
            const int id = node[i];
            if ((role[i] & 3) == kPad || id < first || tfeat[id] < 0) continue;
            const int c = (int)((src[(int64_t)P[tfeat[id]] * pitch + b] >> (2 * e)) & 3u);
            node[i] = (uint8_t)(fimp::goes_left(c, tthr[id], tdir[id]) ? 2 * id + 1 : 2 * id + 2);
          }
        __syncthreads();
      }
      if (tid < (1 << fimp::kMaxDepth)) {
        const int id = (1 << fimp::kMaxDepth) - 1 + tid;
        if (tfeat[id] == -1) tw[id] = fimp::leaf_weight((int64_t)nodeG[id], (int64_t)nodeH[id]);
      }
      __syncthreads();
      for (int64_t b = tid; b < nb; b += kBoostThreads)
        for (int e = 0; e < 4; e++) {
          const int64_t i = 4 * b + e;
          if ((role[i] & 3) != kPad) margin[i] = margin[i] + tw[node[i]];
        }
    }

    // ---- calls: into the missing fields of the new image, against the observed call of the validation samples
    {
      int32_t nerr = 0, nval = 0;
      for (int64_t b = tid; b < nb; b += kBoostThreads) {
        uint32_t x = row[b];
        for (int e = 0; e < 4; e++) {
          const int64_t i = 4 * b + e;
          const int r = role[i] & 3;
          if (r != fimp::kFill && r != fimp::kValid) continue;
          const int call = fimp::call_of(margin[i]);
          if (r == fimp::kFill) {
            x = (x & ~(3u << (2 * e))) | ((uint32_t)call << (2 * e));
          } else {
            nval++;
            nerr += call != (role[i] >> 2);
          }
        }
        dst[j * pitch + b] = (uint8_t)x;
      }
      if (nerr) atomicAdd(&cnt[6], nerr);
      if (nval) atomicAdd(&cnt[7], nval);
    }
    __syncthreads();
    if (tid == 0) {
      valid[2 * tix] = cnt[6];
      valid[2 * tix + 1] = cnt[7];
    }
    __syncthreads();
  }
}

// ---- source and result -> the FBM's bytes -----------------------------------------------------------------------------------
// out: n x cnt column-major for the variants j0 .. j0 + cnt - 1: the call where the source has one, 4 + the result's call
// (CODE_IMPUTE_PRED) at a missing position, 3 where the result is missing too.  One sample per thread, byte stores.
__global__ __launch_bounds__(256) void k_fimp_bytes(const uint8_t *__restrict__ src, const uint8_t *__restrict__ res,
                                                    int64_t pitch, int64_t n, int64_t j0, uint8_t *out) {
  const int64_t jj = blockIdx.y, j = j0 + jj;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t s = (src[j * pitch + (i >> 2)] >> (2 * (i & 3))) & 3u;
    const uint32_t r = (res[j * pitch + (i >> 2)] >> (2 * (i & 3))) & 3u;
    out[jj * n + i] = (uint8_t)(s != 3 ? s : r == 3 ? 3 : 4 + r);
  }
}

void fast_impute(bsn_bed *src, const int64_t *pred_off, const int32_t *pred_idx, double p_train, uint64_t seed, bsn_bed **out,
                 uint8_t *fbm_bytes_out, double *infos, int64_t *n_all_missing) {
  require_gpu();
  if (!src) fail("snp_fastImpute: no genotype handle");
  if (!pred_off) fail("snp_fastImpute: no predictor lists");
  if (!out && !fbm_bytes_out && !infos) fail("snp_fastImpute: neither a result handle, the FBM bytes nor the infos were asked for");
  if (!(p_train > 0.0 && p_train <= 1.0)) fail("snp_fastImpute: 'p_train' must lie in (0, 1].");
  require_resident(src, "snp_fastImpute");
  refuse_generic(src, "snp_fastImpute");
  require_bits(src, 2, "snp_fastImpute");
  if (src->n >= (int64_t)1 << 31 || src->m >= (int64_t)1 << 31) fail("dimension too large");
  const int64_t n = src->n, m = src->m;
  if (pred_off[0] != 0) fail("snp_fastImpute: the predictor offsets do not start at 0");
  for (int64_t j = 0; j < m; j++) {
    if (pred_off[j + 1] < pred_off[j]) fail("snp_fastImpute: the predictor offsets decrease at variant %lld", (long long)j);
    for (int64_t q = pred_off[j]; q < pred_off[j + 1]; q++) {
      if (pred_idx[q] < 0 || pred_idx[q] >= m)
        fail("snp_fastImpute: predictor %d of variant %lld lies outside [0, %lld)", (int)pred_idx[q], (long long)j, (long long)m);
      if (pred_idx[q] == j) fail("snp_fastImpute: variant %lld is named as its own predictor", (long long)j);
    }
  }
  const int64_t total = pred_off[m];
  BSN_HIP(hipSetDevice(src->device));
  hipStream_t st = src->stream;

  // ---- room for the result image and the scratch
  const int64_t n4 = round_up(n, 4);
  const bool lds = n4 <= kLdsSamples;
  const int64_t stride = lds ? 0 : round_up(kStateBytes * n4, 256);
  {
    const double need = (double)(m + 64) * (double)src->pitch, need_scratch = (double)stride * (double)std::min(kGridTargets, m);
    size_t free_b = 0, total_b = 0;
    BSN_HIP(hipMemGetInfo(&free_b, &total_b));
    const double room = (double)(free_b + dev_cache_held());
    if (need > room)
      fail("snp_fastImpute: the result image (%.2f GB, 2 bits per genotype) does not fit the free device memory (%.2f GB); the "
           "source stays resident beside it",
           need / 1e9, room / 1e9);
    if (need + need_scratch > room)
      fail("snp_fastImpute: the per-sample scratch (%.2f GB for %lld workgroups) does not fit the free device memory beside the "
           "result image (%.2f GB left)",
           need_scratch / 1e9, (long long)std::min(kGridTargets, m), (room - need) / 1e9);
  }
  std::unique_ptr<bsn_bed, void (*)(bsn_bed *)> res(new bsn_bed(), bed_free);
  image_alloc(res.get(), n, m, 2);
  if (res->pitch != src->pitch) fail("internal: pitch of the imputed image");
  const int64_t pitch = src->pitch;

  // ---- who is a target: counts over all samples, as snp_fastImputeSimple takes them
  DevBuf<int32_t> d_counts;
  d_counts.ensure((size_t)4 * m);
  const StatsCols sel{nullptr, nullptr, 0, m};
  const bool cache = stats_cache_enabled(src);
  if (cache && stats_cache_known(src, sel)) {
    stats_cache_load(src, sel, d_counts.p, st);
  } else {
    counts_all_rows(src, nullptr, 0, m, d_counts.p);
    if (cache) stats_cache_store(src, sel, d_counts.p, st);
  }
  std::vector<int32_t> counts((size_t)4 * m);
  copy_d2h(src, counts.data(), d_counts.p, (size_t)4 * m * 4);
  BSN_HIP(hipStreamSynchronize(st));
  std::vector<int32_t> targets;
  int64_t n_all = 0;
  for (int64_t j = 0; j < m; j++) {
    const int64_t miss = counts[(size_t)(4 * j + 3)];
    if (miss > 0 && miss < n) targets.push_back((int32_t)j);
    n_all += miss == n;
  }
  const int64_t nt = (int64_t)targets.size();

  // ---- the new image starts as a copy; the boosting kernel rewrites the bytes of its targets
  EventMarks<2> ev_copy, ev_boost, ev_bytes;
  g_last_ms[0] = g_last_ms[1] = g_last_ms[2] = 0.0;
  ev_copy.mark(0, st);
  BSN_HIP(hipMemcpyAsync(res->d_img, src->d_img, (size_t)(m * pitch), hipMemcpyDeviceToDevice, st));
  BSN_HIP(hipMemsetAsync(res->d_img + m * pitch, 0, (size_t)(64 * pitch), st));   // the pad variants
  ev_copy.mark(1, st);

  std::vector<int32_t> valid((size_t)(2 * std::max<int64_t>(nt, 1)), 0);
  if (nt > 0) {
    DevBuf<int64_t> d_off;
    DevBuf<int32_t> d_idx, d_targets, d_valid;
    DevBuf<uint8_t> d_scratch;
    const int64_t grid = std::min(kGridTargets, nt);
    copy_h2d(src, d_off.ensure((size_t)(m + 1)), pred_off, (size_t)(m + 1) * 8);
    d_idx.ensure((size_t)std::max<int64_t>(total, 1));
    if (total > 0) copy_h2d(src, d_idx.p, pred_idx, (size_t)total * 4);
    copy_h2d(src, d_targets.ensure((size_t)nt), targets.data(), (size_t)nt * 4);
    d_valid.ensure((size_t)(2 * nt));
    if (!lds) d_scratch.ensure((size_t)(stride * grid));
    ev_boost.mark(0, st);
    if (lds) {
      const size_t dyn = (size_t)(kStateBytes * n4);
      BSN_HIP(hipFuncSetAttribute((const void *)k_fimp_boost<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
      hipLaunchKernelGGL(k_fimp_boost<true>, dim3((unsigned)grid), dim3(kBoostThreads), dyn, st, src->d_img, res->d_img, pitch, n,
                         d_targets.p, nt, d_off.p, d_idx.p, p_train, seed, (uint8_t *)nullptr, (int64_t)0, d_valid.p);
    } else {
      hipLaunchKernelGGL(k_fimp_boost<false>, dim3((unsigned)grid), dim3(kBoostThreads), 0, st, src->d_img, res->d_img, pitch, n,
                         d_targets.p, nt, d_off.p, d_idx.p, p_train, seed, d_scratch.p, stride, d_valid.p);
    }
    BSN_HIP(hipGetLastError());
    ev_boost.mark(1, st);
    copy_d2h(src, valid.data(), d_valid.p, (size_t)(2 * nt) * 4);
    BSN_HIP(hipStreamSynchronize(st));
    g_last_ms[0] = ev_boost.ms(0, 1);
  }
  BSN_HIP(hipStreamSynchronize(st));
  g_last_ms[1] = ev_copy.ms(0, 1);

  if (n_all_missing) *n_all_missing = n_all;
  if (infos) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t j = 0; j < m; j++) {
      infos[j] = (double)counts[(size_t)(4 * j + 3)] / (double)n;
      infos[m + j] = nan;
    }
    for (int64_t t = 0; t < nt; t++)
      if (valid[(size_t)(2 * t + 1)] > 0) infos[m + targets[(size_t)t]] = (double)valid[(size_t)(2 * t)] / (double)valid[(size_t)(2 * t + 1)];
  }
  res->na_cnt.resize((size_t)m);
  for (int64_t j = 0; j < m; j++) res->na_cnt[(size_t)j] = counts[(size_t)(4 * j + 3)] == n ? (int32_t)n : 0;

  // ---- the FBM's bytes, in column chunks of at most 256 MB
  if (fbm_bytes_out) {
    int64_t cols_per = std::max<int64_t>(1, std::min<int64_t>(kBytesMaxCols, (int64_t)(((size_t)kBytesChunkMiB << 20) / (size_t)n)));
    cols_per = std::min(cols_per, m);
    DevBuf<uint8_t> tmp;
    tmp.ensure((size_t)cols_per * (size_t)n);
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, kBytesGroups));
    for (int64_t j0 = 0; j0 < m; j0 += cols_per) {
      const int64_t c = std::min(cols_per, m - j0);
      ev_bytes.mark(0, st);
      hipLaunchKernelGGL(k_fimp_bytes, dim3(gx, (unsigned)c), dim3(256), 0, st, src->d_img, res->d_img, pitch, n, j0, tmp.p);
      BSN_HIP(hipGetLastError());
      ev_bytes.mark(1, st);
      copy_d2h(src, fbm_bytes_out + j0 * n, tmp.p, (size_t)c * (size_t)n);
      BSN_HIP(hipStreamSynchronize(st));
      g_last_ms[2] += ev_bytes.ms(0, 1);
    }
  }
  if (out) *out = res.release();
}

}  // namespace
}  // namespace bsn

extern "C" {

int bsn_fast_impute(bsn_bed *src, const int64_t *pred_off, const int32_t *pred_idx, double p_train, uint64_t seed, bsn_bed **out,
                    uint8_t *fbm_bytes_out, double *infos, int64_t *n_all_missing) {
  return bsn::guarded([&] { bsn::fast_impute(src, pred_off, pred_idx, p_train, seed, out, fbm_bytes_out, infos, n_all_missing); });
}

int bsn_fast_impute_last_ms(double *ms_out) {
  return bsn::guarded([&] {
    for (int k = 0; k < 3; k++) ms_out[k] = bsn::g_last_ms[k];
  });
}

}  // extern "C"
