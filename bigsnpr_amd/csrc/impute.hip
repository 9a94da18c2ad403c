// impute.hip — snp_fastImputeSimple on the device (bsn_impute_simple): the value of every variant from its code counts,
// then one streaming rewrite of the resident 2-bit image into a NEW image — 2-bit for zero / mode / mean0 / random, the
// int8 grid image of CODE_DOSAGE for mean2 — and, on request, the bytes the reference's FBM file would hold.
//
// Replaces src/impute-simple.cpp:10-73 (the element loop over a memory-mapped byte matrix, rewritten in place) behind
// R/impute.R:189-203.  The rules themselves live in impute_step.hpp, shared with the CPU statement.  DESIGN.md 3.5g.
#include <algorithm>
#include <memory>
#include <vector>

#include "bsn_internal.hpp"
#include "impute_step.hpp"

namespace bsn {
namespace {

// what decides when a loop of the kernels below goes round again (tests/helpers/impute_inputs.py reads these lines and
// tests/test_impute_shapes_cpu.py holds the shapes of tests/test_gpu_impute_shapes.py against them)
constexpr int64_t kRewriteVecs = 256;      // rewrite grid: 16-B vectors of a row per workgroup in x (four turns of a wave)
constexpr int64_t kRewriteGroups = 2048;   // rewrite grid: workgroups in all, a stride for the rest
constexpr int64_t kBytesMaxCols = 65535;   // FBM bytes: variants per launch (gridDim.y)
constexpr int64_t kBytesChunkMiB = 256;    // FBM bytes: size of a column chunk
constexpr int64_t kBytesGroups = 1024;     // FBM bytes: workgroups over the samples of a variant, a stride for the rest

// device milliseconds of the last call of this process (bsn_impute_last_ms): counts + rule, rewrite, FBM bytes
double g_last_ms[3] = {0.0, 0.0, 0.0};

// ---- per variant: counts -> value -------------------------------------------------------------------------------------
// counts: 4 x m (codes 0, 1, 2, missing) over all n samples.  n_all receives the number of variants without a call.
__global__ void k_impute_rule(const int32_t *__restrict__ counts, int64_t m, int64_t n, int method, int32_t *val,
                              double *af, unsigned long long *n_all) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int4 c = *(const int4 *)(counts + 4 * j);
  const int64_t nn = n - c.w;
  const impute::Rule r = impute::rule(method, c.y, c.z, nn);
  val[j] = r.val;
  af[j] = r.af;
  if (nn == 0) atomicAdd(n_all, 1ull);
}

// ---- 2-bit -> 2-bit -------------------------------------------------------------------------------------------------------
// One wave per variant and turn, two loads of 16 B (64 genotypes each) in flight per lane: x -> (x & ~(3 m)) | (v m) with m
// the missing fields.  The whole pitch is rewritten: pad samples are zero fields, never missing, and leave as they came.
// A variant whose value is -1 is copied.  RANDOM: a draw per set field of m (1 % of the fields on real data), nothing for the others.
template <bool RANDOM>
__global__ __launch_bounds__(256) void k_impute_2bit(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                     int64_t pitch, int64_t m, const int32_t *__restrict__ val,
                                                     const double *__restrict__ af, uint64_t seed) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t nvec = pitch / 16;
  for (int64_t j = (int64_t)blockIdx.y * 4 + wave; j < m; j += (int64_t)gridDim.y * 4) {
    const int32_t v = val[j];
    const double a = RANDOM ? af[j] : 0.0;
    const uint4 *in = (const uint4 *)(src + j * pitch);
    uint4 *out = (uint4 *)(dst + j * pitch);
    // two vectors per turn, both loads issued before either is worked on
    const int64_t step = (int64_t)gridDim.x * 64;
    for (int64_t t = (int64_t)blockIdx.x * 64 + lane; t < nvec; t += 2 * step) {
      const bool two = t + step < nvec;
      const uint4 x0 = in[t];
      uint4 x1 = {0, 0, 0, 0};
      if (two) x1 = in[t + step];
      uint32_t w[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
      if (v >= 0) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
          if (RANDOM) {
            const int64_t tq = q < 4 ? t : t + step;
            if (impute::missing_mask(w[q])) w[q] = impute::fill_word_random(w[q], seed, (uint64_t)(tq * 64 + (q & 3) * 16), (uint64_t)j, a);
          } else {
            w[q] = impute::fill_word(w[q], (uint32_t)v);
          }
        }
      }
      out[t] = uint4{w[0], w[1], w[2], w[3]};
      if (two) out[t + step] = uint4{w[4], w[5], w[6], w[7]};
    }
  }
}

// ---- 2-bit -> int8 grid image (mean2) ---------------------------------------------------------------------------------
// One dword of 16 genotypes per lane -> one 16-byte store.  Grid index 100 g - 100 for a call, r - 100 for an imputed
// value, -128 where the variant stays missing; samples at or past n are pad bytes, 0.  dpitch (n rounded up to 256) never
// exceeds 4 * spitch, so every dword read lies inside the source row.
__global__ __launch_bounds__(256) void k_impute_grid8(const uint8_t *__restrict__ src, int64_t spitch,
                                                      uint8_t *__restrict__ dst, int64_t dpitch, int64_t n, int64_t m,
                                                      const int32_t *__restrict__ val) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t nvec = dpitch / 16;
  for (int64_t j = (int64_t)blockIdx.y * 4 + wave; j < m; j += (int64_t)gridDim.y * 4) {
    // byte c of the table = grid index of code c
    const uint32_t lut = 0x9Cu | (0x00u << 8) | (0x64u << 16) | ((uint32_t)(uint8_t)impute::grid_index(val[j]) << 24);
    const uint32_t *in = (const uint32_t *)(src + j * spitch);
    uint4 *out = (uint4 *)(dst + j * dpitch);
    for (int64_t t = (int64_t)blockIdx.x * 64 + lane; t < nvec; t += (int64_t)gridDim.x * 64) {
      const uint32_t x = in[t];
      const int64_t left = n - t * 16;   // real samples from the start of this dword
      uint32_t o[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        uint32_t r = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int f = 4 * q + e;
          const uint32_t code = (x >> (2 * f)) & 3u;
          const uint32_t byte = f < left ? (lut >> (8 * code)) & 0xFFu : 0u;
          r |= byte << (8 * e);
        }
        o[q] = r;
      }
      out[t] = uint4{o[0], o[1], o[2], o[3]};
    }
  }
}

// ---- 2-bit -> the FBM's bytes -------------------------------------------------------------------------------------------
// out: n x cnt column-major (ld = n) for the variants j0 .. j0 + cnt - 1: the call 0 / 1 / 2 where there is one, the
// reference's marker (4 + call, 7 + r, or 3) at a missing position.  One sample per thread: byte stores, a column of
// the FBM starts at any address.  The draws of `random` are the ones the image received (same seed, i, j, af).
__global__ __launch_bounds__(256) void k_impute_bytes(const uint8_t *__restrict__ src, int64_t pitch, int64_t n, int64_t j0,
                                                      int method, const int32_t *__restrict__ val,
                                                      const double *__restrict__ af, uint64_t seed, uint8_t *out) {
  const int64_t jj = blockIdx.y, j = j0 + jj;
  const int32_t v = val[j];
  const double a = af[j];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t code = (src[j * pitch + (i >> 2)] >> (2 * (i & 3))) & 3u;
    uint8_t b = (uint8_t)code;
    if (code == 3) b = impute::fbm_byte(method, method == impute::kRandom && v >= 0 ? impute::draw(seed, (uint64_t)i, (uint64_t)j, a) : v);
    out[jj * n + i] = b;
  }
}

// grid of the two rewrite kernels: x over the 16-B vectors of a row (at most four turns per lane), y over groups of four
// variants, about 2048 workgroups in all with a stride for the rest
dim3 rewrite_grid(int64_t nvec, int64_t m) {
  const int64_t gx = std::max<int64_t>(1, std::min<int64_t>((nvec + kRewriteVecs - 1) / kRewriteVecs, kRewriteGroups));
  const int64_t gy = std::max<int64_t>(1, std::min<int64_t>((m + 3) / 4, std::max<int64_t>(1, kRewriteGroups / gx)));
  return dim3((unsigned)gx, (unsigned)gy);
}

void impute_simple(bsn_bed *src, int method, uint64_t seed, bsn_bed **out, uint8_t *fbm_bytes_out, int64_t *n_all_missing) {
  require_gpu();
  if (!src) fail("snp_fastImputeSimple: no genotype handle");
  if (!out && !fbm_bytes_out) fail("snp_fastImputeSimple: neither a result handle nor the FBM bytes were asked for");
  if (method < impute::kZero || method > impute::kRandom) fail("Parameter 'method' should be 0, 1, 2, 3, or 4.");
  require_resident(src, "snp_fastImputeSimple");
  refuse_generic(src, "snp_fastImputeSimple");
  require_bits(src, 2, "snp_fastImputeSimple");
  if (src->n >= (int64_t)1 << 31 || src->m >= (int64_t)1 << 31) fail("dimension too large");
  BSN_HIP(hipSetDevice(src->device));
  const int64_t n = src->n, m = src->m;
  const int bits = method == impute::kMean2 ? 8 : 2;

  std::unique_ptr<bsn_bed, void (*)(bsn_bed *)> res(nullptr, bed_free);
  if (out) {
    // does the result fit?  (image_alloc would fail with the runtime's "out of memory"; this names the reason)
    const int64_t pitch = round_up(bits == 8 ? n : (n + 3) / 4, kPitchAlign);
    const double need = (double)(m + 64) * (double)pitch;
    size_t free_b = 0, total_b = 0;
    BSN_HIP(hipMemGetInfo(&free_b, &total_b));
    const double room = (double)(free_b + dev_cache_held());
    if (need > room)
      fail("snp_fastImputeSimple: the result image (%.2f GB, %s) does not fit the free device memory (%.2f GB); the source "
           "stays resident beside it",
           need / 1e9, bits == 8 ? "one byte per genotype for 'mean2'" : "2 bits per genotype", room / 1e9);
    res.reset(new bsn_bed());
    image_alloc(res.get(), n, m, bits);
    if (bits == 8) {
      res->v_off = 1.0;   // the grid bsn_fbm_open derives from CODE_DOSAGE: 0.00 .. 2.00 by 0.01 about 1
      res->v_step = 2.0 / 200.0;
    }
  }

  // ---- counts over all samples: the handle's device-resident ones when they are there, one counting pass otherwise ----
  hipStream_t st = src->stream;
  DevBuf<int32_t> d_counts, d_val;
  DevBuf<double> d_af;
  DevBuf<unsigned long long> d_nall;
  d_counts.ensure((size_t)4 * m);
  EventMarks<2> ev_rule, ev_write;
  g_last_ms[0] = g_last_ms[1] = g_last_ms[2] = 0.0;
  ev_rule.mark(0, st);
  const StatsCols sel{nullptr, nullptr, 0, m};
  const bool cache = stats_cache_enabled(src);
  if (cache && stats_cache_known(src, sel)) {
    stats_cache_load(src, sel, d_counts.p, st);
  } else {
    counts_all_rows(src, nullptr, 0, m, d_counts.p);
    if (cache) stats_cache_store(src, sel, d_counts.p, st);   // (this call synchronises the stream before it returns)
  }
  d_val.ensure((size_t)m);
  d_af.ensure((size_t)m);
  BSN_HIP(hipMemsetAsync(d_nall.ensure(1), 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_impute_rule, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, d_counts.p, m, n, method, d_val.p,
                     d_af.p, d_nall.p);
  BSN_HIP(hipGetLastError());
  ev_rule.mark(1, st);

  // ---- the rewrite ------------------------------------------------------------------------------------------------------
  if (res) {
    bsn_bed *r = res.get();
    ev_write.mark(0, st);
    if (bits == 2) {
      if (r->pitch != src->pitch) fail("internal: pitch of the imputed image");
      const dim3 grid = rewrite_grid(r->pitch / 16, m);
      if (method == impute::kRandom)
        hipLaunchKernelGGL(k_impute_2bit<true>, grid, dim3(256), 0, st, src->d_img, r->d_img, r->pitch, m, d_val.p, d_af.p, seed);
      else
        hipLaunchKernelGGL(k_impute_2bit<false>, grid, dim3(256), 0, st, src->d_img, r->d_img, r->pitch, m, d_val.p, d_af.p, seed);
    } else {
      if (r->pitch > 4 * src->pitch) fail("internal: pitch of the imputed image");
      hipLaunchKernelGGL(k_impute_grid8, rewrite_grid(r->pitch / 16, m), dim3(256), 0, st, src->d_img, src->pitch, r->d_img,
                         r->pitch, n, m, d_val.p);
    }
    BSN_HIP(hipGetLastError());
    ev_write.mark(1, st);
    BSN_HIP(hipMemsetAsync(r->d_img + m * r->pitch, 0, (size_t)(64 * r->pitch), st));   // the pad variants
  }

  // ---- what the host needs: which variants stayed missing, how many had no call ------------------------------------------
  std::vector<int32_t> val((size_t)m);
  copy_d2h(src, val.data(), d_val.p, (size_t)m * 4);
  unsigned long long nall = 0;
  copy_d2h(src, &nall, d_nall.p, sizeof(nall));
  BSN_HIP(hipStreamSynchronize(st));
  if (n_all_missing) *n_all_missing = (int64_t)nall;
  g_last_ms[0] = ev_rule.ms(0, 1);
  if (res) g_last_ms[1] = ev_write.ms(0, 1);
  if (res) {
    res->na_cnt.resize((size_t)m);
    for (int64_t j = 0; j < m; j++) res->na_cnt[(size_t)j] = val[(size_t)j] < 0 ? (int32_t)n : 0;
  }

  // ---- the FBM's bytes, in column chunks of at most 256 MB ---------------------------------------------------------------
  if (fbm_bytes_out) {
    int64_t cols_per =
        std::max<int64_t>(1, std::min<int64_t>(kBytesMaxCols, (int64_t)(((size_t)kBytesChunkMiB << 20) / (size_t)n)));
    cols_per = std::min(cols_per, m);
    DevBuf<uint8_t> tmp;
    tmp.ensure((size_t)cols_per * (size_t)n);
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, kBytesGroups));
    for (int64_t j0 = 0; j0 < m; j0 += cols_per) {
      const int64_t cnt = std::min(cols_per, m - j0);
      ev_write.mark(0, st);
      hipLaunchKernelGGL(k_impute_bytes, dim3(gx, (unsigned)cnt), dim3(256), 0, st, src->d_img, src->pitch, n, j0, method,
                         d_val.p, d_af.p, seed, tmp.p);
      BSN_HIP(hipGetLastError());
      ev_write.mark(1, st);
      copy_d2h(src, fbm_bytes_out + j0 * n, tmp.p, (size_t)cnt * (size_t)n);
      BSN_HIP(hipStreamSynchronize(st));
      g_last_ms[2] += ev_write.ms(0, 1);
    }
  }
  if (out) *out = res.release();
}

}  // namespace
}  // namespace bsn

extern "C" {

int bsn_impute_simple(bsn_bed *src, int method, uint64_t seed, bsn_bed **out, uint8_t *fbm_bytes_out, int64_t *n_all_missing) {
  return bsn::guarded([&] { bsn::impute_simple(src, method, seed, out, fbm_bytes_out, n_all_missing); });
}

int bsn_impute_last_ms(double *ms_out) {
  return bsn::guarded([&] {
    for (int k = 0; k < 3; k++) ms_out[k] = bsn::g_last_ms[k];
  });
}

}  // extern "C"
