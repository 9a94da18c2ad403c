// image.hip — the HBM-resident 2-bit genotype image: upload, FBM repack, synthetic
// generator, per-variant code counts, dense read-back.
//
// Replaces the storage accessors of the reference: `class bed` / bedAcc
// (src/bed-acc.h:18-82) and the byte-per-genotype FBM accessor used by the snp_*
// functions (bigstatsr SubBMCode256Acc; layout per src/read-plink.cpp:17-48).
#include <unistd.h>

#include <algorithm>
#include <cstring>
#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

#include "bsn_internal.hpp"

namespace bsn {

// ---------------------------------------------------------------------------
// In-place finish of an uploaded payload: .bed codes -> device codes (bsn_internal.hpp), pad
// bits of the last real byte and all pad bytes -> 0 (genotype 0, non-missing).  One thread
// per 16 B.
__global__ void k_recode_fix(uint8_t *img, int64_t pitch, int64_t n, int64_t n_byte, int64_t m, int recode) {
  const int64_t j = blockIdx.y + (int64_t)blockIdx.z * 65535;
  const int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
  if (b >= pitch || j >= m) return;
  uint4 *p = (uint4 *)(img + j * pitch + b);
  uint4 v = {0, 0, 0, 0};
  if (b < n_byte) {
    v = *p;
    if (recode) {
      v.x = dev_from_plink(v.x); v.y = dev_from_plink(v.y);
      v.z = dev_from_plink(v.z); v.w = dev_from_plink(v.w);
    }
    // genotypes at or beyond sample n in this 16-B group (64 samples) -> 0
    const int64_t left = n - b * 4;  // real samples from the start of the group
    if (left < 64) {
      uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int64_t l = left - 16 * q;
        if (l <= 0) w[q] = 0;
        else if (l < 16) w[q] &= (1u << (2 * (int)l)) - 1u;
      }
      v = uint4{w[0], w[1], w[2], w[3]};
    }
  }
  *p = v;
}

constexpr int64_t kPadRows = 64;  // extra all-zero rows after the last variant

void image_alloc(bsn_bed *b, int64_t n, int64_t m, int bits) {
  if (n <= 0 || m <= 0) fail("n and p must be positive.");
  b->n = n;
  b->m = m;
  b->bits = bits;
  b->n_byte = bits == 8 ? n : (n + 3) / 4;
  b->pitch = round_up(b->n_byte, kPitchAlign);
  BSN_HIP(hipGetDevice(&b->device));
  BSN_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
  BSN_HIP(hipEventCreate(&b->ev0));
  BSN_HIP(hipEventCreate(&b->ev1));
  size_t bytes = (size_t)(m + kPadRows) * (size_t)b->pitch;
  BSN_HIP(hipMalloc((void **)&b->d_img, bytes));
  b->cap_m = m;
  // a large image gets its page-locked staging buffers now (2 x 32 MB, ~ 12 ms): every entry point that moves host data
  // needs them, and the first call on the handle — the one callers time — should not be the one that makes them
  if (bytes >= ((size_t)1 << 30)) stage_init(b);
}

// ---- streaming layout (second copy) --------------------------------------------------------
// One workgroup copies one 16-KB tile: 64 variants x 256 B.  Source rows are read 256 B at a time (16 lanes
// x 16 B), the tile is written front to back; variants past the end are written as zeros.
__global__ __launch_bounds__(256) void k_tile_image(const uint8_t *__restrict__ img, int64_t pitch, int64_t m,
                                                    uint8_t *__restrict__ tiled) {
  const int64_t SB = pitch >> 8;
  const int64_t sb = blockIdx.x, vb = (int64_t)blockIdx.y + (int64_t)blockIdx.z * 65535;
  if (vb * 64 >= m) return;
  const int seg = threadIdx.x & 15, r0 = threadIdx.x >> 4;
  uint4 *dst = (uint4 *)(tiled + (vb * SB + sb) * 16384);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int row = r0 + 16 * i;
    const int64_t j = vb * 64 + row;
    uint4 v = {0, 0, 0, 0};
    if (j < m) v = *(const uint4 *)(img + j * pitch + sb * 256 + seg * 16);
    dst[row * 16 + seg] = v;
  }
}

static void tile_launch(bsn_bed *b) {
  const int64_t nvb = (b->m + 63) / 64;
  const int64_t gy = nvb < 65535 ? nvb : 65535, gz = (nvb + 65534) / 65535;
  hipLaunchKernelGGL(k_tile_image, dim3((unsigned)(b->pitch >> 8), (unsigned)gy, (unsigned)gz), dim3(256), 0,
                     b->stream, b->d_img, b->pitch, b->m, b->d_tiled);
  BSN_HIP(hipGetLastError());
}

bool image_tile(bsn_bed *b) {
  if (b->d_tiled) return true;
  if (b->streamed()) return false;
  if (b->tiled_tried || b->bits != 2 || getenv("BSN_NO_TILED")) return false;
  b->tiled_tried = true;
  BSN_HIP(hipSetDevice(b->device));
  const int64_t nvb = (b->m + 63) / 64;
  const size_t bytes = (size_t)nvb * 64 * (size_t)b->pitch;
  // leave room for the workspace of a solve and for the other entry points' buffers
  size_t free_b = 0, total_b = 0;
  BSN_HIP(hipMemGetInfo(&free_b, &total_b));
  if ((double)(free_b + dev_cache_held()) < (double)bytes + 24e9) return false;
  if (hipMalloc((void **)&b->d_tiled, bytes) != hipSuccess) {
    (void)hipGetLastError();
    b->d_tiled = nullptr;
    return false;
  }
  b->tiled_cap = bytes;
  tile_launch(b);
  return true;
}

// the image changed in place (image_gather with `reuse`): an existing streaming-layout copy holds the PREVIOUS selection.
// It is rebuilt inside its allocation when the new selection fits, dropped otherwise (the next solve asks for a new one).
// (Round 5 left it alone: a later solve on the one-block kernels — vec_floor < 0, slices fixed by the caller, BSN_NO_SMAJ,
// no room for the sample-major copy — then streamed the old selection's genotypes without any error.)
static void tiled_refresh(bsn_bed *b) {
  b->tiled_tried = false;
  if (!b->d_tiled) return;
  const size_t bytes = (size_t)((b->m + 63) / 64) * 64 * (size_t)b->pitch;
  if (bytes <= b->tiled_cap) {
    tile_launch(b);
    return;
  }
  BSN_HIP(hipStreamSynchronize(b->stream));
  (void)hipFree(b->d_tiled);
  b->d_tiled = nullptr;
  b->tiled_cap = 0;
}

// ---- sample-major copy (bsn_internal.hpp) ------------------------------------------------------------------
// One workgroup transposes 512 variants x 256 samples (2-bit elements): the 512 x 64 B of the variant-major tile go
// to LDS; thread (sq = t & 63, vq = t >> 6) reads the 64 bytes "4 samples 4 sq .. 4 sq + 3 of variants 64 vq .. + 63"
// and spreads their 2-bit fields over four 16-byte rows (one per sample, 64 variants each); the 256 x 128 B of the
// sample-major tile leave through LDS again so that every global store instruction writes whole 128-B lines — and, the
// copy being chunk-major, the whole tile is one contiguous 32-KB run.  Variants past m are written as zeros.  One-off,
// about one read + one write pass.
__global__ __launch_bounds__(512) void k_smaj_build(const uint8_t *__restrict__ img, int64_t pitch, int64_t m,
                                                    uint8_t *__restrict__ out, int64_t pitch_t, int64_t rows_t) {
  __shared__ uint32_t sin[512 * 17];   // 512 variant rows of 64 B, row pitch 68 B
  __shared__ uint4 sout[256 * 9];      // 256 sample rows of 128 B, row pitch 144 B; row of sample 4 sq + e at e * 64 + sq
  const int t = threadIdx.x;
  const int64_t s0 = (int64_t)blockIdx.x * 256;
  const int64_t v0 = ((int64_t)blockIdx.y + (int64_t)blockIdx.z * 65535) * 512;
  if (v0 / 4 >= pitch_t) return;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int idx = t + 512 * i, row = idx >> 2, seg = idx & 3;
    const int64_t j = v0 + row;
    uint4 v = {0, 0, 0, 0};
    if (j < m) v = *(const uint4 *)(img + j * pitch + (s0 >> 2) + seg * 16);
    uint32_t *d = sin + row * 17 + seg * 4;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  __syncthreads();
  const int sq = t & 63, vq = t >> 6;
  uint32_t o[4][4];
#pragma unroll
  for (int e = 0; e < 4; e++)
#pragma unroll
    for (int w = 0; w < 4; w++) o[e][w] = 0;
  const uint8_t *sb = (const uint8_t *)sin;
#pragma unroll
  for (int i = 0; i < 64; i++) {
    const uint32_t b = sb[(vq * 64 + i) * 68 + sq];
#pragma unroll
    for (int e = 0; e < 4; e++) o[e][i >> 4] |= ((b >> (2 * e)) & 3u) << (2 * (i & 15));
  }
#pragma unroll
  for (int e = 0; e < 4; e++) sout[(e * 64 + sq) * 9 + vq] = uint4{o[e][0], o[e][1], o[e][2], o[e][3]};
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int idx = t + 512 * i, row = idx >> 3, seg = idx & 7;   // row = sample of the tile
    const int64_t sidx = s0 + row;
    // chunk-major: the 128 B "512 variants v0 .. of sample sidx" at ((v0 / 512) * rows_t + sidx) * 128
    if (sidx < rows_t) *(uint4 *)(out + ((v0 >> 9) * rows_t + sidx) * 128 + seg * 16) = sout[((row & 3) * 64 + (row >> 2)) * 9 + seg];
  }
}

static void smaj_launch(bsn_bed *b, int64_t pitch_t, int64_t rows_t, uint8_t *dst = nullptr, hipStream_t st = nullptr) {
  if (!dst) {   // (the handle's own copy on the handle's stream; a background build passes its pending buffer and stream)
    b->pitch_smaj = pitch_t;
    b->rows_smaj = rows_t;
  }
  const int64_t nvb = pitch_t * 4 / 512;
  const int64_t gy = nvb < 65535 ? nvb : 65535, gz = (nvb + 65534) / 65535;
  hipLaunchKernelGGL(k_smaj_build, dim3((unsigned)(rows_t / 256), (unsigned)gy, (unsigned)gz), dim3(512), 0, st ? st : b->stream,
                     b->d_img, b->pitch, b->m, dst ? dst : b->d_smaj, pitch_t, rows_t);
  BSN_HIP(hipGetLastError());
}

static bool smaj_room(bsn_bed *b, size_t bytes) {
  // leave room for the workspace of a solve and for the other entry points' buffers
  size_t free_b = 0, total_b = 0;
  BSN_HIP(hipMemGetInfo(&free_b, &total_b));
  return (double)(free_b + dev_cache_held()) >= (double)bytes + 24e9;
}

// ---- the copy made beside the first solve (round 6) ---------------------------------------------------
// The reference's unit of work is ONE bed_randomSVD on a freshly opened object (R/autoSVD.R:205-219).  Building the copy
// inside that call cost 50 ms of transposition plus the allocation of 100 GB (50 ms .. 1.8 s depending on the box) before
// the first pass could start.  Now a helper thread allocates and queues k_smaj_build on a low-priority stream of its own,
// behind an event that marks what the handle's stream had queued (the image itself: generation, upload, gather); the
// passes of the solve that would read the copy take k_prod<2> on the variant-major image until an event says it is
// complete — the same integer sums (tests/test_gpu_smaj.py) — and k_prodT from then on.
struct SmajJob {
  std::thread th;
  std::atomic<int> state{0};   // 0 the thread is allocating, 1 build queued (ev marks its end), 2 failed (no room / no memory)
  uint8_t *buf = nullptr;
  size_t bytes = 0;
  int64_t pitch_t = 0, rows_t = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev = nullptr, ev_img = nullptr;
};

static void smaj_job_finish(bsn_bed *b, bool adopt) {
  SmajJob *j = (SmajJob *)b->smaj_job;
  if (!j) return;
  if (j->th.joinable()) j->th.join();
  if (j->state.load() == 1) (void)hipEventSynchronize(j->ev);
  if (adopt && j->state.load() == 1 && !b->d_smaj) {
    b->d_smaj = j->buf;
    b->smaj_cap = j->bytes;
    b->pitch_smaj = j->pitch_t;
    b->rows_smaj = j->rows_t;
    j->buf = nullptr;
  }
  if (j->buf) (void)hipFree(j->buf);
  if (j->ev) (void)hipEventDestroy(j->ev);
  if (j->ev_img) (void)hipEventDestroy(j->ev_img);
  if (j->st) (void)hipStreamDestroy(j->st);
  delete j;
  b->smaj_job = nullptr;
}

void image_smaj_wait(bsn_bed *b) { smaj_job_finish(b, true); }

bool image_smaj_poll(bsn_bed *b) {
  if (b->d_smaj) return true;
  SmajJob *j = (SmajJob *)b->smaj_job;
  if (!j) return false;
  const int st = j->state.load(std::memory_order_acquire);
  if (st == 0) return false;
  if (st == 1 && hipEventQuery(j->ev) != hipSuccess) {
    (void)hipGetLastError();   // (hipErrorNotReady is not an error of this thread)
    return false;
  }
  smaj_job_finish(b, true);
  return b->d_smaj != nullptr;
}

bool image_smaj_start(bsn_bed *b) {
  if (b->d_smaj) return true;
  if (b->smaj_job) return ((SmajJob *)b->smaj_job)->state.load() != 2 || image_smaj_poll(b);
  if (b->streamed()) return false;
  if (b->smaj_tried || b->bits != 2 || getenv("BSN_NO_SMAJ")) return false;
  b->smaj_tried = true;
  BSN_HIP(hipSetDevice(b->device));
  const int64_t pitch_t = round_up((b->m + 3) / 4 + 128, 256), rows_t = round_up(b->n, 256);
  if (rows_t / 4 > b->pitch) return false;
  const size_t bytes = (size_t)rows_t * (size_t)pitch_t;
  if (!smaj_room(b, bytes)) return false;
  SmajJob *j = new SmajJob();
  j->bytes = bytes;
  j->pitch_t = pitch_t;
  j->rows_t = rows_t;
  try {
    int lo = 0, hi = 0;
    BSN_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));   // lo = least priority
    BSN_HIP(hipStreamCreateWithPriority(&j->st, hipStreamNonBlocking, lo));
    BSN_HIP(hipEventCreateWithFlags(&j->ev, hipEventDisableTiming));
    BSN_HIP(hipEventCreateWithFlags(&j->ev_img, hipEventDisableTiming));
    BSN_HIP(hipEventRecord(j->ev_img, b->stream));        // the image is complete behind this point of the handle's stream
  } catch (...) {
    if (j->ev) (void)hipEventDestroy(j->ev);
    if (j->ev_img) (void)hipEventDestroy(j->ev_img);
    if (j->st) (void)hipStreamDestroy(j->st);
    delete j;
    throw;
  }
  b->smaj_job = j;
  const int device = b->device;
  j->th = std::thread([b, j, device] {
    const auto t0 = std::chrono::steady_clock::now();
    bool ok = hipSetDevice(device) == hipSuccess && hipMalloc((void **)&j->buf, j->bytes) == hipSuccess;
    if (getenv("BSN_ALLOC_TRACE"))
      std::fprintf(stderr, "[bsn alloc] sample-major copy, helper thread: hipMalloc of %zu bytes %s after %.1f ms\n", j->bytes,
                   ok ? "returned" : "FAILED", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (ok) {
      ok = hipStreamWaitEvent(j->st, j->ev_img, 0) == hipSuccess;
      if (ok) {
        const int64_t nvb = j->pitch_t * 4 / 512;
        const int64_t gy = nvb < 65535 ? nvb : 65535, gz = (nvb + 65534) / 65535;
        hipLaunchKernelGGL(k_smaj_build, dim3((unsigned)(j->rows_t / 256), (unsigned)gy, (unsigned)gz), dim3(512), 0, j->st,
                           b->d_img, b->pitch, b->m, j->buf, j->pitch_t, j->rows_t);
        ok = hipGetLastError() == hipSuccess && hipEventRecord(j->ev, j->st) == hipSuccess;
      }
    }
    if (!ok) {
      (void)hipGetLastError();
      if (j->buf) (void)hipFree(j->buf);
      j->buf = nullptr;
    }
    j->state.store(ok ? 1 : 2, std::memory_order_release);
  });
  return true;
}

bool image_smaj(bsn_bed *b) {
  if (b->d_smaj) return true;
  if (b->smaj_job) {   // a build in flight: wait for it
    smaj_job_finish(b, true);
    return b->d_smaj != nullptr;
  }
  if (b->streamed()) return false;
  if (b->smaj_tried || b->bits != 2 || getenv("BSN_NO_SMAJ")) return false;
  b->smaj_tried = true;
  BSN_HIP(hipSetDevice(b->device));
  const int64_t pitch_t = round_up((b->m + 3) / 4 + 128, 256), rows_t = round_up(b->n, 256);
  if (rows_t / 4 > b->pitch) return false;   // (never: pitch = ceil(n / 4) rounded up to 256 B)
  const size_t bytes = (size_t)rows_t * (size_t)pitch_t;
  if (!smaj_room(b, bytes)) return false;
  if (hipMalloc((void **)&b->d_smaj, bytes) != hipSuccess) {
    (void)hipGetLastError();
    b->d_smaj = nullptr;
    return false;
  }
  b->smaj_cap = bytes;
  smaj_launch(b, pitch_t, rows_t);
  return true;
}

// the image changed in place (image_gather with `reuse`): an existing sample-major copy is rebuilt inside its
// allocation when it fits, dropped otherwise (the next solve asks for a new one)
static void smaj_refresh(bsn_bed *b) {
  image_smaj_wait(b);   // (a build in flight read the image that was just replaced: finish it, then rebuild inside its allocation)
  b->smaj_tried = false;
  if (!b->d_smaj) return;
  const int64_t pitch_t = round_up((b->m + 3) / 4 + 128, 256), rows_t = round_up(b->n, 256);
  if ((size_t)rows_t * (size_t)pitch_t <= b->smaj_cap) {
    smaj_launch(b, pitch_t, rows_t);
    return;
  }
  BSN_HIP(hipStreamSynchronize(b->stream));
  (void)hipFree(b->d_smaj);
  b->d_smaj = nullptr;
  b->smaj_cap = 0;
}

// recode = 1: the rows hold .bed codes (uploads); 0: device codes already (FBM repack)
static void finish_image(bsn_bed *b, int recode) {
  const int64_t gy = b->m < 65535 ? b->m : 65535, gz = (b->m + 65534) / 65535;
  hipLaunchKernelGGL(k_recode_fix, dim3((unsigned)((b->pitch / 16 + 255) / 256), (unsigned)gy, (unsigned)gz),
                     dim3(256), 0, b->stream, b->d_img, b->pitch, b->n, b->n_byte, b->m, recode);
  BSN_HIP(hipGetLastError());
  BSN_HIP(hipMemsetAsync(b->d_img + b->m * b->pitch, 0, (size_t)(kPadRows * b->pitch), b->stream));
}

void image_from_host(bsn_bed *b, const uint8_t *payload, int64_t n_byte_src) {
  b->forget_counts();
  // Column chunks keep each 2-D copy below 1 GiB so that pageable (mmap'd) sources are
  // staged piecewise by the runtime.
  int64_t rows_per = (int64_t)((1ull << 30) / (size_t)n_byte_src);
  if (rows_per < 1) rows_per = 1;
  for (int64_t j = 0; j < b->m; j += rows_per) {
    int64_t cnt = (b->m - j < rows_per) ? b->m - j : rows_per;
    BSN_HIP(hipMemcpy2DAsync(b->d_img + j * b->pitch, (size_t)b->pitch, payload + j * n_byte_src,
                             (size_t)n_byte_src, (size_t)b->n_byte, (size_t)cnt,
                             hipMemcpyHostToDevice, b->stream));
  }
  finish_image(b, 1);
  BSN_HIP(hipStreamSynchronize(b->stream));
}

// Upload straight from the file: copying out of a page-cache mapping faults one 4-KiB page at a
// time (4.8 GB/s measured); instead a few threads pread() slices of a 256-MiB column chunk into
// one of two pinned buffers while the other one is on its way to the device (DMA, 2-D copy
// into the padded pitch).
FileStage::~FileStage() {
  for (int i = 0; i < 2; i++) {
    if (pin[i]) (void)hipHostFree(pin[i]);
    if (done[i]) (void)hipEventDestroy(done[i]);
  }
}

void image_from_file(bsn_bed *b, int fd, int64_t offset, int64_t n_byte_src, FileStage *stage) {
  b->forget_counts();
  const int64_t chunk_bytes = 256ll << 20;
  int64_t cols_per = chunk_bytes / n_byte_src;
  if (cols_per < 1) cols_per = 1;
  FileStage own;
  FileStage &fs = stage ? *stage : own;
  if (fs.bytes < (size_t)(cols_per * n_byte_src)) {
    for (int i = 0; i < 2; i++) {
      if (fs.pin[i]) (void)hipHostFree(fs.pin[i]);
      fs.pin[i] = nullptr;
      BSN_HIP(hipHostMalloc((void **)&fs.pin[i], (size_t)(cols_per * n_byte_src), hipHostMallocDefault));
      if (!fs.done[i]) BSN_HIP(hipEventCreateWithFlags(&fs.done[i], hipEventDisableTiming));
    }
    fs.bytes = (size_t)(cols_per * n_byte_src);
  }
  uint8_t **pin = fs.pin;
  hipEvent_t *done = fs.done;
  unsigned hw = std::thread::hardware_concurrency();
  const int nthr = (int)std::max(1u, std::min(16u, hw ? hw / 2 : 4u));
  int k = 0;
  for (int64_t j = 0; j < b->m; j += cols_per, k++) {
    const int64_t cnt = std::min(cols_per, b->m - j);
    const int64_t bytes = cnt * n_byte_src, base = offset + j * n_byte_src;
    uint8_t *dst = pin[k & 1];
    if (k >= 2) BSN_HIP(hipEventSynchronize(done[k & 1]));  // its previous upload has left the buffer
    std::atomic<int> bad{0};
    std::vector<std::thread> th;
    const int64_t slice = (bytes + nthr - 1) / nthr;
    for (int t = 0; t < nthr; t++) {
      const int64_t lo = (int64_t)t * slice, hi = std::min(bytes, lo + slice);
      if (lo >= hi) break;
      th.emplace_back([=, &bad] {
        int64_t pos = lo;
        while (pos < hi) {
          ssize_t r = pread(fd, dst + pos, (size_t)(hi - pos), (off_t)(base + pos));
          if (r <= 0) {
            bad = 1;
            return;
          }
          pos += r;
        }
      });
    }
    for (auto &t : th) t.join();
    if (bad) fail("Error when mapping file:\n  %s.\n", "short read");
    BSN_HIP(hipMemcpy2DAsync(b->d_img + j * b->pitch, (size_t)b->pitch, dst, (size_t)n_byte_src,
                             (size_t)b->n_byte, (size_t)cnt, hipMemcpyHostToDevice, b->stream));
    BSN_HIP(hipEventRecord(done[k & 1], b->stream));
  }
  finish_image(b, 1);
  BSN_HIP(hipStreamSynchronize(b->stream));
}

// ---------------------------------------------------------------------------
// FBM.code256 bytes -> device image through a 256-entry byte look-up.
// 2-bit image: lut[byte] = device code 0..3 (four source bytes per image byte).
__global__ void k_pack_fbm(const uint8_t *src, int64_t ld, int64_t n, int64_t n_byte, uint8_t *img,
                           int64_t pitch, int64_t ncols, const uint8_t *__restrict__ lut) {
  __shared__ uint8_t sl[256];
  sl[threadIdx.x & 255] = lut[threadIdx.x & 255];
  __syncthreads();
  int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t j = blockIdx.y;
  if (b >= n_byte || j >= ncols) return;
  const uint8_t *col = src + j * ld;
  uint32_t out = 0;
  for (int e = 0; e < 4; e++) {
    int64_t i = b * 4 + e;
    uint32_t code = 0;
    if (i < n) code = sl[col[i]];
    out |= code << (2 * e);
  }
  img[j * pitch + b] = (uint8_t)out;
}
// byte image: lut[byte] = grid index k as int8, 0x80 for a missing value; pad samples 0
__global__ void k_pack_fbm8(const uint8_t *src, int64_t ld, int64_t n, uint8_t *img, int64_t pitch,
                            int64_t ncols, const uint8_t *__restrict__ lut) {
  __shared__ uint8_t sl[256];
  sl[threadIdx.x & 255] = lut[threadIdx.x & 255];
  __syncthreads();
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t j = blockIdx.y;
  if (i >= pitch || j >= ncols) return;
  img[j * pitch + i] = i < n ? sl[src[j * ld + i]] : (uint8_t)0;
}

// Column chunks of the host matrix go through two pinned buffers (filled by a few threads, the
// source may be a page-cache mapping of a .bk file) while the previous chunk is on its way to the
// device and being packed — the same pipeline as image_from_file.
void image_from_fbm(bsn_bed *b, const uint8_t *bytes, int64_t ld, const uint8_t *lut) {
  const int64_t chunk_bytes = 256ll << 20;
  int64_t cols_per = chunk_bytes / ld;
  if (cols_per < 1) cols_per = 1;
  if (cols_per > 65535) cols_per = 65535;
  uint8_t *pin[2] = {nullptr, nullptr};
  hipEvent_t done[2];
  struct Cleanup {
    uint8_t **pin;
    hipEvent_t *ev;
    int nev = 0;
    ~Cleanup() {
      for (int i = 0; i < 2; i++)
        if (pin[i]) (void)hipHostFree(pin[i]);
      for (int i = 0; i < nev; i++) (void)hipEventDestroy(ev[i]);
    }
  } cleanup{pin, done};
  for (int i = 0; i < 2; i++) {
    BSN_HIP(hipHostMalloc((void **)&pin[i], (size_t)(cols_per * ld), hipHostMallocDefault));
    BSN_HIP(hipEventCreateWithFlags(&done[i], hipEventDisableTiming));
    cleanup.nev = i + 1;
  }
  DevBuf<uint8_t> tmp[2], d_lut;
  tmp[0].ensure((size_t)cols_per * (size_t)ld);
  tmp[1].ensure((size_t)cols_per * (size_t)ld);
  BSN_HIP(hipMemcpy(d_lut.ensure(256), lut, 256, hipMemcpyHostToDevice));
  unsigned hw = std::thread::hardware_concurrency();
  const int nthr = (int)std::max(1u, std::min(16u, hw ? hw / 2 : 4u));
  int k = 0;
  for (int64_t j = 0; j < b->m; j += cols_per, k++) {
    const int64_t cnt = std::min(cols_per, b->m - j);
    const int64_t total = cnt * ld;
    uint8_t *dst = pin[k & 1];
    if (k >= 2) BSN_HIP(hipEventSynchronize(done[k & 1]));  // its previous chunk has been packed
    std::vector<std::thread> th;
    const int64_t slice = (total + nthr - 1) / nthr;
    for (int t = 0; t < nthr; t++) {
      const int64_t lo = (int64_t)t * slice, hi = std::min(total, lo + slice);
      if (lo >= hi) break;
      th.emplace_back([=] { std::memcpy(dst + lo, bytes + j * ld + lo, (size_t)(hi - lo)); });
    }
    for (auto &t : th) t.join();
    BSN_HIP(hipMemcpyAsync(tmp[k & 1].p, dst, (size_t)total, hipMemcpyHostToDevice, b->stream));
    if (b->bits == 8) {
      dim3 grid((unsigned)((b->pitch + 255) / 256), (unsigned)cnt);
      hipLaunchKernelGGL(k_pack_fbm8, grid, dim3(256), 0, b->stream, tmp[k & 1].p, ld, b->n,
                         b->d_img + j * b->pitch, b->pitch, cnt, d_lut.p);
    } else {
      dim3 grid((unsigned)((b->n_byte + 255) / 256), (unsigned)cnt);
      hipLaunchKernelGGL(k_pack_fbm, grid, dim3(256), 0, b->stream, tmp[k & 1].p, ld, b->n, b->n_byte,
                         b->d_img + j * b->pitch, b->pitch, cnt, d_lut.p);
    }
    BSN_HIP(hipGetLastError());
    BSN_HIP(hipEventRecord(done[k & 1], b->stream));
  }
  if (b->bits == 8)
    BSN_HIP(hipMemsetAsync(b->d_img + b->m * b->pitch, 0, (size_t)(kPadRows * b->pitch), b->stream));
  else
    finish_image(b, 0);
  BSN_HIP(hipStreamSynchronize(b->stream));
}

// ---- byte image statistics -----------------------------------------------------------------
// value plane of a register of four int8 grid indices: missing (0x80) -> 0; `na` gets 1 per missing byte
__device__ __forceinline__ uint32_t val8(uint32_t w, uint32_t &na) {
  const uint32_t t = w ^ 0x80808080u;
  const uint32_t y = (t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;   // bit 7 set iff the low 7 bits are non-zero
  const uint32_t z = ~(y | t | 0x7F7F7F7Fu);             // 0x80 iff the byte of w is 0x80
  na = z >> 7;
  return w & ~(z | (z - na));                            // per byte 0x80 | 0x7F: no borrow across bytes
}
__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int c) {
  int s = c;
#pragma unroll
  for (int e = 0; e < 4; e++) s += (int)(int8_t)(a >> (8 * e)) * (int)(int8_t)(b >> (8 * e));
  return s;
}
// one wave per variant, all file rows, 16 B per lane per iteration
__global__ __launch_bounds__(256) void k_stats8(const uint8_t *img, int64_t pitch, const int32_t *cols,
                                                int64_t col0, int64_t m, long long *out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + wave;
  if (j >= m) return;
  const int64_t col = cols ? (int64_t)cols[j] : col0 + j;
  const uint4 *row = (const uint4 *)(img + col * pitch);
  long long s1 = 0, s2 = 0;
  int nna = 0;
  for (int64_t t = lane; t < pitch / 16; t += 64) {
    const uint4 v = row[t];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    int a1 = 0, a2 = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      uint32_t na;
      const uint32_t x = val8(w[q], na);
      a1 = dot4(x, 0x01010101u, a1);
      a2 = dot4(x, x, a2);
      nna += __popc(na);
    }
    s1 += a1;
    s2 += a2;
  }
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_down(s1, off);
    s2 += __shfl_down(s2, off);
    nna += __shfl_down(nna, off);
  }
  if (lane == 0) {
    out[3 * j + 0] = s1;
    out[3 * j + 1] = s2;
    out[3 * j + 2] = nna;
  }
}
// row list (any order, duplicates count as often as they occur): one wave per variant, byte gathers
__global__ __launch_bounds__(256) void k_stats8_rows(const uint8_t *img, int64_t pitch, const int32_t *rows,
                                                     int64_t n, const int32_t *cols, int64_t col0, int64_t m,
                                                     long long *out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + wave;
  if (j >= m) return;
  const int64_t col = cols ? (int64_t)cols[j] : col0 + j;
  const int8_t *row = (const int8_t *)(img + col * pitch);
  long long s1 = 0, s2 = 0;
  int nna = 0;
  for (int64_t i = lane; i < n; i += 64) {
    const int k = row[rows[i]];
    if (k == -128) nna++;
    else {
      s1 += k;
      s2 += k * k;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_down(s1, off);
    s2 += __shfl_down(s2, off);
    nna += __shfl_down(nna, off);
  }
  if (lane == 0) {
    out[3 * j + 0] = s1;
    out[3 * j + 1] = s2;
    out[3 * j + 2] = nna;
  }
}
void stats8(bsn_bed *b, const int32_t *d_rows, int64_t n, const int32_t *d_cols, int64_t col0, int64_t m,
            long long *d_out) {
  refuse_generic(b, "this function");
  if (d_rows)
    hipLaunchKernelGGL(k_stats8_rows, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, b->stream, b->d_img, b->pitch,
                       d_rows, n, d_cols, col0, m, d_out);
  else
    hipLaunchKernelGGL(k_stats8, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, b->stream, b->d_img, b->pitch, d_cols,
                       col0, m, d_out);
  BSN_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Generic decode table (bsn_bed::generic): value = lut[byte], any 256 doubles (src/colstats.cpp:13-14,
// R/bigSNP-class.R:7-13).  No integer image exists, so these are plain fp64 kernels: one look-up (LDS), one FMA
// per genotype — VALU-bound at a fraction of the streaming rate, but no table is refused.  A NaN entry
// (missing code) propagates like NA_real does through the reference's accessor.
void refuse_generic(const bsn_bed *b, const char *what) {
  if (b->generic)
    fail("%s is not available for this FBM.code256: its decode table is neither genotype calls (0, 1, 2, NA) nor a "
         "regular grid (like CODE_DOSAGE); snp_colstats / snp_MAF / snp_scale*, big_prodVec and big_cprodVec are",
         what);
}
// one wave per variant: out[2 j] = sum v, out[2 j + 1] = sum v^2 over the selected rows (fixed order)
__global__ __launch_bounds__(256) void k_lut_colstats(const uint8_t *__restrict__ img, int64_t pitch,
                                                      const double *__restrict__ lut, const int32_t *rows, int64_t n,
                                                      const int32_t *cols, int64_t col0, int64_t m, double *out) {
  __shared__ double sl[256];
  sl[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= m) return;
  const uint8_t *row = img + (cols ? (int64_t)cols[j] : col0 + j) * pitch;
  double s1 = 0, s2 = 0;
  for (int64_t i = lane; i < n; i += 64) {
    const double v = sl[row[rows ? rows[i] : i]];
    s1 += v;
    s2 += v * v;
  }
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_down(s1, off);
    s2 += __shfl_down(s2, off);
  }
  if (lane == 0) {
    out[2 * j] = s1;
    out[2 * j + 1] = s2;
  }
}
void lut_colstats(bsn_bed *b, const int32_t *d_rows, int64_t n, const int32_t *d_cols, int64_t col0, int64_t m,
                  double *d_out) {
  hipLaunchKernelGGL(k_lut_colstats, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, b->stream, b->d_img, b->pitch,
                     b->d_lut, d_rows, n, d_cols, col0, m, d_out);
  BSN_HIP(hipGetLastError());
}
// one wave per variant: z[j] = (sum_i v_ij x_i - c_j sum_i x_i) / s_j
__global__ __launch_bounds__(256) void k_lut_cprod(const uint8_t *__restrict__ img, int64_t pitch,
                                                   const double *__restrict__ lut, const int32_t *rows, int64_t n,
                                                   const int32_t *cols, int64_t col0, int64_t m,
                                                   const double *center, const double *scale,
                                                   const double *__restrict__ x, double *z) {
  __shared__ double sl[256];
  sl[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= m) return;
  const uint8_t *row = img + (cols ? (int64_t)cols[j] : col0 + j) * pitch;
  double s = 0, sx = 0;
  for (int64_t i = lane; i < n; i += 64) {
    const double xi = x[i];
    s += sl[row[rows ? rows[i] : i]] * xi;
    sx += xi;
  }
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off);
    sx += __shfl_down(sx, off);
  }
  if (lane == 0) z[j] = (s - (center ? center[j] : 0.0) * sx) / (scale ? scale[j] : 1.0);
}
void lut_cprod(bsn_bed *b, const int32_t *d_rows, int64_t n, const int32_t *d_cols, int64_t col0, int64_t m,
               const double *d_center, const double *d_scale, const double *d_x, double *d_z) {
  hipLaunchKernelGGL(k_lut_cprod, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, b->stream, b->d_img, b->pitch,
                     b->d_lut, d_rows, n, d_cols, col0, m, d_center, d_scale, d_x, d_z);
  BSN_HIP(hipGetLastError());
}
// one thread per selected row and slab of variants: part[slab][i] = sum_j (v_ij - c_j) x_j / s_j over the slab
__global__ __launch_bounds__(256) void k_lut_prod(const uint8_t *__restrict__ img, int64_t pitch,
                                                  const double *__restrict__ lut, const int32_t *rows, int64_t n,
                                                  const int32_t *cols, int64_t col0, int64_t m, int64_t per_slab,
                                                  const double *center, const double *scale,
                                                  const double *__restrict__ x, double *part) {
  __shared__ double sl[256];
  sl[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t ri = rows ? rows[i] : i;
  const int64_t j0 = (int64_t)blockIdx.y * per_slab, j1 = j0 + per_slab < m ? j0 + per_slab : m;
  double s = 0;
  for (int64_t j = j0; j < j1; j++) {
    const double w = x[j] / (scale ? scale[j] : 1.0);
    s += (sl[img[(cols ? (int64_t)cols[j] : col0 + j) * pitch + ri]] - (center ? center[j] : 0.0)) * w;
  }
  part[(int64_t)blockIdx.y * n + i] = s;
}
__global__ void k_lut_prod_sum(const double *part, int nslab, int64_t n, double *y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0;
  for (int k = 0; k < nslab; k++) s += part[(int64_t)k * n + i];   // slab order: deterministic
  y[i] = s;
}
void lut_prod(bsn_bed *b, const int32_t *d_rows, int64_t n, const int32_t *d_cols, int64_t col0, int64_t m,
              const double *d_center, const double *d_scale, const double *d_x, double *d_y) {
  const int64_t wg = (n + 255) / 256;
  int64_t nslab = std::max<int64_t>(1, std::min<int64_t>(4096 / wg, (m + 63) / 64));
  const int64_t per = (m + nslab - 1) / nslab;
  nslab = (m + per - 1) / per;
  DevBuf<double> part;
  part.ensure((size_t)nslab * (size_t)n);
  hipLaunchKernelGGL(k_lut_prod, dim3((unsigned)wg, (unsigned)nslab), dim3(256), 0, b->stream, b->d_img, b->pitch,
                     b->d_lut, d_rows, n, d_cols, col0, m, per, d_center, d_scale, d_x, part.p);
  hipLaunchKernelGGL(k_lut_prod_sum, dim3((unsigned)wg), dim3(256), 0, b->stream, part.p, (int)nslab, n, d_y);
  BSN_HIP(hipGetLastError());
  BSN_HIP(hipStreamSynchronize(b->stream));   // `part` is released on return
}

// ---------------------------------------------------------------------------
// Synthetic generator — must stay bit-identical to oracle/bsn_oracle.c:orc_fake_bed.
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t gen_pop(uint32_t seed, uint32_t i, uint32_t npop) {
  uint32_t u = mix32(i * 0x9E3779B1U + mix32(seed ^ 0xA5A5A5A5U)) >> 8;
  uint32_t u2 = (uint32_t)(((uint64_t)u * u) >> 24);
  return (uint32_t)(((uint64_t)u2 * npop) >> 24);
}
__device__ __forceinline__ uint32_t gen_freq16(uint32_t seed, uint32_t j, uint32_t k) {
  uint32_t hj = mix32(j * 0x85EBCA6BU + mix32(seed ^ 0x3C6EF372U));
  int32_t p = 3277 + (int32_t)(((hj & 0xFFFF) * 29491U) >> 16);
  uint32_t hk = mix32(hj + (k + 1) * 0xC2B2AE35U);
  int32_t amp = 1311 + 393 * (int32_t)(k % 24);
  int32_t dev = (int32_t)(((int64_t)((int32_t)(hk & 0xFFFF) - 32768) * amp) >> 15);
  p += dev;
  if (p < 655) p = 655;
  if (p > 64880) p = 64880;
  return (uint32_t)p;
}
__device__ __forceinline__ uint32_t gen_code(uint32_t seed, uint32_t i, uint32_t j, uint32_t p16,
                                             uint32_t na16) {
  uint32_t r = mix32(i * 0x9E3779B1U + mix32(j * 0x85EBCA6BU + seed));
  uint32_t r2 = mix32(r ^ 0x68E31DA4U);
  if ((r2 & 0xFFFF) < na16) return 3;  // device code of a missing value
  return ((r & 0xFFFF) < p16) + ((r >> 16) < p16);
}

// one thread = one dword (16 samples) of one variant
__global__ void k_generate(uint8_t *img, int64_t pitch, int64_t n, int64_t m, uint32_t seed,
                           uint32_t npop, uint32_t na16, int64_t j_begin) {
  int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t j = blockIdx.y + (int64_t)blockIdx.z * 65535;
  if (d * 4 >= pitch || j >= m) return;
  uint32_t jj = (uint32_t)(j + j_begin);
  uint32_t out = 0;
  for (int e = 0; e < 16; e++) {
    int64_t i = d * 16 + e;
    uint32_t code = 0;
    if (i < n) {
      uint32_t k = gen_pop(seed, (uint32_t)i, npop);
      code = gen_code(seed, (uint32_t)i, jj, gen_freq16(seed, jj, k), na16);
    }
    out |= code << (2 * e);
  }
  *(uint32_t *)(img + j * pitch + d * 4) = out;
}

void image_generate(bsn_bed *b, uint32_t seed, uint32_t npop, uint32_t na16, int64_t j_begin) {
  b->forget_counts();
  int64_t dwords = b->pitch / 4;
  int64_t gy = b->m < 65535 ? b->m : 65535;
  int64_t gz = (b->m + 65534) / 65535;
  dim3 grid((unsigned)((dwords + 255) / 256), (unsigned)gy, (unsigned)gz);
  hipLaunchKernelGGL(k_generate, grid, dim3(256), 0, b->stream, b->d_img, b->pitch, b->n, b->m,
                     seed, npop, na16, j_begin);
  BSN_HIP(hipGetLastError());
  // pad rows only (pad samples were already written as 0 above)
  BSN_HIP(hipMemsetAsync(b->d_img + b->m * b->pitch, 0, (size_t)(kPadRows * b->pitch), b->stream));
  BSN_HIP(hipStreamSynchronize(b->stream));
}

// back to .bed payload layout; pad bits of the last byte are written as 0 like PLINK does
__global__ void k_unpad(const uint8_t *img, int64_t pitch, int64_t n, int64_t n_byte,
                        uint8_t *out) {
  int64_t j = blockIdx.y + (int64_t)blockIdx.z * 65535;
  int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_byte) return;
  uint8_t v = (uint8_t)plink_from_dev(img[j * pitch + b]);
  int rem = (int)(n & 3);
  if (rem && b == n_byte - 1) v &= (uint8_t)((1u << (2 * rem)) - 1);
  out[j * n_byte + b] = v;
}

void image_download(bsn_bed *b, uint8_t *payload_out) {
  require_bits(b, 2, "the .bed payload download");
  int64_t rows_per = (int64_t)((256ull << 20) / (size_t)b->n_byte);
  if (rows_per < 1) rows_per = 1;
  if (rows_per > 65535) rows_per = 65535;
  DevBuf<uint8_t> tmp;
  tmp.ensure((size_t)rows_per * (size_t)b->n_byte);
  for (int64_t j = 0; j < b->m; j += rows_per) {
    int64_t cnt = (b->m - j < rows_per) ? b->m - j : rows_per;
    dim3 grid((unsigned)((b->n_byte + 255) / 256), (unsigned)cnt, 1);
    hipLaunchKernelGGL(k_unpad, grid, dim3(256), 0, b->stream, b->d_img + j * b->pitch, b->pitch,
                       b->n, b->n_byte, tmp.p);
    BSN_HIP(hipGetLastError());
    copy_d2h(b, payload_out + j * b->n_byte, tmp.p, (size_t)cnt * (size_t)b->n_byte);
    BSN_HIP(hipStreamSynchronize(b->stream));
  }
}

// ---------------------------------------------------------------------------
// Per-variant counts of the four codes over ALL file rows: one wave per variant,
// 16 B per lane per iteration, popcount on the 2-bit planes.  HBM-bound, pure
// integer; replaces the element loop of src/bed-fun.cpp:51-69.
__global__ __launch_bounds__(256) void k_counts(const uint8_t *img, int64_t pitch,
                                                const int32_t *cols, int64_t col0, int64_t m,
                                                int64_t n_pad_samples, int32_t *counts) {
  int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int64_t j = (int64_t)blockIdx.x * 4 + wave;
  if (j >= m) return;
  int64_t col = cols ? (int64_t)cols[j] : col0 + j;
  const uint4 *row = (const uint4 *)(img + col * pitch);
  int64_t nvec = pitch / 16;
  uint32_t c1 = 0, c2 = 0, c3 = 0;
  for (int64_t t = lane; t < nvec; t += 64) {
    uint4 v = row[t];
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; q++) {
      uint32_t lo = w[q] & 0x55555555u, hi = (w[q] >> 1) & 0x55555555u;
      c3 += __popc(lo & hi);   // 0b11 -> missing
      c1 += __popc(lo & ~hi);  // 0b01 -> genotype 1
      c2 += __popc(hi & ~lo);  // 0b10 -> genotype 2
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    c1 += __shfl_down(c1, off);
    c2 += __shfl_down(c2, off);
    c3 += __shfl_down(c3, off);
  }
  if (lane == 0) {
    int64_t total = pitch * 4;
    counts[4 * j + 0] = (int32_t)(total - c1 - c2 - c3 - n_pad_samples);  // pad samples are code 0
    counts[4 * j + 1] = (int32_t)c1;
    counts[4 * j + 2] = (int32_t)c2;
    counts[4 * j + 3] = (int32_t)c3;
  }
}

void counts_all_rows(bsn_bed *b, const int32_t *d_cols, int64_t col0, int64_t m,
                     int32_t *d_counts) {
  require_bits(b, 2, "bed_counts");
  hipLaunchKernelGGL(k_counts, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, b->stream, b->d_img,
                     b->pitch, d_cols, col0, m, b->pitch * 4 - b->n, d_counts);
  BSN_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Dense read-back (src/bed-mat-acc.cpp:8-49): the test ground truth and the block
// loader of bed_tcrossprodSelf.
__global__ void k_read_dense(const uint8_t *img, int64_t pitch, const int32_t *rows, int64_t n,
                             const int32_t *cols, int64_t m, const double *center,
                             const double *scale, int32_t na_val, int32_t *out_i, double *out_d) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t j = blockIdx.y + (int64_t)blockIdx.z * 65535;
  if (i >= n || j >= m) return;
  int64_t i2 = rows ? rows[i] : i, j2 = cols ? cols[j] : j;
  uint32_t code = (img[j2 * pitch + (i2 >> 2)] >> (2 * (i2 & 3))) & 3;
  int g = code == 3 ? -1 : (int)code;
  if (out_i) out_i[i + j * n] = g < 0 ? na_val : g;
  if (out_d) out_d[i + j * n] = g < 0 ? 0.0 : ((double)g - center[j]) / scale[j];
}

void read_dense(bsn_bed *b, const int32_t *d_rows, int64_t n, const int32_t *d_cols, int64_t m,
                const double *d_center, const double *d_scale, int32_t na_val, int32_t *d_out_i,
                double *d_out_d) {
  require_bits(b, 2, "read_bed");
  int64_t gy = m < 65535 ? m : 65535, gz = (m + 65534) / 65535;
  dim3 grid((unsigned)((n + 255) / 256), (unsigned)gy, (unsigned)gz);
  hipLaunchKernelGGL(k_read_dense, grid, dim3(256), 0, b->stream, b->d_img, b->pitch, d_rows, n,
                     d_cols, m, d_center, d_scale, na_val, d_out_i, d_out_d);
  BSN_HIP(hipGetLastError());
}


// ---------------------------------------------------------------------------
// .bed <-> FBM.code256 conversions (src/read-plink.cpp:13-80, src/write-plink.cpp:13-52).
// bytes out: decoded genotype 0/1/2 and 3 for missing, one byte each, column-major n x m
__global__ void k_to_bytes(const uint8_t *img, int64_t pitch, const int32_t *rows, int64_t n,
                           const int32_t *cols, int64_t m, uint8_t *out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t j = blockIdx.y + (int64_t)blockIdx.z * 65535;
  if (i >= n || j >= m) return;
  int64_t i2 = rows ? rows[i] : i, j2 = cols ? cols[j] : j;
  uint32_t code = (img[j2 * pitch + (i2 >> 2)] >> (2 * (i2 & 3))) & 3;
  out[i + j * n] = (uint8_t)code;  // the device code is the CODE_012 byte
}

// readbina (src/read-plink.cpp:13-56): every byte of the .bed payload goes through the caller's 4 x 256 table
// (tab[4 * byte + e] = FBM byte of genotype e of that .bed byte; getCode() in R/utils.R:21-31), whole matrix, no
// subsets.  One thread per payload byte: device code -> PLINK byte -> four table bytes.
__global__ __launch_bounds__(256) void k_readbina(const uint8_t *__restrict__ img, int64_t pitch, int64_t n,
                                                  int64_t m, const uint8_t *__restrict__ tab,
                                                  uint8_t *__restrict__ out) {
  __shared__ uint32_t stab[256];
  stab[threadIdx.x] = ((const uint32_t *)tab)[threadIdx.x];
  __syncthreads();
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t j = blockIdx.y + (int64_t)blockIdx.z * 65535;
  if (4 * b >= n || j >= m) return;
  const int64_t left = n - 4 * b;
  // the pad genotypes of a variant's last byte are 00 in a .bed file (the image holds them as genotype 0): the table
  // is indexed with the byte as PLINK writes it
  const uint32_t keep = left >= 4 ? 0xFFu : (1u << (2 * left)) - 1u;
  const uint32_t t = stab[plink_from_dev(img[j * pitch + b]) & keep];
  uint8_t *o = out + j * n + 4 * b;
  if (left >= 4 && (((uintptr_t)o) & 3) == 0) {
    *(uint32_t *)o = t;
  } else {
    for (int e = 0; e < 4 && e < left; e++) o[e] = (uint8_t)(t >> (8 * e));
  }
}

// packed .bed payload of the sub-matrix [rows, cols]: ceil(n/4) bytes per variant, pad bits 0
__global__ void k_subset_pack(const uint8_t *img, int64_t pitch, const int32_t *rows, int64_t n,
                              const int32_t *cols, int64_t m, int64_t n_byte_out, uint8_t *out) {
  int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t j = blockIdx.y + (int64_t)blockIdx.z * 65535;
  if (b >= n_byte_out || j >= m) return;
  int64_t j2 = cols ? cols[j] : j;
  uint32_t v = 0, keep = 0;
  for (int e = 0; e < 4; e++) {
    int64_t i = b * 4 + e;
    if (i < n) {
      int64_t i2 = rows ? rows[i] : i;
      v |= ((img[j2 * pitch + (i2 >> 2)] >> (2 * (i2 & 3))) & 3u) << (2 * e);
      keep |= 3u << (2 * e);
    }
  }
  out[j * n_byte_out + b] = (uint8_t)(plink_from_dev(v) & keep);
}

// ---------------------------------------------------------------------------
// A gathered copy of the image: sample i of the copy is sample rows[i] of the source (any order, repeats
// allowed), variant j is variant cols[j]; same coding, pad samples 0.  One thread per output byte.
__global__ void k_gather_image(const uint8_t *img, int64_t pitch, int bits, const int32_t *rows, int64_t n,
                               const int32_t *cols, int64_t m, uint8_t *out, int64_t pitch_out) {
  int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t j = blockIdx.y + (int64_t)blockIdx.z * 65535;
  if (b >= pitch_out || j >= m) return;
  const uint8_t *col = img + (int64_t)cols[j] * pitch;
  uint32_t v = 0;
  if (bits == 8) {
    if (b < n) v = col[rows[b]];
  } else {
    for (int e = 0; e < 4; e++) {
      const int64_t i = b * 4 + e;
      if (i < n) {
        const int64_t i2 = rows[i];
        v |= ((col[i2 >> 2] >> (2 * (i2 & 3))) & 3u) << (2 * e);
      }
    }
  }
  out[j * pitch_out + b] = (uint8_t)v;
}

// all samples in file order: a variant row of the copy IS a variant row of the source (16-byte copies, one
// workgroup row per variant)
__global__ void k_copy_rows(const uint8_t *__restrict__ img, int64_t pitch, const int32_t *__restrict__ cols, int64_t m,
                            uint8_t *__restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t j = blockIdx.y + (int64_t)blockIdx.z * 65535;
  if (q * 16 >= pitch || j >= m) return;
  ((uint4 *)(out + j * pitch))[q] = ((const uint4 *)(img + (int64_t)cols[j] * pitch))[q];
}

bsn_bed *image_gather(bsn_bed *src, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, bsn_bed *reuse) {
  if (n <= 0 || m <= 0) fail("'ind.row' and 'ind.col' can't be empty.");
  if (src->generic) fail("internal: image_gather on a look-up image");
  require_resident(src, "a row list with repeated samples");
  BSN_HIP(hipSetDevice(src->device));
  std::vector<int32_t> rows((size_t)n), cols((size_t)m);
  for (int64_t i = 0; i < n; i++) {
    const int64_t r = ind_row ? ind_row[i] : i;
    if (r < 0 || r >= src->n) fail("Tested %lld < %lld. Subscript out of bounds (ind.row).", (long long)r, (long long)src->n);
    rows[(size_t)i] = (int32_t)r;
  }
  for (int64_t j = 0; j < m; j++) {
    const int64_t c = ind_col ? ind_col[j] : j;
    if (c < 0 || c >= src->m) fail("Tested %lld < %lld. Subscript out of bounds (ind.col).", (long long)c, (long long)src->m);
    cols[(size_t)j] = (int32_t)c;
  }
  bool rows_ident = n == src->n;
  for (int64_t i = 0; rows_ident && i < n; i++) rows_ident = rows[(size_t)i] == (int32_t)i;
  const bool in_place = reuse && reuse->n == n && reuse->bits == src->bits && reuse->cap_m >= m && reuse->d_img;
  std::unique_ptr<bsn_bed, void (*)(bsn_bed *)> fresh(nullptr, bed_free);
  bsn_bed *b = reuse;
  if (in_place) {
    image_smaj_wait(b);   // a background build of the copy still reads the selection that is about to be overwritten
    BSN_HIP(hipStreamSynchronize(b->stream));
    b->m = m;
    b->na_cnt.clear();
    b->forget_counts();
    b->na_blocks_state = 0;   // (the share of K-steps without a missing code is the old selection's)
  } else {
    fresh.reset(new bsn_bed());
    b = fresh.get();
    image_alloc(b, n, m, src->bits);
  }
  b->v_off = src->v_off;
  b->v_step = src->v_step;
  DevBuf<int32_t> d_rows, d_cols;
  BSN_HIP(hipStreamSynchronize(src->stream));   // whatever still writes the source image
  // the index lists go through the new handle's pinned staging buffers (no blocking copy from pageable memory)
  if (!rows_ident) copy_h2d(b, d_rows.ensure((size_t)n), rows.data(), (size_t)n * 4);
  copy_h2d(b, d_cols.ensure((size_t)m), cols.data(), (size_t)m * 4);
  BSN_HIP(hipMemsetAsync(b->d_img + b->m * b->pitch, 0, (size_t)(kPadRows * b->pitch), b->stream));
  const int64_t gy = m < 65535 ? m : 65535, gz = (m + 65534) / 65535;
  if (rows_ident && b->pitch == src->pitch)
    hipLaunchKernelGGL(k_copy_rows, dim3((unsigned)((b->pitch / 16 + 255) / 256), (unsigned)gy, (unsigned)gz), dim3(256), 0,
                       b->stream, src->d_img, src->pitch, d_cols.p, m, b->d_img);
  else
    hipLaunchKernelGGL(k_gather_image, dim3((unsigned)((b->pitch + 255) / 256), (unsigned)gy, (unsigned)gz), dim3(256), 0,
                       b->stream, src->d_img, src->pitch, src->bits, d_rows.p, n, d_cols.p, m, b->d_img, b->pitch);
  BSN_HIP(hipGetLastError());
  if (in_place) {
    smaj_refresh(b);
    tiled_refresh(b);
  }
  BSN_HIP(hipStreamSynchronize(b->stream));
  if (in_place) return b;
  return fresh.release();
}

void to_bytes(bsn_bed *b, const int32_t *d_rows, int64_t n, const int32_t *d_cols, int64_t m,
              uint8_t *d_out) {
  require_bits(b, 2, "readbina2");
  require_resident(b, "readbina2");
  int64_t gy = m < 65535 ? m : 65535, gz = (m + 65534) / 65535;
  hipLaunchKernelGGL(k_to_bytes, dim3((unsigned)((n + 255) / 256), (unsigned)gy, (unsigned)gz), dim3(256),
                     0, b->stream, b->d_img, b->pitch, d_rows, n, d_cols, m, d_out);
  BSN_HIP(hipGetLastError());
}

void readbina_bytes(bsn_bed *b, const uint8_t *d_tab, uint8_t *d_out) {
  require_bits(b, 2, "readbina");
  require_resident(b, "readbina");
  const int64_t nb = (b->n + 3) / 4;
  int64_t gy = b->m < 65535 ? b->m : 65535, gz = (b->m + 65534) / 65535;
  hipLaunchKernelGGL(k_readbina, dim3((unsigned)((nb + 255) / 256), (unsigned)gy, (unsigned)gz), dim3(256), 0,
                     b->stream, b->d_img, b->pitch, b->n, b->m, d_tab, d_out);
  BSN_HIP(hipGetLastError());
}

void subset_pack(bsn_bed *b, const int32_t *d_rows, int64_t n, const int32_t *d_cols, int64_t m,
                 uint8_t *d_out) {
  require_bits(b, 2, "writebina");
  require_resident(b, "writebina");
  int64_t nb = (n + 3) / 4;
  int64_t gy = m < 65535 ? m : 65535, gz = (m + 65534) / 65535;
  hipLaunchKernelGGL(k_subset_pack, dim3((unsigned)((nb + 255) / 256), (unsigned)gy, (unsigned)gz),
                     dim3(256), 0, b->stream, b->d_img, b->pitch, d_rows, n, d_cols, m, nb, d_out);
  BSN_HIP(hipGetLastError());
}

}  // namespace bsn
