// bgen.hip — snp_readBGEN / snp_prodBGEN on the device (bsn_bgen_read, bsn_bgen_prod) and the inflate they rest on
// (bsn_inflate): the compressed probabilities of a block of variants are uploaded as they lie in the file, inflated one
// wave per zlib stream (k_inflate), and turned into rows of the int8 grid image of CODE_DOSAGE with the per-variant INFO
// score and allele frequency (k_bgen_grid8, k_bgen_final) or multiplied into a matrix without any image (k_bgen_prod).
//
// Replaces src/read-bgen.cpp and src/prod-bgen.cpp behind R/read-bgen.R and R/prod-bgen.R.  The statement of a stream
// lives in inflate_step.hpp, the rules of a sample in bgen_step.hpp; both are shared with the CPU statements under
// tests/native.  The library links no zlib.  DESIGN.md 3.5m.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "bsn_internal.hpp"
#include "bgen_step.hpp"
#include "inflate_step.hpp"

namespace bsn {
namespace {

constexpr int kInflateWavesPerCU = 4;      // 34 KB of LDS per wave: four of them share the 160 KB of a CU
constexpr int64_t kFlushBytes = 2048;      // k_inflate: ring -> output once this much is waiting
constexpr int64_t kMaxBlockVariants = 16384;
constexpr int kProdCols = 8;               // k_bgen_prod: columns of Y per thread (one register tile)
constexpr int kProdRows = 128;             // k_bgen_prod: variants of Y in LDS at a time

// device milliseconds of the last call of this process (bsn_bgen_last_ms): inflate, convert, product
double g_last_ms[3] = {0.0, 0.0, 0.0};

// ---- the sink of k_inflate ----------------------------------------------------------------------------------------------------
// One wave runs inflate::stream with every lane on the same path and the same values (the input bytes are the only
// data, and every lane loads the same ones), so the tables and the literals are written to LDS by all lanes alike: same
// address, same value.  What is spread over the lanes is the moving of bytes: a match reads its len <= 258 source bytes
// (at most five per lane) from the ring, THEN writes them — the serial copy's out[pos + i] = out[pos + i - dist] equals
// out[pos - dist + i % dist] of the bytes before the match, which is what every lane reads — and a flush stores the ring's
// new bytes to the output, lane after lane, and takes their Adler-32 sums along.  The workgroup is this one wave:
// __syncthreads() orders its LDS writes before the other lanes' reads.
// The ring holds the last 32 KiB produced.  The statement has checked dist <= pos and pos + len <= out_cap before copy()
// and pos < out_cap before lit(); a flush writes [flushed, pos) with pos <= out_cap.  Unflushed bytes never exceed
// kFlushBytes + 258, far inside the ring.
struct WaveSink {
  uint8_t *ring;
  uint8_t *out;
  int lane;
  int64_t flushed = 0;
  uint32_t a = 1, b = 0;
  static constexpr int64_t kMask = inflate::kWindow - 1;

  __device__ WaveSink(uint8_t *r, uint8_t *o, int l) : ring(r), out(o), lane(l) {}
  __device__ void lit(int64_t pos, uint8_t v) { ring[pos & kMask] = v; }
  __device__ void copy(int64_t pos, int dist, int len) {
    __syncthreads();
    uint8_t v[5];
#pragma unroll
    for (int q = 0; q < 5; q++) {
      const int i = lane + 64 * q;
      v[q] = i < len ? ring[(pos - dist + i % dist) & kMask] : (uint8_t)0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 5; q++) {
      const int i = lane + 64 * q;
      if (i < len) ring[(pos + i) & kMask] = v[q];
    }
    __syncthreads();
  }
  __device__ void flush(int64_t pos) {
    __syncthreads();
    const int64_t L = pos - flushed;   // <= kFlushBytes + 258
    uint32_t s1 = 0;
    unsigned long long s2 = 0;
    for (int64_t i = lane; i < L; i += 64) {
      const uint32_t x = ring[(flushed + i) & kMask];
      out[flushed + i] = (uint8_t)x;
      s1 += x;
      s2 += (unsigned long long)(L - i) * x;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o, 64);
      s2 += __shfl_xor(s2, o, 64);
    }
    // after L more bytes x_0 .. x_{L-1}:  a' = a + sum x_i,  b' = b + L a + sum (L - i) x_i   (mod 65521)
    b = (uint32_t)(((unsigned long long)b + (unsigned long long)L * a + s2) % inflate::kAdlerMod);
    a = (a + s1) % inflate::kAdlerMod;
    flushed = pos;
  }
  __device__ void after(int64_t pos) {
    if (pos - flushed >= kFlushBytes) flush(pos);
  }
  __device__ uint32_t finish(int64_t pos) {
    flush(pos);
    return (b << 16) | a;
  }
};

// one wave (= one workgroup) per stream, a stride over the streams
__global__ __launch_bounds__(64) void k_inflate(const uint8_t *__restrict__ in, const int64_t *__restrict__ in_off, int64_t K,
                                                uint8_t *out, const int64_t *__restrict__ out_off, int32_t *status) {
  __shared__ uint8_t ring[inflate::kWindow];
  __shared__ inflate::Tables tab;
  const int lane = threadIdx.x;
  for (int64_t k = blockIdx.x; k < K; k += gridDim.x) {
    const int64_t i0 = in_off[k], o0 = out_off[k], cap = out_off[k + 1] - o0;
    WaveSink sink(ring, out + o0, lane);
    const int st = inflate::stream(in + i0, in_off[k + 1] - i0, cap, cap, tab, sink);
    if (lane == 0) status[k] = st;
    __syncthreads();   // the next stream's first writes come after this one's last reads
  }
}

// ---- inflated block -> image rows ---------------------------------------------------------------------------------------------
// buf: variant v of the block at v * D.  One thread per position of ind_row (rows: file samples, any order, repeats
// allowed; validated on the host), blockIdx.y = variant.  img (may be NULL): row col0 + v of the int8 grid image;
// bytes (may be NULL): n x (variants of the block), the FBM's bytes.  sums: 3 per variant (nona, af, num), added with
// integer atomics: exact in any order.  bad: set when a sample's 2 p0 + p1 leaves the table.
__global__ __launch_bounds__(256) void k_bgen_grid8(const uint8_t *__restrict__ buf, int64_t D, int64_t N,
                                                    const int32_t *__restrict__ rows, int64_t n,
                                                    const uint8_t *__restrict__ decode, int dosage, uint64_t seed, int64_t col0,
                                                    uint8_t *img, int64_t pitch, uint8_t *bytes, unsigned long long *sums,
                                                    int32_t *bad) {
  __shared__ uint8_t tab[bgen::kTable + 1];
  for (int t = threadIdx.x; t < bgen::kTable; t += 256) tab[t] = decode[t];
  __syncthreads();
  const int64_t v = blockIdx.y;
  const uint8_t *b = buf + v * D;
  long long nona = 0, af = 0, num = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t ig = rows[i];
    uint8_t fb = 3;
    if (b[bgen::ploidy_at(ig)] < 0x80) {
      const int p0 = b[bgen::prob_at(N, ig)], p1 = b[bgen::prob_at(N, ig) + 1];
      const int k = 2 * p0 + p1;
      if (k >= bgen::kTable) {
        *bad = 1;
      } else {
        nona++;
        af += bgen::af_term(p0, p1);
        num += bgen::num_term(p0, p1);
        fb = dosage ? tab[k] : (uint8_t)(4 + bgen::random_call(bgen::unit(seed, (uint64_t)i, (uint64_t)(col0 + v)), p0, p1));
      }
    }
    if (img) img[(col0 + v) * pitch + i] = (uint8_t)bgen::grid_of_byte(fb);
    if (bytes) bytes[v * n + i] = fb;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nona += __shfl_xor(nona, o, 64);
    af += __shfl_xor(af, o, 64);
    num += __shfl_xor(num, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&sums[3 * v + 0], (unsigned long long)nona);
    atomicAdd(&sums[3 * v + 1], (unsigned long long)af);
    atomicAdd(&sums[3 * v + 2], (unsigned long long)num);
  }
}

__global__ void k_bgen_final(const unsigned long long *__restrict__ sums, int64_t cnt, double *info, double *freq) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= cnt) return;
  const bgen::InfoFreq r = bgen::info_freq((int64_t)sums[3 * v], (int64_t)sums[3 * v + 1], (int64_t)sums[3 * v + 2]);
  info[v] = r.info;
  freq[v] = r.freq;
}

// ---- inflated block x Y ---------------------------------------------------------------------------------------------------------
// XY[i, c] += sum_v x(i, v) Y[v, c] in fp64, v ascending.  Samples along the lanes, kProdCols columns of Y per thread in
// registers (blockIdx.y = column tile), kProdRows rows of Y in LDS at a time.  x = decode[2 p0 + p1] (dosage) or the
// drawn call; a missing sample is NaN and stays NaN in its row.  Y: cnt x ncol, column-major, ld = cnt.
__global__ __launch_bounds__(256) void k_bgen_prod(const uint8_t *__restrict__ buf, int64_t D, int64_t N, int64_t cnt,
                                                   const int32_t *__restrict__ rows, int64_t n,
                                                   const double *__restrict__ decode, int dosage, uint64_t seed, int64_t col0,
                                                   const double *__restrict__ Y, int64_t ncol, double *XY, int32_t *bad) {
  __shared__ double Ys[kProdRows * kProdCols];
  const int64_t c0 = (int64_t)blockIdx.y * kProdCols;
  const int nc = (int)std::min<int64_t>(kProdCols, ncol - c0);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ig = i < n ? rows[i] : 0;
  double acc[kProdCols];
#pragma unroll
  for (int c = 0; c < kProdCols; c++) acc[c] = 0.0;
  for (int64_t v0 = 0; v0 < cnt; v0 += kProdRows) {
    const int nv = (int)std::min<int64_t>(kProdRows, cnt - v0);
    __syncthreads();
    for (int t = threadIdx.x; t < kProdRows * kProdCols; t += 256) {
      const int v = t / kProdCols, c = t % kProdCols;
      Ys[t] = (v < nv && c < nc) ? Y[(v0 + v) + (c0 + c) * cnt] : 0.0;
    }
    __syncthreads();
    if (i < n) {
      for (int v = 0; v < nv; v++) {
        const uint8_t *b = buf + (v0 + v) * D;
        double x = __builtin_nan("");
        if (b[bgen::ploidy_at(ig)] < 0x80) {
          const int p0 = b[bgen::prob_at(N, ig)], p1 = b[bgen::prob_at(N, ig) + 1];
          const int k = 2 * p0 + p1;
          if (k >= bgen::kTable)
            *bad = 1;
          else
            x = dosage ? decode[k] : (double)bgen::random_call(bgen::unit(seed, (uint64_t)i, (uint64_t)(col0 + v0 + v)), p0, p1);
        }
#pragma unroll
        for (int c = 0; c < kProdCols; c++) acc[c] += x * Ys[v * kProdCols + c];
      }
    }
  }
  if (i < n)
    for (int c = 0; c < nc; c++) XY[i + (c0 + c) * n] += acc[c];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// a mapped .bgen file whose header has been checked (R/read-bgen.R:67-82)
struct BgenFile {
  const uint8_t *p = nullptr;
  size_t len = 0;
  int64_t N = 0;
  explicit BgenFile(const char *path) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) fail("Error while opening '%s'.", path);
    struct stat sb;
    if (fstat(fd, &sb) != 0 || sb.st_size <= 0) {
      close(fd);
      fail("'%s' is not a BGEN file.", path);
    }
    len = (size_t)sb.st_size;
    void *m = mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) fail("Error when mapping file:\n  %s.\n", strerror(errno));
    p = (const uint8_t *)m;
    try {
      if (len < 24 || std::memcmp(p + 16, "bgen", 4) != 0) fail("'%s' is not a BGEN file.", path);
      const size_t LH = rd32(p + 4);
      if (LH < 20 || 4 + LH > len) fail("'%s' is not a BGEN file.", path);
      const uint32_t flags = rd32(p + 4 + LH - 4);
      if ((flags & 3u) != 1u) fail("'%s' is not compressed with zlib.", path);
      if (((flags >> 2) & 15u) != 2u) fail("'%s' is not using Layout 2.", path);
      N = rd32(p + 12);
    } catch (...) {
      munmap((void *)p, len);
      throw;
    }
  }
  ~BgenFile() {
    if (p) munmap((void *)p, len);
  }
  BgenFile(const BgenFile &) = delete;
  BgenFile &operator=(const BgenFile &) = delete;

  // the compressed probabilities of the variant whose record starts at `off` (src/read-bgen.cpp:27-39)
  struct Payload {
    const uint8_t *z;
    int64_t C;
  };
  Payload variant(int64_t off, int64_t N_arg) const {
    size_t q = 0;
    auto room = [&](size_t k) {
      if (q + k > len || q + k < q) fail("A variant's record runs past the end of the file.");
    };
    if (off < 0 || (size_t)off >= len) fail("A variant's record runs past the end of the file.");
    q = (size_t)off;
    for (int s = 0; s < 3; s++) {   // id, rsid, chromosome
      room(2);
      const size_t l = rd16(p + q);
      q += 2;
      room(l);
      q += l;
    }
    room(6);
    const int32_t pos = (int32_t)rd32(p + q);
    const uint32_t K = rd16(p + q + 4);
    q += 6;
    if (pos <= 0) fail("Positions should be positive.");
    if (K != 2) fail("Only 2 alleles allowed.");
    for (int s = 0; s < 2; s++) {
      room(4);
      const size_t l = rd32(p + q);
      q += 4;
      room(l);
      q += l;
    }
    room(8);
    const int64_t C = (int64_t)rd32(p + q) - 4, D = (int64_t)rd32(p + q + 4);
    q += 8;
    if (D != 10 + 3 * N_arg) fail("Probabilities should be stored using 8 bits.");
    if (C < 0) fail("Problem when uncompressing.");
    room((size_t)C);
    return Payload{p + q, C};
  }
};

// a handle that owns nothing but a stream and the two staging buffers: the context of copy_h2d / copy_d2h for the entries
// that have no image
std::unique_ptr<bsn_bed, void (*)(bsn_bed *)> staging_context() {
  std::unique_ptr<bsn_bed, void (*)(bsn_bed *)> c(new bsn_bed(), bed_free);
  image_alloc(c.get(), 1, 1, 8);
  return c;
}

int inflate_grid(int64_t K) {
  int dev = 0, cus = 0;
  BSN_HIP(hipGetDevice(&dev));
  BSN_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  return (int)std::max<int64_t>(1, std::min<int64_t>(K, (int64_t)std::max(cus, 1) * kInflateWavesPerCU));
}

void check_offsets(const int64_t *off, int64_t K, const char *what) {
  if (off[0] < 0) fail("bsn_inflate: '%s' starts below 0", what);
  for (int64_t k = 0; k < K; k++)
    if (off[k + 1] < off[k]) fail("bsn_inflate: '%s' decreases at %lld", what, (long long)k);
}

void inflate_host(const uint8_t *in, const int64_t *in_off, int64_t K, uint8_t *out, const int64_t *out_off, int32_t *status) {
  require_gpu();
  if (K < 0 || !in_off || !out_off || !status) fail("bsn_inflate: missing argument");
  if (K == 0) return;
  check_offsets(in_off, K, "in_off");
  check_offsets(out_off, K, "out_off");
  auto ctx = staging_context();
  hipStream_t st = ctx->stream;
  DevBuf<uint8_t> d_in, d_out;
  DevBuf<int64_t> d_off;
  DevBuf<int32_t> d_status;
  const size_t nin = (size_t)in_off[K], nout = (size_t)out_off[K];
  d_in.ensure(std::max<size_t>(nin, 1));
  d_out.ensure(std::max<size_t>(nout, 1));
  d_off.ensure((size_t)2 * (K + 1));
  d_status.ensure((size_t)K);
  if (nin) copy_h2d(ctx.get(), d_in.p, in, nin);
  copy_h2d(ctx.get(), d_off.p, in_off, (size_t)(K + 1) * 8);
  copy_h2d(ctx.get(), d_off.p + (K + 1), out_off, (size_t)(K + 1) * 8);
  BSN_HIP(hipMemsetAsync(d_out.p, 0, std::max<size_t>(nout, 1), st));
  EventMarks<2> ev;
  g_last_ms[0] = g_last_ms[1] = g_last_ms[2] = 0.0;
  ev.mark(0, st);
  hipLaunchKernelGGL(k_inflate, dim3((unsigned)inflate_grid(K)), dim3(64), 0, st, d_in.p, d_off.p, K, d_out.p, d_off.p + (K + 1),
                     d_status.p);
  BSN_HIP(hipGetLastError());
  ev.mark(1, st);
  copy_d2h(ctx.get(), status, d_status.p, (size_t)K * 4);
  if (nout && out) copy_d2h(ctx.get(), out, d_out.p, nout);
  BSN_HIP(hipStreamSynchronize(st));
  g_last_ms[0] = ev.ms(0, 1);
}

// What both BGEN entries share: the file, the row list on the device, and the walk over blocks of variants — pack the
// compressed payloads, upload, inflate, check every stream's status, hand the inflated block to `f`.
struct BlockWalk {
  bsn_bed *ctx;
  hipStream_t st;
  int64_t N, D, K, bv;
  DevBuf<uint8_t> d_in, d_out;
  DevBuf<int64_t> d_off;
  DevBuf<int32_t> d_status, d_rows, d_bad;
  std::vector<uint8_t> h_in;
  std::vector<int64_t> h_off;
  std::vector<int32_t> h_status;
};

int64_t choose_block(int64_t K, int64_t D, int64_t n, int64_t block_variants, bool bytes) {
  if (block_variants < 0) fail("'block_variants' should not be negative.");
  int64_t bv = block_variants;
  if (bv == 0) {
    // inflated block + its compressed bytes (never more than a little above D per variant) + FBM bytes, in a quarter
    // of the free memory, at most 1 GiB of inflated bytes
    size_t free_b = 0, total_b = 0;
    BSN_HIP(hipMemGetInfo(&free_b, &total_b));
    const double per = 2.2 * (double)D + (bytes ? (double)n : 0.0) + 64;
    bv = (int64_t)std::min((double)(free_b + dev_cache_held()) / 4.0 / per, (double)((size_t)1 << 30) / (double)D);
  }
  return std::max<int64_t>(1, std::min<int64_t>(std::min(bv, K), kMaxBlockVariants));
}

template <class F>
void walk_blocks(const char *path, const int64_t *offsets, int64_t K, int64_t N, const int64_t *ind_row, int64_t n,
                 int64_t block_variants, bool bytes, bsn_bed *ctx, F &&f) {
  if (!path || !offsets || !ind_row) fail("BGEN: missing argument");
  if (K <= 0 || n <= 0 || N <= 0) fail("BGEN: nothing to read");
  if (N >= ((int64_t)1 << 30) || n >= ((int64_t)1 << 31)) fail("dimension too large");
  for (int64_t i = 0; i < n; i++)
    if (ind_row[i] < 0 || ind_row[i] >= N) fail("all(ind_row >= 1 & ind_row <= N) is not TRUE");
  BgenFile file(path);
  if (file.N != N) fail("'%s' holds %lld samples, not %lld.", path, (long long)file.N, (long long)N);
  BlockWalk w;
  w.ctx = ctx;
  w.st = ctx->stream;
  w.N = N;
  w.D = 10 + 3 * N;
  w.K = K;
  w.bv = choose_block(K, w.D, n, block_variants, bytes);
  std::vector<int32_t> rows((size_t)n);
  for (int64_t i = 0; i < n; i++) rows[(size_t)i] = (int32_t)ind_row[i];
  copy_h2d(ctx, w.d_rows.ensure((size_t)n), rows.data(), (size_t)n * 4);
  BSN_HIP(hipMemsetAsync(w.d_bad.ensure(1), 0, 4, w.st));
  w.d_out.ensure((size_t)w.bv * (size_t)w.D);
  w.d_off.ensure((size_t)2 * (w.bv + 1));
  w.d_status.ensure((size_t)w.bv);
  EventMarks<2> ev;
  const int grid_cap = inflate_grid(kMaxBlockVariants);
  for (int64_t k0 = 0; k0 < K; k0 += w.bv) {
    const int64_t cnt = std::min(w.bv, K - k0);
    w.h_off.assign((size_t)2 * (cnt + 1), 0);
    w.h_in.clear();
    for (int64_t v = 0; v < cnt; v++) {
      const BgenFile::Payload pl = file.variant(offsets[k0 + v], N);
      w.h_in.insert(w.h_in.end(), pl.z, pl.z + pl.C);
      w.h_off[(size_t)v + 1] = (int64_t)w.h_in.size();
      w.h_off[(size_t)(cnt + 1) + v + 1] = (v + 1) * w.D;
    }
    w.d_in.ensure(std::max<size_t>(w.h_in.size(), 1));
    if (!w.h_in.empty()) copy_h2d(ctx, w.d_in.p, w.h_in.data(), w.h_in.size());
    copy_h2d(ctx, w.d_off.p, w.h_off.data(), w.h_off.size() * 8);
    ev.mark(0, w.st);
    hipLaunchKernelGGL(k_inflate, dim3((unsigned)std::min<int64_t>(cnt, grid_cap)), dim3(64), 0, w.st, w.d_in.p, w.d_off.p, cnt,
                       w.d_out.p, w.d_off.p + (cnt + 1), w.d_status.p);
    BSN_HIP(hipGetLastError());
    ev.mark(1, w.st);
    w.h_status.resize((size_t)cnt);
    copy_d2h(ctx, w.h_status.data(), w.d_status.p, (size_t)cnt * 4);   // (waits for the kernel)
    g_last_ms[0] += ev.ms(0, 1);
    for (int64_t v = 0; v < cnt; v++)
      if (w.h_status[(size_t)v] != 0)
        fail("Problem when uncompressing. (variant %lld, status %d)", (long long)(k0 + v), (int)w.h_status[(size_t)v]);
    f(w, k0, cnt);
  }
  int32_t bad = 0;
  copy_d2h(ctx, &bad, w.d_bad.p, 4);
  if (bad) fail("Probabilities of a sample add up to more than 1: this is not 8-bit unphased biallelic data.");
}

void bgen_read(const char *path, const int64_t *offsets, int64_t K, int64_t N, const int64_t *ind_row, int64_t n,
               const uint8_t *decode, int dosage, uint64_t seed, int64_t col0, int64_t m_total, int64_t block_variants,
               bsn_bed **inout, uint8_t *fbm_bytes_out, double *info_out, double *freq_out) {
  require_gpu();
  g_last_ms[0] = g_last_ms[1] = g_last_ms[2] = 0.0;
  if (!inout || !decode) fail("snp_readBGEN: missing argument");
  for (int k = 0; k < bgen::kTable; k++)
    if (decode[k] > bgen::kMaxFbmByte)
      fail("snp_readBGEN: 'decode' holds the byte %d (at %d): CODE_DOSAGE has no value above byte %d, so the int8 grid image "
           "cannot hold it",
           (int)decode[k], k, bgen::kMaxFbmByte);
  if (col0 < 0 || K <= 0 || col0 + K > m_total) fail("snp_readBGEN: columns %lld .. %lld do not lie in 0 .. %lld", (long long)col0,
                                                      (long long)(col0 + K - 1), (long long)m_total - 1);
  std::unique_ptr<bsn_bed, void (*)(bsn_bed *)> made(nullptr, bed_free);   // a failed call frees the image it created
  bsn_bed *img = *inout;
  if (!img) {
    if (n <= 0) fail("n and p must be positive.");
    const double need = (double)(m_total + 64) * (double)round_up(n, kPitchAlign);
    size_t free_b = 0, total_b = 0;
    BSN_HIP(hipMemGetInfo(&free_b, &total_b));
    const double room = (double)(free_b + dev_cache_held());
    if (need > room)
      fail("snp_readBGEN: the result image (%.2f GB, one byte per genotype) does not fit the free device memory (%.2f GB); an "
           "out-of-core result is not supported",
           need / 1e9, room / 1e9);
    made.reset(new bsn_bed());
    img = made.get();
    image_alloc(img, n, m_total, 8);
    img->v_off = 1.0;   // the grid bsn_fbm_open derives from CODE_DOSAGE: 0.00 .. 2.00 by 0.01 about 1
    img->v_step = 2.0 / 200.0;
    BSN_HIP(hipMemsetAsync(img->d_img, 0, (size_t)(m_total + 64) * (size_t)img->pitch, img->stream));   // pad samples, pad variants
    img->na_cnt.assign((size_t)m_total, -1);
  } else {
    BSN_HIP(hipSetDevice(img->device));
    require_resident(img, "snp_readBGEN");
    refuse_generic(img, "snp_readBGEN");
    require_bits(img, 8, "snp_readBGEN");
    if (img->n != n || img->m != m_total) fail("Incompatibility between dimensions.");
    if ((int64_t)img->na_cnt.size() != m_total) img->na_cnt.assign((size_t)m_total, -1);
  }
  DevBuf<uint8_t> d_dec, d_bytes;
  DevBuf<unsigned long long> d_sums;
  DevBuf<double> d_if;
  copy_h2d(img, d_dec.ensure(512), decode, bgen::kTable);
  EventMarks<2> ev;
  std::vector<unsigned long long> sums;
  walk_blocks(path, offsets, K, N, ind_row, n, block_variants, fbm_bytes_out != nullptr, img,
              [&](BlockWalk &w, int64_t k0, int64_t cnt) {
                hipStream_t st = w.st;
                BSN_HIP(hipMemsetAsync(d_sums.ensure((size_t)3 * w.bv), 0, (size_t)3 * cnt * 8, st));
                d_if.ensure((size_t)2 * w.bv);
                if (fbm_bytes_out) d_bytes.ensure((size_t)w.bv * (size_t)n);
                ev.mark(0, st);
                const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1024));
                hipLaunchKernelGGL(k_bgen_grid8, dim3(gx, (unsigned)cnt), dim3(256), 0, st, w.d_out.p, w.D, w.N, w.d_rows.p, n,
                                   d_dec.p, dosage, seed, col0 + k0, img->d_img, img->pitch, fbm_bytes_out ? d_bytes.p : nullptr,
                                   d_sums.p, w.d_bad.p);
                BSN_HIP(hipGetLastError());
                hipLaunchKernelGGL(k_bgen_final, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, d_sums.p, cnt, d_if.p,
                                   d_if.p + w.bv);
                BSN_HIP(hipGetLastError());
                ev.mark(1, st);
                sums.resize((size_t)3 * cnt);
                copy_d2h(img, sums.data(), d_sums.p, sums.size() * 8);
                if (info_out) copy_d2h(img, info_out + k0, d_if.p, (size_t)cnt * 8);
                if (freq_out) copy_d2h(img, freq_out + k0, d_if.p + w.bv, (size_t)cnt * 8);
                if (fbm_bytes_out) copy_d2h(img, fbm_bytes_out + k0 * n, d_bytes.p, (size_t)cnt * (size_t)n);
                g_last_ms[1] += ev.ms(0, 1);
                for (int64_t v = 0; v < cnt; v++) img->na_cnt[(size_t)(col0 + k0 + v)] = (int32_t)(n - (int64_t)sums[(size_t)(3 * v)]);
              });
  img->forget_counts();
  BSN_HIP(hipStreamSynchronize(img->stream));
  if (made) *inout = made.release();
}

void bgen_prod(const char *path, const int64_t *offsets, int64_t K, int64_t N, const int64_t *ind_row, int64_t n,
               const double *decode, int dosage, uint64_t seed, int64_t col0, const double *Y, int64_t ldy, int64_t ncol,
               int64_t block_variants, double *XY) {
  require_gpu();
  g_last_ms[0] = g_last_ms[1] = g_last_ms[2] = 0.0;
  if (!decode || !Y || !XY) fail("snp_prodBGEN: missing argument");
  if (ncol <= 0 || ldy < K) fail("Incompatibility between dimensions.");
  if (ncol > 65535 * (int64_t)kProdCols) fail("snp_prodBGEN: too many columns in 'beta'");
  auto ctx = staging_context();
  DevBuf<double> d_dec, d_Y, d_XY;
  copy_h2d(ctx.get(), d_dec.ensure(512), decode, bgen::kTable * 8);
  if (n > 0 && K > 0) copy_h2d(ctx.get(), d_XY.ensure((size_t)n * (size_t)ncol), XY, (size_t)n * (size_t)ncol * 8);
  EventMarks<2> ev;
  std::vector<double> hY;
  walk_blocks(path, offsets, K, N, ind_row, n, block_variants, false, ctx.get(), [&](BlockWalk &w, int64_t k0, int64_t cnt) {
    hipStream_t st = w.st;
    hY.resize((size_t)cnt * (size_t)ncol);
    for (int64_t c = 0; c < ncol; c++) std::memcpy(hY.data() + c * cnt, Y + c * ldy + k0, (size_t)cnt * 8);
    copy_h2d(ctx.get(), d_Y.ensure((size_t)w.bv * (size_t)ncol), hY.data(), hY.size() * 8);
    ev.mark(0, st);
    hipLaunchKernelGGL(k_bgen_prod, dim3((unsigned)((n + 255) / 256), (unsigned)((ncol + kProdCols - 1) / kProdCols)), dim3(256), 0,
                       st, w.d_out.p, w.D, w.N, cnt, w.d_rows.p, n, d_dec.p, dosage, seed, col0 + k0, d_Y.p, ncol, d_XY.p,
                       w.d_bad.p);
    BSN_HIP(hipGetLastError());
    ev.mark(1, st);
    BSN_HIP(hipStreamSynchronize(st));   // hY and the inflated block are reused by the next turn
    g_last_ms[2] += ev.ms(0, 1);
  });
  copy_d2h(ctx.get(), XY, d_XY.p, (size_t)n * (size_t)ncol * 8);
}

}  // namespace
}  // namespace bsn

extern "C" {

int bsn_inflate(const uint8_t *in, const int64_t *in_off, int64_t K, uint8_t *out, const int64_t *out_off, int32_t *status) {
  return bsn::guarded([&] { bsn::inflate_host(in, in_off, K, out, out_off, status); });
}

int bsn_bgen_read(const char *path, const int64_t *offsets, int64_t K, int64_t N, const int64_t *ind_row, int64_t n,
                  const uint8_t *decode, int dosage, uint64_t seed, int64_t col0, int64_t m_total, int64_t block_variants,
                  bsn_bed **inout, uint8_t *fbm_bytes_out, double *info_out, double *freq_out) {
  return bsn::guarded([&] {
    bsn::bgen_read(path, offsets, K, N, ind_row, n, decode, dosage, seed, col0, m_total, block_variants, inout, fbm_bytes_out,
                   info_out, freq_out);
  });
}

int bsn_bgen_prod(const char *path, const int64_t *offsets, int64_t K, int64_t N, const int64_t *ind_row, int64_t n,
                  const double *decode, int dosage, uint64_t seed, int64_t col0, const double *Y, int64_t ldy, int64_t ncol,
                  int64_t block_variants, double *XY) {
  return bsn::guarded([&] {
    bsn::bgen_prod(path, offsets, K, N, ind_row, n, decode, dosage, seed, col0, Y, ldy, ncol, block_variants, XY);
  });
}

int bsn_bgen_last_ms(double *ms_out) {
  return bsn::guarded([&] {
    for (int k = 0; k < 3; k++) ms_out[k] = bsn::g_last_ms[k];
  });
}

}  // extern "C"
