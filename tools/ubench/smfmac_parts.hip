// Would k_prodT be faster with ONE structured-sparsity instruction for the code plane and the missing-value plane
// (v_smfmac_i32_16x16x128_i8: 16 compressed int8 per lane + a 32-bit index register against 128 dense K of B) than with
// the two v_mfma_i32_16x16x64_i8 it issues per tile and column block today?  (bigsnpr_amd/csrc/prodt_sparse.hpp has the
// arithmetic.)  This file answers, on the device:
//  (1) the operand LAYOUT — found, not assumed: one-hot A values against B operands that carry their own position — and
//      the EXACTNESS of random compressed values x random legal indices x random int8 B against a host loop; whether the
//      two indices of a group must ascend;
//  (2) the issue cost of the sparse instruction against the dense one (independent accumulators, back to back);
//  (3) the skeleton of k_prodT (16 waves x 2 tiles, chunk-major 64-KB runs, double-buffered digit panel, two / three
//      column blocks) with the dense two-plane decode and with the sparse decode, ms per 100 GB, same run.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I ../../bigsnpr_amd/csrc smfmac_parts.hip -o smfmac_parts
// run:   smfmac_parts [reps] [digits: 0 random, 1 all zero] [quick: 1 = skeletons only (the counter passes)]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <vector>
#include <type_traits>
#include "prodt_sparse.hpp"
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

// ---- (1) layout and exactness -------------------------------------------------------------------------------------
__global__ void k_once(const unsigned *A, const unsigned *I, const unsigned *B, int *D) {
  const int l = threadIdx.x;
  v4i a, c = {0, 0, 0, 0};
  v8i b;
  for (int w = 0; w < 4; w++) a[w] = (int)A[l * 4 + w];
  for (int w = 0; w < 8; w++) b[w] = (int)B[l * 8 + w];
  c = __builtin_amdgcn_smfmac_i32_16x16x128_i8(a, b, c, (int)I[l], 0, 0);
  for (int r = 0; r < 4; r++) D[l * 4 + r] = c[r];
}
struct Once {
  unsigned *dA, *dI, *dB; int *dD;
  std::vector<unsigned> A, I, B; std::vector<int> D;
  Once() : A(256), I(64), B(512), D(256) {
    CK(hipMalloc(&dA, 1024)); CK(hipMalloc(&dI, 256)); CK(hipMalloc(&dB, 2048)); CK(hipMalloc(&dD, 1024));
  }
  void clear() { std::fill(A.begin(), A.end(), 0u); std::fill(I.begin(), I.end(), 0u); std::fill(B.begin(), B.end(), 0u); }
  void setA(int lane, int p, int val, int iv) {
    A[lane * 4 + p / 4] |= (unsigned)(uint8_t)val << (8 * (p & 3));
    I[lane] |= (unsigned)iv << (2 * p);
  }
  void setB(int lane, int e, int val) { B[lane * 8 + e / 4] |= (unsigned)(uint8_t)val << (8 * (e & 3)); }
  void run() {
    CK(hipMemcpy(dA, A.data(), 1024, hipMemcpyHostToDevice)); CK(hipMemcpy(dI, I.data(), 256, hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, B.data(), 2048, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_once, dim3(1), dim3(64), 0, 0, dA, dI, dB, dD);
    CK(hipMemcpy(D.data(), dD, 1024, hipMemcpyDeviceToHost));
  }
};

// map[g][p][iv] = (lane group, byte) of the B operand that compressed value p with index iv of lane group g multiplies
static int map_g[4][16][4], map_e[4][16][4];
static int layout(Once &o) {
  int odd = 0, dbad = 0;
  const int row = 5, col = 3;
  for (int g = 0; g < 4; g++)
    for (int p = 0; p < 16; p++)
      for (int iv = 0; iv < 4; iv++) {
        int got[2];
        for (int pass = 0; pass < 2; pass++) {
          o.clear();
          o.setA(g * 16 + row, p, 1, iv);
          // (the other value of the group keeps index 0 and value 0: it adds nothing wherever it points)
          for (int g2 = 0; g2 < 4; g2++)
            for (int e = 0; e < 32; e++) o.setB(g2 * 16 + col, e, pass == 0 ? e + 1 : g2 + 1);
          o.run();
          int nz = 0, at = -1;
          for (int i = 0; i < 256; i++) if (o.D[i] != 0) nz++, at = i;
          // D as for the dense instruction: lane -> column (l & 15), rows 4 (l >> 4) + r
          if (nz != 1 || at != ((row / 4) * 16 + col) * 4 + row % 4) dbad++;
          got[pass] = nz == 1 ? o.D[at] - 1 : -1;
        }
        map_e[g][p][iv] = got[0];
        map_g[g][p][iv] = got[1];
        if (got[1] != 2 * (g & 1) + (p >> 3) || got[0] != 16 * (g >> 1) + 4 * ((p & 7) / 2) + iv) odd++;
      }
  printf("layout: D as the dense 16x16 form (lane -> column l & 15, rows 4 (l >> 4) + r): %s\n", dbad ? "NO" : "yes");
  printf("layout: value p (byte p of the v4i A of lane group ga), index bits 2p, 2p+1 = iv  ->  dense K 32 ga + 4 (p / 2) + iv; "
         "B: byte e of the v8i of lane group gb is dense K 64 (e / 16) + 16 gb + e %% 16: %s (%d of 256 probes elsewhere)\n",
         odd ? "NO" : "yes", odd);
  if (odd) {
    for (int g = 0; g < 4; g++)
      for (int p = 0; p < 16; p++) {
        printf("  g %d p %2d:", g, p);
        for (int iv = 0; iv < 4; iv++) printf("  iv %d -> (g %d, byte %2d)", iv, map_g[g][p][iv], map_e[g][p][iv]);
        printf("\n");
      }
  }
  return dbad;
}
// random values x indices x B against the host loop over the map found above
// mode 0: legal indices (the two of a group distinct and ascending), 1: distinct but descending in every group,
// 2: both indices of a group equal, 3: the indices and values that prodt_sparse_decode makes from random genotype dwords
static int exactness(Once &o, int mode) {
  srand(17 + mode);
  o.clear();
  std::vector<int> av(64 * 16), ai(64 * 16), bv(64 * 32);
  for (int l = 0; l < 64; l++) {
    if (mode == 3) {
      uint32_t w = 0, a[4], idx;
      for (int e = 0; e < 16; e++) w |= (uint32_t)(rand() % 100 < 20 ? 3 : rand() % 3) << (2 * e);
      bsn::prodt_sparse_decode(w, a, idx);
      for (int p = 0; p < 16; p++) { av[l * 16 + p] = (int)(int8_t)(a[p / 4] >> (8 * (p & 3))); ai[l * 16 + p] = (idx >> (2 * p)) & 3; }
    } else {
      for (int q = 0; q < 8; q++) {
        int i0 = rand() & 3, i1 = rand() & 3;
        if (mode == 2) i1 = i0;
        else {
          while (i1 == i0) i1 = rand() & 3;
          if ((mode == 0) != (i0 < i1)) std::swap(i0, i1);
        }
        ai[l * 16 + 2 * q] = i0; ai[l * 16 + 2 * q + 1] = i1;
        av[l * 16 + 2 * q] = (rand() % 256) - 128; av[l * 16 + 2 * q + 1] = (rand() % 256) - 128;
      }
    }
    for (int p = 0; p < 16; p++) o.setA(l, p, av[l * 16 + p], ai[l * 16 + p]);
    for (int e = 0; e < 32; e++) { bv[l * 32 + e] = (rand() % 256) - 128; o.setB(l, e, bv[l * 32 + e]); }
  }
  o.run();
  int bad = 0;
  for (int l = 0; l < 64; l++)
    for (int r = 0; r < 4; r++) {
      const int i = 4 * (l >> 4) + r, j = l & 15;
      long long s = 0;
      for (int g = 0; g < 4; g++)
        for (int p = 0; p < 16; p++) {
          const int iv = ai[(g * 16 + i) * 16 + p];
          s += (long long)av[(g * 16 + i) * 16 + p] * bv[(map_g[g][p][iv] * 16 + j) * 32 + map_e[g][p][iv]];
        }
      if (s != o.D[l * 4 + r]) bad++;
    }
  static const char *names[] = {"legal indices (distinct, ascending)", "distinct, DEscending in every group", "both indices of a group EQUAL",
                                "operands of prodt_sparse_decode (20 % missing)"};
  printf("exactness, %-48s: %3d of 256 sums differ from the host loop (every value taking the B byte its index names)\n", names[mode], bad);
  return bad;
}

// ---- (2) instruction rate -----------------------------------------------------------------------------------------
template <int KIND>   // 0: dense i8 16x16x64, 1: sparse i8 16x16x128
__global__ __launch_bounds__(256) void k_rate(int *out, int iters) {
  v8i b = {5, 6, 7, (int)blockIdx.x, 9, 10, 11, 12};
  v4i a = {(int)threadIdx.x & 0x03030303, 0x01020102, 0x02010001, 0x01010202};
  const int idx = 0x88888888 | ((int)threadIdx.x & 0x55555555);
  v4i c[8];
  for (int t = 0; t < 8; t++) c[t] = v4i{0, 0, 0, 0};
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int t = 0; t < 8; t++) {
      if (KIND == 1) c[t] = __builtin_amdgcn_smfmac_i32_16x16x128_i8(a, b, c[t], idx, 0, 0);
      else c[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, v4i{b[0], b[1], b[2], b[3]}, c[t], 0, 0, 0);
    }
  }
  int s = 0;
  for (int t = 0; t < 8; t++) s += c[t][0];
  if (s == 0x12345679) out[0] = s;
}
template <int KIND>
static double rate(const char *name, int *dO) {
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int iters = 20000, blocks = 256 * 8;
  for (int rep = 0; rep < 2; rep++) {
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL(k_rate<KIND>, dim3(blocks), dim3(256), 0, 0, dO, iters);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
  }
  float ms; CK(hipEventElapsedTime(&ms, e0, e1));
  const double n = (double)blocks * 4 * iters * 8;
  printf("rate %-28s %8.2f ms  %6.0f dense-equivalent TOP/s  %5.1f cycles per instruction and SIMD at 2.4 GHz\n", name, ms,
         n * 16 * 16 * (KIND ? 128 : 64) * 2 / ms / 1e9, ms * 1e-3 * 2.4e9 / (n / 1024));
  return ms;
}

// ---- (3) kernel skeletons -----------------------------------------------------------------------------------------
// SPARSE 0: the shipped two-plane decode (7 + 4 VALU, 2 NB dense instructions per tile and K-step)
// SPARSE 1: prodt_sparse_decode (NB sparse instructions); the digit panel has the same bytes per lane either way
// PF: the digit operands of the next K-step are read into a second register set while this one's instructions run
template <int SPARSE, int NB, int TILES, int WAVES, int PF>
__global__ __launch_bounds__(64 * WAVES) void k(const uint8_t *__restrict__ img, int64_t pitch, const uint4 *__restrict__ xq4,
                                                unsigned *out, unsigned lutB) {
  constexpr int NCOL = 16 * NB, NT = 64 * WAVES, RW = WAVES * 16 * TILES;
  constexpr int XS = 32 * NCOL * 2;   // uint4 of one chunk's panel: 32 blocks of 16 variants x two 16-B rows x NCOL
  constexpr int NX = XS / NT;
  static_assert(XS % NT == 0 && NX <= 4, "digit staging");
  __shared__ uint4 xs[2][XS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int nchunks = (int)(pitch / 128);
  const int64_t wg = blockIdx.x, nwg = gridDim.x;
  auto addr = [&](int t, int ch, int it) -> const uint4 * {
    const int64_t row = wave * (16 * TILES) + t * 16 + c;
    return (const uint4 *)(img + ((int64_t)ch * nwg + wg) * (RW * 128) + row * 128 + it * 64 + g * 16);
  };
  v4i acc[TILES][NB];
#pragma unroll
  for (int t = 0; t < TILES; t++)
#pragma unroll
    for (int nb = 0; nb < NB; nb++) acc[t][nb] = v4i{0, 0, 0, 0};
  uint4 ga[2][TILES][2];
#pragma unroll
  for (int t = 0; t < TILES; t++)
#pragma unroll
    for (int it = 0; it < 2; it++) { ga[0][t][it] = *addr(t, 0, it); ga[1][t][it] = *addr(t, nchunks > 1 ? 1 : 0, it); }
#pragma unroll
  for (int x = 0; x < NX; x++) xs[0][tid + x * NT] = xq4[tid + x * NT];
  __syncthreads();
  auto chunk = [&](auto SETC, const int ch) {
    constexpr int SET = decltype(SETC)::value;
    const int ch1 = ch + 1 < nchunks ? ch + 1 : nchunks - 1, ch2 = ch + 2 < nchunks ? ch + 2 : nchunks - 1;
    uint4 xr0 = xq4[(int64_t)ch1 * XS + tid], xr1 = {0, 0, 0, 0}, xr2 = xr1, xr3 = xr1;   // (scalars: an array ends up in scratch)
    if constexpr (NX > 1) xr1 = xq4[(int64_t)ch1 * XS + tid + NT];
    if constexpr (NX > 2) xr2 = xq4[(int64_t)ch1 * XS + tid + 2 * NT];
    if constexpr (NX > 3) xr3 = xq4[(int64_t)ch1 * XS + tid + 3 * NT];
    __builtin_amdgcn_sched_barrier(0);
    uint4 bv[2][NB], bn[PF ? 2 : 1][PF ? NB : 1];
    auto readb = [&](const int step, uint4 (&dst)[2][NB]) {
      const int it = step >> 2, d = step & 3;
#pragma unroll
      for (int p = 0; p < 2; p++)
#pragma unroll
        for (int nb = 0; nb < NB; nb++)   // (sparse: the rows the layout found in part (1) asks for, as in k_prodT)
          dst[p][nb] = xs[SET][(SPARSE ? (it * 16 + (2 * p + (g >> 1)) * 4 + d) * 2 + (g & 1) : (it * 16 + g * 4 + d) * 2 + p) * NCOL + nb * 16 + c];
    };
    if constexpr (PF) readb(0, bv);
#pragma unroll
    for (int step = 0; step < 8; step++) {
      const int it = step >> 2, d = step & 3;
      if constexpr (!PF) readb(step, bv);
      else if (step + 1 < 8) readb(step + 1, bn);
#pragma unroll
      for (int t = 0; t < TILES; t++) {
        const uint32_t w = d == 0 ? ga[SET][t][it].x : d == 1 ? ga[SET][t][it].y : d == 2 ? ga[SET][t][it].z : ga[SET][t][it].w;
        if constexpr (SPARSE) {
          uint32_t a[4], idx;
          bsn::prodt_sparse_decode(w, a, idx);
          const v4i av = {(int)a[0], (int)a[1], (int)a[2], (int)a[3]};
#pragma unroll
          for (int nb = 0; nb < NB; nb++) {
            const v8i b = {(int)bv[0][nb].x, (int)bv[0][nb].y, (int)bv[0][nb].z, (int)bv[0][nb].w,
                           (int)bv[1][nb].x, (int)bv[1][nb].y, (int)bv[1][nb].z, (int)bv[1][nb].w};
            acc[t][nb] = __builtin_amdgcn_smfmac_i32_16x16x128_i8(av, b, acc[t][nb], (int)idx, 0, 0);
          }
        } else {
          const uint32_t s0 = w & 0x03030303u, s1 = (w >> 2) & 0x03030303u, s2 = (w >> 4) & 0x03030303u, s3 = (w >> 6) & 0x03030303u;
          const v4i a0 = {(int)s0, (int)s1, (int)s2, (int)s3};
          const v4i a1 = {(int)__builtin_amdgcn_perm(lutB, lutB, s0), (int)__builtin_amdgcn_perm(lutB, lutB, s1),
                          (int)__builtin_amdgcn_perm(lutB, lutB, s2), (int)__builtin_amdgcn_perm(lutB, lutB, s3)};
#pragma unroll
          for (int nb = 0; nb < NB; nb++) {
            const v4i b0 = {(int)bv[0][nb].x, (int)bv[0][nb].y, (int)bv[0][nb].z, (int)bv[0][nb].w};
            const v4i b1 = {(int)bv[1][nb].x, (int)bv[1][nb].y, (int)bv[1][nb].z, (int)bv[1][nb].w};
            acc[t][nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b0, acc[t][nb], 0, 0, 0);
            acc[t][nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b1, acc[t][nb], 0, 0, 0);
          }
        }
      }
      if constexpr (PF) {
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
          for (int nb = 0; nb < NB; nb++) bv[p][nb] = bn[p][nb];
      }
    }
#pragma unroll
    for (int t = 0; t < TILES; t++)
#pragma unroll
      for (int it = 0; it < 2; it++) ga[SET][t][it] = *addr(t, ch2, it);
    __builtin_amdgcn_sched_barrier(0);
    xs[SET ^ 1][tid] = xr0;
    if constexpr (NX > 1) xs[SET ^ 1][tid + NT] = xr1;
    if constexpr (NX > 2) xs[SET ^ 1][tid + 2 * NT] = xr2;
    if constexpr (NX > 3) xs[SET ^ 1][tid + 3 * NT] = xr3;
    __syncthreads();
  };
  for (int ch = 0; ch < nchunks; ch += 2) {
    chunk(std::integral_constant<int, 0>{}, ch);
    if (ch + 1 < nchunks) chunk(std::integral_constant<int, 1>{}, ch + 1);
  }
  unsigned r = 0;
#pragma unroll
  for (int t = 0; t < TILES; t++)
#pragma unroll
    for (int nb = 0; nb < NB; nb++) r ^= (unsigned)(acc[t][nb][0] ^ acc[t][nb][3]);
  if (r == 0x12345679u) out[0] = r;
}

__global__ void fill(uint32_t *p, size_t n, int genotypes) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint32_t h = (uint32_t)(i * 2654435761u) ^ (uint32_t)(i >> 7), w = 0;
    if (genotypes) {
      for (int e = 0; e < 16; e++) {
        h = h * 1664525u + 1013904223u;
        const uint32_t r = h >> 24;
        w |= (r < 3 ? 3u : r < 140 ? 0u : r < 220 ? 1u : 2u) << (2 * e);   // 1 % missing
      }
    } else {
      w = h * 1664525u + 1013904223u;
      w ^= w >> 15;
    }
    p[i] = w;
  }
}

template <int SPARSE, int NB, int TILES, int WAVES, int PF>
static double run(const uint8_t *img, int64_t pitch, int64_t rows, const uint4 *xq, unsigned *out, int reps) {
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  constexpr int RW = WAVES * 16 * TILES;
  const unsigned grid = (unsigned)(rows / RW);
  auto kern = k<SPARSE, NB, TILES, WAVES, PF>;
  hipFuncAttributes fa;
  CK(hipFuncGetAttributes(&fa, (const void *)kern));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * WAVES), 0, 0, img, pitch, xq, out, 0x01000000u);
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0));
  for (int i = 0; i < reps; i++) hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * WAVES), 0, 0, img, pitch, xq, out, 0x01000000u);
  CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
  float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ms /= reps;
  const double bytes = (double)grid * RW * pitch;
  // matrix instructions: per 16 rows x 64 variants (16 B of a row tile) 2 NB dense or NB sparse, 16 pipe cycles each if the
  // sparse form costs what the dense one does
  const double mfma = bytes / 16 / 16 * (SPARSE ? 1 : 2) * NB, cyc = mfma * 16 / 1024;
  printf("prodT %-6s NB=%d tiles=%d waves=%2d pf=%d regs %3d scratch %3zu lds %6zu  %7.2f ms per 100 GB  %5.0f GB/s  pipe floor %5.2f ms at 1.7 GHz\n",
         SPARSE ? "sparse" : "dense", NB, TILES, WAVES, PF, fa.numRegs, (size_t)fa.localSizeBytes, (size_t)fa.sharedSizeBytes,
         ms * 100e9 / bytes, bytes / ms / 1e6, cyc / 1.7e9 * 1e3 * 100e9 / bytes);
  fflush(stdout);
  return ms;
}

int main(int argc, char **argv) {
  const int reps = argc > 1 ? atoi(argv[1]) : 12;
  const int zero_digits = argc > 2 ? atoi(argv[2]) : 0;
  const int quick = argc > 3 ? atoi(argv[3]) : 0;
  if (!quick) {
    Once o;
    int bad = layout(o);
    bad += exactness(o, 0);
    const int desc = exactness(o, 1), same = exactness(o, 2);
    bad += exactness(o, 3);
    printf("exactness: %s; indices of a group %s ascend, %s differ\n", bad ? "FAILED" : "all legal sums exact",
           desc ? "MUST" : "need not", same ? "MUST" : "need not");
    int *dO; CK(hipMalloc(&dO, 4));
    const double d = rate<0>("dense  i8 16x16x64", dO), s = rate<1>("sparse i8 16x16x128 (2:4)", dO);
    printf("rate: the sparse instruction costs %.3f x the dense one\n", s / d);
    fflush(stdout);
  }
  const int64_t pitch = 100096, rows = 245760;   // 480 workgroups of 512 rows x 782 chunks: 24.6 GB per launch
  uint8_t *img; uint4 *xq; unsigned *out;
  const size_t xq_bytes = (size_t)(pitch / 128) * (32 * 48 * 2) * 16;
  CK(hipMalloc(&img, (size_t)rows * pitch)); CK(hipMalloc(&xq, xq_bytes)); CK(hipMalloc(&out, 64));
  hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, 0, (uint32_t *)img, (size_t)rows * pitch / 4, 1);
  if (zero_digits) CK(hipMemset(xq, 0, xq_bytes));
  else hipLaunchKernelGGL(fill, dim3(1024), dim3(256), 0, 0, (uint32_t *)xq, xq_bytes / 4, 0);
  CK(hipDeviceSynchronize());
  printf("digit panels: %s\n", zero_digits ? "all zero" : "random bits");
  for (int pass = 0; pass < (quick ? 1 : 2); pass++) {
    printf("--- pass %d ---\n", pass);
    run<0, 3, 2, 16, 0>(img, pitch, rows, xq, out, reps);   // the shipped shape of k_prodT<3>
    run<1, 3, 2, 16, 0>(img, pitch, rows, xq, out, reps);
    run<1, 3, 2, 16, 1>(img, pitch, rows, xq, out, reps);
    run<0, 2, 2, 16, 1>(img, pitch, rows, xq, out, reps);   // ... of k_prodT<2>
    run<1, 2, 2, 16, 1>(img, pitch, rows, xq, out, reps);
    run<1, 2, 2, 16, 0>(img, pitch, rows, xq, out, reps);
  }
  return 0;
}
