// svd_panel.hip — the panel kernels of the block-Lanczos partial SVD (svd.hip: HipSvdBackend), their launches
// (svd_panel.hpp) and the kernel-level test entries bsn_panel_*.  The tall-skinny fp64 panel algebra is memory-bound
// on the basis Q (n x p doubles) and is a few percent of a block step.
#include <algorithm>
#include <vector>

#include "svd_panel.hpp"

namespace bsn {

constexpr int kTP = 256;  // basis columns per LDS tile of k_gemm_nn

__device__ __forceinline__ uint32_t hmix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}

// rows [row0, row0 + n) of the n_total x b start block (a function of the global row index, so that
// sample blocks of different ranks are pieces of the same matrix); rows past n_total are zero
__global__ void k_random(double *W, int64_t ld, int64_t n, int b, uint32_t seed, int64_t row0, int64_t n_total) {
  int64_t il = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int j = blockIdx.y;
  if (il >= n || j >= b) return;
  const int64_t i = il + row0;
  if (i >= n_total) {
    W[il + j * ld] = 0.0;
    return;
  }
  uint32_t h = hmix((uint32_t)i * 0x9E3779B1U + hmix(seed * 0x85EBCA6BU + (uint32_t)j + 0x1234567U));
  uint32_t h2 = hmix(h ^ 0xDEADBEEFU);
  // uniform in (-1, 1) with 53 random bits
  double x = ((double)(((uint64_t)h << 21) ^ (uint64_t)h2) + 0.5) * (1.0 / 9007199254740992.0);
  W[il + j * ld] = 2.0 * x - 1.0;
}

typedef double v4d __attribute__((ext_vector_type(4)));
struct __attribute__((aligned(8))) d2 {
  double x, y;
};

// C (p x cb, leading dimension ldc) = A[:, :p]' B[:, :cb]: the tall-skinny TN product of the panel algebra
// on the fp64 matrix pipe.  v_mfma_f64_16x16x4 with the 16 columns of an A tile as M, the (<= 16) columns
// of B as N and four rows as K: lane l supplies A[row, tile*16 + (l & 15)] and B[row, l & 15] for row slot
// l >> 4; which row a slot stands for is free as long as A and B agree, so a lane takes TWO consecutive
// rows per 16-byte load (rows r + 2 (l >> 4) + {0, 1} of an 8-row group, two MFMAs): every load
// instruction then reads 64 contiguous bytes per column, straight from global memory — A is read exactly
// once, B once per 16 columns of A (round 2's VALU kernel re-read B once per FOUR columns of A and was
// the largest item of a solve outside the streaming passes).
// Workgroup (tile, rc) covers rows [rc, rc + 1) * kGemmRows with four waves and writes the 16 x 16 sums to
// partial[rc][tile]; k_gemm_tn_reduce adds the chunks up.
// NT: 16-column tiles of B (cb <= 16 NT); an A tile is loaded once for all of them.
template <int NT>
__global__ __launch_bounds__(256) void k_gemm_tn(const double *__restrict__ A, int64_t lda, int p,
                                                 const double *__restrict__ B, int64_t ldb, int cb, int64_t n,
                                                 double *partial) {
  const int tile = blockIdx.x, rc = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int a = lane & 15, kq = lane >> 4;
  // columns past p (past cb) are read from a valid one and discarded (masked): no branch around the loads
  const int ca = tile * 16 + a < p ? tile * 16 + a : p - 1;
  const double *Ap = A + (int64_t)ca * lda;
  bool bval[NT];
  const double *Bp[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    bval[t] = t * 16 + a < cb;
    Bp[t] = B + (int64_t)(bval[t] ? t * 16 + a : 0) * ldb;
  }
  const int64_t c0 = (int64_t)rc * kGemmRows, c1 = c0 + kGemmRows < n ? c0 + kGemmRows : n;
  const int64_t r0 = c0 + wave * (kGemmRows / 4);
  const int64_t r1 = r0 + kGemmRows / 4 < c1 ? r0 + kGemmRows / 4 : c1;
  v4d acc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
  // groups of 32 rows through two register sets: the loads of a group are in flight while the MFMAs of the
  // previous one run (a wave that waited out every group's memory round trip left the kernel latency-bound
  // at a quarter of the bandwidth).  No branch around the loads: past the end the last group is loaded again.
  d2 av0[4], bv0[NT][4], av1[4], bv1[NT][4];
  auto ld = [&](int64_t rr, d2 (&av)[4], d2 (&bv)[NT][4]) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      av[u] = *(const d2 *)(Ap + rr + 8 * u + 2 * kq);
#pragma unroll
      for (int t = 0; t < NT; t++) bv[t][u] = *(const d2 *)(Bp[t] + rr + 8 * u + 2 * kq);
    }
  };
  auto mm = [&](const d2 (&av)[4], const d2 (&bv)[NT][4]) {
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int t = 0; t < NT; t++) {
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u].x, bval[t] ? bv[t][u].x : 0.0, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u].y, bval[t] ? bv[t][u].y : 0.0, acc[t], 0, 0, 0);
      }
  };
  const int64_t nfull = r1 > r0 ? (r1 - r0) / 32 : 0;
  if (nfull > 0) {
    ld(r0, av0, bv0);
    for (int64_t g = 0; g < nfull; g += 2) {
      ld(r0 + 32 * (g + 1 < nfull ? g + 1 : nfull - 1), av1, bv1);
      mm(av0, bv0);
      ld(r0 + 32 * (g + 2 < nfull ? g + 2 : nfull - 1), av0, bv0);
      if (g + 1 < nfull) mm(av1, bv1);
    }
  }
  int64_t r = r0 + 32 * nfull;
  for (; r < r1; r += 8) {   // the ragged end of the last chunk
    const int64_t i0 = r + 2 * kq, i1 = i0 + 1;
    const double a0 = i0 < r1 ? Ap[i0] : 0.0, a1 = i1 < r1 ? Ap[i1] : 0.0;
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const double b0 = (bval[t] && i0 < r1) ? Bp[t][i0] : 0.0, b1 = (bval[t] && i1 < r1) ? Bp[t][i1] : 0.0;
      acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[t], 0, 0, 0);
    }
  }
  // D: column of B = lane & 15, column of the A tile = (lane >> 4) + 4 * reg
  __shared__ double red[4][256];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    if (t > 0) __syncthreads();
#pragma unroll
    for (int g = 0; g < 4; g++) red[wave][(kq + 4 * g) * 16 + a] = acc[t][g];
    __syncthreads();
    partial[(((int64_t)rc * gridDim.x + tile) * NT + t) * 256 + tid] =
        (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  }
}

// C[tile*16 + mrow, ncol] = sum over the row chunks, in a fixed order (four interleaved running sums, then
// their sum): identical on every rank and in every run.  (A single launch with a "last workgroup adds up"
// tail was tried in round 3: the device-scope fences it needs write back the L2 of every XCD, 0.15 us per
// workgroup, several times the product itself.)
__global__ __launch_bounds__(1024) void k_gemm_tn_reduce(const double *__restrict__ partial, int nrc, int ntile, int p,
                                                         int cb, double *C, int ldc) {
  const int tile = blockIdx.x, bt = blockIdx.y, nt = gridDim.y, t = threadIdx.x & 255, part = threadIdx.x >> 8;
  double sum = 0;
#pragma unroll 4
  for (int c = part; c < nrc; c += 4) sum += partial[(((int64_t)c * ntile + tile) * nt + bt) * 256 + t];
  __shared__ double sp[4][256];
  sp[part][t] = sum;
  __syncthreads();
  if (part == 0) {
    sum = (sp[0][t] + sp[1][t]) + (sp[2][t] + sp[3][t]);
    const int mrow = t >> 4, ncol = bt * 16 + (t & 15);
    if (tile * 16 + mrow < p && ncol < cb) C[(tile * 16 + mrow) + (int64_t)ncol * ldc] = sum;
  }
}

// Out[i, j] = alpha * In[i, j] + beta * sum_a Q[i, a] S[a, j],  j < nc <= 8; S (p x nc) in global
__global__ __launch_bounds__(256) void k_gemm_nn(const double *__restrict__ Q, int64_t ldq, int p,
                                                 const double *__restrict__ S, int nc,
                                                 const double *In, int64_t ldi, double alpha,
                                                 double beta, double *Out, int64_t ldo, int64_t n) {
  extern __shared__ __attribute__((aligned(16))) double sS[];  // tile of S: TP x kMaxB
  constexpr int TP = kTP;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double acc[kMaxB];
#pragma unroll
  for (int j = 0; j < kMaxB; j++) acc[j] = 0;
  for (int a0 = 0; a0 < p; a0 += TP) {
    int ta = p - a0 < TP ? p - a0 : TP;
    __syncthreads();
    for (int t = threadIdx.x; t < ta * kMaxB; t += blockDim.x) {
      int a = t / kMaxB, j = t % kMaxB;
      sS[t] = j < nc ? S[(a0 + a) + (int64_t)j * p] : 0.0;
    }
    __syncthreads();
    if (i < n) {
      for (int a = 0; a < ta; a++) {
        double q = Q[i + (int64_t)(a0 + a) * ldq];
#pragma unroll
        for (int j = 0; j < kMaxB; j++) acc[j] += q * sS[a * kMaxB + j];
      }
    }
  }
  if (i < n) {
#pragma unroll
    for (int j = 0; j < kMaxB; j++)
      if (j < nc) {
        double base = alpha != 0.0 ? alpha * In[i + (int64_t)j * ldi] : 0.0;
        Out[i + (int64_t)j * ldo] = base + beta * acc[j];
      }
  }
}

__global__ void k_put_block(double *M, int ld, int r, const double *src) {   // M[:r, :r] (leading dimension ld) = src (r x r)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < r * r) M[(t % r) + (int64_t)(t / r) * ld] = src[t];
}

// in place W[:, :r] = W[:, :cb] * M (cb x r), one thread per row
__global__ void k_right_mult(double *W, int64_t ld, int64_t n, int cb, int r, const double *M) {
  __shared__ double sM[kMaxB * kMaxB];
  if ((int)threadIdx.x < cb * r) sM[threadIdx.x] = M[threadIdx.x];
  __syncthreads();
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double w[kMaxB], o[kMaxB];
#pragma unroll
  for (int j = 0; j < kMaxB; j++) w[j] = j < cb ? W[i + j * ld] : 0.0;
#pragma unroll
  for (int c = 0; c < kMaxB; c++) {
    double s = 0;
#pragma unroll
    for (int j = 0; j < kMaxB; j++)
      if (j < cb && c < r) s += w[j] * sM[j + c * cb];
    o[c] = s;
  }
#pragma unroll
  for (int c = 0; c < kMaxB; c++)
    if (c < r) W[i + c * ld] = o[c];
}

// The small-matrix half of one pass of the two-pass orthonormalisation (orth_small.hpp) on one
// workgroup; the coefficient iterate lives in LDS.  mx_clear: the column maxima that the following
// k_update accumulates (rounding of the finished block) start from zero.
struct DevCtx {
  int tid, nt;
  __device__ void sync() { __syncthreads(); }
};
__global__ __launch_bounds__(512) void k_orth2(OrthSmall a, unsigned long long *mx_clear) {
  __shared__ double sCs[kOrthMaxP * kOrthMaxB];
  __shared__ double sG[kOrthMaxB * kOrthMaxB], sR[kOrthMaxB * kOrthMaxB], sRi[kOrthMaxB * kOrthMaxB],
      sRo[kOrthMaxB * kOrthMaxB], sD[kOrthMaxB * kOrthMaxB], sT[2 * kOrthMaxB + 4];
  a.Cs = sCs;
  a.Gs = sG;
  a.Rs = sR;
  a.Ris = sRi;
  a.Ro = sRo;
  a.Dv = sD;
  a.tmp = sT;
  if (mx_clear && threadIdx.x < kOrthMaxB) mx_clear[threadIdx.x] = 0ull;
  DevCtx cx{(int)threadIdx.x, (int)blockDim.x};
  orth_small(cx, a);
}

// W[i, :cb] <- (W[i, :cb] - Q[i, :p] C) Ri   in place, one thread per row (the tall half of a pass);
// mx != null: also the column maxima of the result (bits of a non-negative double order like u64)
template <int CBT>
__global__ __launch_bounds__(256) void k_update(const double *__restrict__ Q, int64_t ldq, int p,
                                                const double *__restrict__ C, const double *__restrict__ Ri,
                                                int cb, double *W, int64_t ldw, int64_t n,
                                                unsigned long long *mx) {
  constexpr int TP = 128, ROWS = 4;   // a workgroup covers 1024 rows: few atomics on the column maxima
  __shared__ double sS[TP * CBT], sRi[CBT * CBT], smx[4][CBT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int t = tid; t < CBT * CBT; t += 256) {
    const int j = t % CBT, c = t / CBT;
    sRi[t] = (j < cb && c < cb) ? Ri[j + c * cb] : 0.0;
  }
  if (tid < 4 * CBT) smx[tid / CBT][tid % CBT] = 0.0;
  const bool one_tile = p <= TP;
  for (int it = 0; it < ROWS; it++) {
    const int64_t i = ((int64_t)blockIdx.x * ROWS + it) * 256 + tid;
    double acc[CBT];
#pragma unroll
    for (int j = 0; j < CBT; j++) acc[j] = 0;
    for (int a0 = 0; a0 < p; a0 += TP) {
      const int ta = p - a0 < TP ? p - a0 : TP;
      if (!(one_tile && it > 0)) {   // (uniform) the coefficient tile stays in LDS when it is the only one
        __syncthreads();
        for (int t = tid; t < ta * CBT; t += 256) {
          const int a = t / CBT, j = t % CBT;
          sS[t] = j < cb ? C[(a0 + a) + (int64_t)j * p] : 0.0;
        }
        __syncthreads();
      }
      if (i < n) {
        // (unrolled by 8: the eight loads of Q go out together instead of one memory round trip per column)
#pragma unroll 8
        for (int a = 0; a < ta; a++) {
          const double q = Q[i + (int64_t)(a0 + a) * ldq];
#pragma unroll
          for (int j = 0; j < CBT; j++) acc[j] += q * sS[a * CBT + j];
        }
      }
    }
    if (p == 0 && it == 0) __syncthreads();   // sRi / smx are ready
    double w[CBT];
#pragma unroll
    for (int j = 0; j < CBT; j++) w[j] = (i < n && j < cb) ? W[i + j * ldw] - acc[j] : 0.0;
    // one output column at a time (the loop is kept rolled: 16 x 16 products unrolled need 300 registers)
#pragma unroll 1
    for (int c = 0; c < cb; c++) {
      double s = 0;
#pragma unroll
      for (int j = 0; j < CBT; j++) s += w[j] * sRi[j + c * CBT];
      if (i < n) W[i + c * ldw] = s;
      if (mx) {
        double m = fabs(s);
        for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off));
        if (lane == 0) smx[wave][c] = fmax(smx[wave][c], m);
      }
    }
  }
  if (mx) {
    __syncthreads();
    if (tid < cb) {
      const double m = fmax(fmax(smx[0][tid], smx[1][tid]), fmax(smx[2][tid], smx[3][tid]));
      atomicMax(&mx[tid], (unsigned long long)__double_as_longlong(m));
    }
  }
}

// ---- rounding of a finished basis block to the fixed-point grid of the streaming products ----
// (svd_driver.hpp: the products are then exact for the stored vectors).  The scale is the largest
// power of two with absmax * qs <= 0.98 * 2^(8S-1): one notch below the 0.99 the product's own
// quantiser uses, so that re-quantising the rounded vector can only pick the same or a finer grid.
__global__ void k_col_absmax(const double *W, int64_t ld, int64_t n, unsigned long long *mx) {
  const int v = blockIdx.y;
  double m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    m = fmax(m, fabs(W[i + v * ld]));
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off));
  __shared__ double sm[16];
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) sm[wave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < nw; w++) m = fmax(m, sm[w]);
    atomicMax(&mx[v], (unsigned long long)__double_as_longlong(m));
  }
}
__global__ void k_round_cols(double *W, int64_t ld, int64_t n, const unsigned long long *mx, int slices) {
  const int v = blockIdx.y;
  const double m = __longlong_as_double((long long)mx[v]);
  if (!(m > 0)) return;
  int e;
  frexp(ldexp(0.98, 8 * slices - 1) / m, &e);
  const double qs = ldexp(1.0, e - 1), iq = ldexp(1.0, 1 - e);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) W[i + v * ld] = (double)llrint(W[i + v * ld] * qs) * iq;
}

// ---- sample-block layout of a panel for the collectives ------------------------------------
// full: n x cb column-major (ld n).  blk: [rank][column][row of the rank's block], blocks of nr
// rows (the last one zero-padded) — the chunk of rank r is contiguous, which is what
// reduce-scatter / all-gather exchange.
__global__ void k_block(const double *__restrict__ full, int64_t n, int cb, int64_t nr, int world,
                        double *__restrict__ blk) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)world * cb * nr) return;
  const int64_t i = t % nr, j = (t / nr) % cb, r = t / (nr * cb);
  const int64_t gi = r * nr + i;
  blk[t] = gi < n ? full[gi + j * n] : 0.0;
}
__global__ void k_unblock(const double *__restrict__ blk, int64_t n, int cb, int64_t nr,
                          double *__restrict__ full) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * cb) return;
  const int64_t gi = t % n, j = t / n;
  full[t] = blk[((gi / nr) * cb + j) * nr + gi % nr];
}
// ---- the all-gather of a finished basis block as the 16-bit integers it is rounded to (sharded solve, round 4) ----
// mx[v] = max over the ranks of their column maxima (bit patterns of non-negative doubles order like integers)
__global__ void k_max_over_ranks(const unsigned long long *__restrict__ all, int world, int cb,
                                 unsigned long long *__restrict__ mx) {
  const int v = threadIdx.x;
  if (v >= cb) return;
  unsigned long long m = 0;
  for (int r = 0; r < world; r++) m = all[r * cb + v] > m ? all[r * cb + v] : m;
  mx[v] = m;
}
// the rounding of k_round_cols on this rank's rows: the integers go to q (column-major, nr rows), the rounded values
// back into W
template <typename INT>   // int16_t up to 16 bits, int32_t up to 32
__global__ void k_pack_int(double *__restrict__ W, int64_t nr, const unsigned long long *__restrict__ mx, int slices,
                           INT *__restrict__ q) {
  const int v = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nr) return;
  const double m = __longlong_as_double((long long)mx[v]);
  if (!(m > 0)) {
    q[i + v * nr] = 0;
    return;   // (an all-zero column stays as it is, like in k_round_cols)
  }
  int e;
  frexp(ldexp(0.98, 8 * slices - 1) / m, &e);
  const double qs = ldexp(1.0, e - 1), iq = ldexp(1.0, 1 - e);
  const long long k = llrint(W[i + v * nr] * qs);
  q[i + v * nr] = (INT)k;
  W[i + v * nr] = (double)k * iq;
}
// all ranks' integers ([rank][column][row of the block]) -> the rounded block with all n rows (column-major, ld n)
template <typename INT>
__global__ void k_unpack_int(const INT *__restrict__ q, int64_t n, int cb, int64_t nr,
                             const unsigned long long *__restrict__ mx, int slices, double *__restrict__ full) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * cb) return;
  const int64_t gi = t % n, v = t / n;
  const double m = __longlong_as_double((long long)mx[v]);
  double val = 0.0;
  if (m > 0) {
    int e;
    frexp(ldexp(0.98, 8 * slices - 1) / m, &e);
    val = (double)q[((gi / nr) * cb + v) * nr + gi % nr] * ldexp(1.0, 1 - e);
  }
  full[t] = val;
}

// a received segment (rows x cb, ld rows) into rows [r0, r0 + rows) of the panel W (ld nr)
__global__ void k_place_rows(const double *__restrict__ src, int64_t rows, int cb, int64_t r0, int64_t nr,
                             double *__restrict__ W) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * cb) return;
  W[r0 + t % rows + (t / rows) * nr] = src[t];
}
// W (nr x cb, ld nr) = rows [row0, row0 + nr) of full (n x cb, ld n), zero past n
__global__ void k_take_rows(const double *__restrict__ full, int64_t n, int cb, int64_t nr, int64_t row0,
                            double *__restrict__ W) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nr * cb) return;
  const int64_t i = t % nr, j = t / nr;
  W[t] = row0 + i < n ? full[row0 + i + j * n] : 0.0;
}

// ---- the launches of the panel kernels (svd_panel.hpp) --------------------------------------------------------
// One free function per launch: grid, block, template choice and LDS size live here and nowhere else, so that the
// backend (svd.hip) and the kernel-level test entries at the end of this file (bsn_panel_*) run the same launches.
void panel_random(hipStream_t st, double *W, int64_t ld, int64_t n, int b, uint32_t seed, int64_t row0, int64_t n_total) {
  hipLaunchKernelGGL(k_random, dim3((unsigned)((n + 255) / 256), b), dim3(256), 0, st, W, ld, n, b, seed, row0, n_total);
}
void panel_put_block(hipStream_t st, double *M, int ld, int r, const double *src) {
  hipLaunchKernelGGL(k_put_block, dim3((unsigned)((r * r + 255) / 256)), dim3(256), 0, st, M, ld, r, src);
}
// dC (p x cb, leading dimension ldc) = A[:, :p]' B[:, :cb] for operands with `rows` rows; cb <= 32
void panel_gemm_tn(hipStream_t st, const double *A, int64_t lda, int p, const double *B, int64_t ldb, int cb, int64_t rows,
                   double *dC, int ldc, double *partial) {
  if (p <= 0 || cb <= 0) return;
  dim3 grid((unsigned)((p + 15) / 16), (unsigned)((rows + kGemmRows - 1) / kGemmRows));
  const int nt = (cb + 15) / 16;
  if (nt == 1)
    hipLaunchKernelGGL((k_gemm_tn<1>), grid, dim3(256), 0, st, A, lda, p, B, ldb, cb, rows, partial);
  else if (nt == 2)
    hipLaunchKernelGGL((k_gemm_tn<2>), grid, dim3(256), 0, st, A, lda, p, B, ldb, cb, rows, partial);
  else
    fail("internal: panel product with %d columns", cb);
  hipLaunchKernelGGL(k_gemm_tn_reduce, dim3(grid.x, nt), dim3(1024), 0, st, partial, (int)grid.y, (int)grid.x, p, cb, dC, ldc);
}
void panel_gemm_nn(hipStream_t st, const double *Q, int64_t ldq, int p, const double *S, int nc, const double *In, int64_t ldi,
                   double alpha, double beta, double *Out, int64_t ldo, int64_t n) {
  hipLaunchKernelGGL(k_gemm_nn, dim3((unsigned)((n + 255) / 256)), dim3(256), kTP * kMaxB * 8, st, Q, ldq, p, S, nc, In, ldi,
                     alpha, beta, Out, ldo, n);
}
void panel_right_mult(hipStream_t st, double *W, int64_t ld, int64_t n, int cb, int r, const double *M) {
  hipLaunchKernelGGL(k_right_mult, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, W, ld, n, cb, r, M);
}
void panel_update(hipStream_t st, const double *Q, int64_t ldq, int p, const double *C, const double *Ri, int cb, double *W,
                  int64_t ldw, int64_t n, unsigned long long *mx) {
  const dim3 rows((unsigned)((n + 1023) / 1024));
  if (cb <= 8)
    hipLaunchKernelGGL((k_update<8>), rows, dim3(256), 0, st, Q, ldq, p, C, Ri, cb, W, ldw, n, mx);
  else
    hipLaunchKernelGGL((k_update<16>), rows, dim3(256), 0, st, Q, ldq, p, C, Ri, cb, W, ldw, n, mx);
}
void panel_orth2(hipStream_t st, const OrthSmall &a, unsigned long long *mx_clear) {
  hipLaunchKernelGGL(k_orth2, dim3(1), dim3(512), 0, st, a, mx_clear);
}
// wide: 256 workgroups per column (a whole panel on one GPU), else 64 (a rank's sample block)
void panel_col_absmax(hipStream_t st, const double *X, int64_t ld, int64_t n, int cb, unsigned long long *mx, bool wide) {
  hipLaunchKernelGGL(k_col_absmax, dim3(wide ? 256 : 64, cb), dim3(1024), 0, st, X, ld, n, mx);
}
void panel_round_cols(hipStream_t st, double *X, int64_t ld, int64_t n, int cb, const unsigned long long *mx, int slices) {
  hipLaunchKernelGGL(k_round_cols, dim3((unsigned)((n + 255) / 256), cb), dim3(256), 0, st, X, ld, n, mx, slices);
}
void panel_block(hipStream_t st, const double *full, int64_t n, int cb, int64_t nr, int world, double *blk) {
  const int64_t tot = (int64_t)world * cb * nr;
  hipLaunchKernelGGL(k_block, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, full, n, cb, nr, world, blk);
}
void panel_unblock(hipStream_t st, const double *blk, int64_t n, int cb, int64_t nr, double *full) {
  hipLaunchKernelGGL(k_unblock, dim3((unsigned)((n * cb + 255) / 256)), dim3(256), 0, st, blk, n, cb, nr, full);
}
void panel_place_rows(hipStream_t st, const double *src, int64_t rows, int cb, int64_t r0, int64_t nr, double *W) {
  hipLaunchKernelGGL(k_place_rows, dim3((unsigned)((rows * cb + 255) / 256)), dim3(256), 0, st, src, rows, cb, r0, nr, W);
}
void panel_take_rows(hipStream_t st, const double *full, int64_t n, int cb, int64_t nr, int64_t row0, double *W) {
  hipLaunchKernelGGL(k_take_rows, dim3((unsigned)((nr * cb + 255) / 256)), dim3(256), 0, st, full, n, cb, nr, row0, W);
}
void panel_max_over_ranks(hipStream_t st, const unsigned long long *all, int world, int cb, unsigned long long *mx) {
  hipLaunchKernelGGL(k_max_over_ranks, dim3(1), dim3(64), 0, st, all, world, cb, mx);
}
// int16 up to 16 bits (slices <= 2), int32 up to 32: q is the rank's [column][row] block of integers
void panel_pack_int(hipStream_t st, double *W, int64_t nr, int cb, const unsigned long long *mx, int slices, void *q) {
  const dim3 gp((unsigned)((nr + 255) / 256), cb);
  if (slices <= 2)
    hipLaunchKernelGGL((k_pack_int<int16_t>), gp, dim3(256), 0, st, W, nr, mx, slices, (int16_t *)q);
  else
    hipLaunchKernelGGL((k_pack_int<int32_t>), gp, dim3(256), 0, st, W, nr, mx, slices, (int32_t *)q);
}
void panel_unpack_int(hipStream_t st, const void *q_all, int64_t n, int cb, int64_t nr, const unsigned long long *mx, int slices,
                      double *full) {
  const dim3 gu((unsigned)((n * cb + 255) / 256));
  if (slices <= 2)
    hipLaunchKernelGGL((k_unpack_int<int16_t>), gu, dim3(256), 0, st, (const int16_t *)q_all, n, cb, nr, mx, slices, full);
  else
    hipLaunchKernelGGL((k_unpack_int<int32_t>), gu, dim3(256), 0, st, (const int32_t *)q_all, n, cb, nr, mx, slices, full);
}

}  // namespace bsn

using namespace bsn;

// ---- kernel-level entries for the tests (tests/test_gpu_svd_panel.py) --------------------------------------------------
// The panel kernels one at a time, through the launch functions the backend uses, on caller-owned device memory
// (bsn_malloc / bsn_memcpy_h2d / bsn_memcpy_d2h).  Null stream, synchronised before returning.  Every argument is checked
// on the host before the first launch: no call can launch out of bounds.
namespace bsn {
namespace {
constexpr int kPanelMaxP = 4096;   // basis columns the entries accept (the solve's cap is far below)
void panel_done() {
  BSN_HIP(hipGetLastError());
  BSN_HIP(hipStreamSynchronize(nullptr));
}
// rows of a "rank's" sample block in the one-device restatements of the sharded exchanges
int64_t panel_block_rows(int64_t n, int world) { return ((n + world - 1) / world + 3) / 4 * 4; }
}  // namespace
}  // namespace bsn

extern "C" {

int bsn_panel_gemm_tn(const double *d_A, int64_t lda, int32_t p, const double *d_B, int64_t ldb, int32_t cb, int64_t rows,
                      double *d_C, int32_t ldc) {
  return guarded([&] {
    require_gpu();
    if (!d_A || !d_B || !d_C) fail("bsn_panel_gemm_tn: null pointer");
    if (cb > 32) fail("internal: panel product with %d columns", (int)cb);
    if (p < 1 || p > kPanelMaxP || cb < 1 || rows < 1 || rows > ((int64_t)1 << 31) || lda < rows || ldb < rows || ldc < p)
      fail("bsn_panel_gemm_tn: dimensions");
    DevBuf<double> partial;
    partial.ensure(panel_partial_count(rows, p));
    panel_gemm_tn(nullptr, d_A, lda, p, d_B, ldb, cb, rows, d_C, ldc, partial.p);
    panel_done();
  });
}

int bsn_panel_gemm_nn(const double *d_Q, int64_t ldq, int32_t p, const double *d_S, int32_t nc, const double *d_In, int64_t ldi,
                      double alpha, double beta, double *d_Out, int64_t ldo, int64_t n) {
  return guarded([&] {
    require_gpu();
    if (!d_Q || !d_S || !d_Out || (alpha != 0.0 && !d_In)) fail("bsn_panel_gemm_nn: null pointer");
    if (p < 1 || p > kPanelMaxP || nc < 1 || nc > kMaxB || n < 1 || n > ((int64_t)1 << 31) || ldq < n || ldo < n ||
        (alpha != 0.0 && ldi < n))
      fail("bsn_panel_gemm_nn: dimensions (at most %d columns)", kMaxB);
    panel_gemm_nn(nullptr, d_Q, ldq, p, d_S, nc, d_In, ldi, alpha, beta, d_Out, ldo, n);
    panel_done();
  });
}

int bsn_panel_right_mult(double *d_W, int64_t ld, int64_t n, int32_t cb, int32_t r, const double *d_M) {
  return guarded([&] {
    require_gpu();
    if (!d_W || !d_M) fail("bsn_panel_right_mult: null pointer");
    if (cb < 1 || cb > kMaxB || r < 1 || r > kMaxB || cb * r > 256 || n < 1 || n > ((int64_t)1 << 31) || ld < n)
      fail("bsn_panel_right_mult: dimensions (at most %d columns)", kMaxB);
    panel_right_mult(nullptr, d_W, ld, n, cb, r, d_M);
    panel_done();
  });
}

int bsn_panel_update(const double *d_Q, int64_t ldq, int32_t p, const double *d_C, const double *d_Ri, int32_t cb, double *d_W,
                     int64_t ldw, int64_t n, uint64_t *d_mx) {
  return guarded([&] {
    require_gpu();
    if (!d_Ri || !d_W || (p > 0 && (!d_Q || !d_C))) fail("bsn_panel_update: null pointer");
    if (p < 0 || p > kPanelMaxP || cb < 1 || cb > kMaxB || n < 1 || n > ((int64_t)1 << 31) || ldw < n || (p > 0 && ldq < n))
      fail("bsn_panel_update: dimensions (at most %d columns)", kMaxB);
    panel_update(nullptr, d_Q, ldq, p, d_C, d_Ri, cb, d_W, ldw, n, (unsigned long long *)d_mx);
    panel_done();
  });
}

int bsn_panel_round_cols(double *d_X, int64_t ld, int64_t rows, int32_t cb, int32_t slices, int32_t have_mx, uint64_t *d_mx,
                         int32_t wide_grid) {
  return guarded([&] {
    require_gpu();
    if (!d_X || !d_mx) fail("bsn_panel_round_cols: null pointer");
    if (cb < 1 || cb > kMaxB || rows < 1 || rows > ((int64_t)1 << 31) || ld < rows || slices < 1 || slices > 7)
      fail("bsn_panel_round_cols: dimensions (at most %d columns, 1 to 7 slices)", kMaxB);
    unsigned long long *mx = (unsigned long long *)d_mx;
    if (!have_mx) {
      BSN_HIP(hipMemsetAsync(mx, 0, (size_t)cb * 8, nullptr));
      panel_col_absmax(nullptr, d_X, ld, rows, cb, mx, wide_grid != 0);
    }
    panel_round_cols(nullptr, d_X, ld, rows, cb, mx, slices);
    panel_done();
  });
}

// returns -1 where HipSvdBackend::fused would (the caller takes the step-by-step path), 0 when the queue ran
int bsn_panel_fused_orth(double *d_QW, int64_t nr, int32_t p, int32_t p0, int32_t cb, int32_t iters, double *flag_out,
                         double *Rout_out) {
  bool unsupported = false;
  const int rc = guarded([&] {
    require_gpu();
    if (!d_QW || !flag_out || !Rout_out) fail("bsn_panel_fused_orth: null pointer");
    if (p < 0 || cb < 1 || nr < 1 || nr > ((int64_t)1 << 31) || iters < 0 || iters > 8)
      fail("bsn_panel_fused_orth: dimensions");
    if (cb > kMaxB || p + cb > kOrthMaxP) {
      unsupported = true;
      return;
    }
    // the newest basis block is the cb columns in front of the panel, as in a solve
    if ((p == 0 && p0 != 0) || (p > 0 && (p < cb || p0 != p - cb))) fail("bsn_panel_fused_orth: p0 must be p - cb");
    constexpr int B2 = kMaxB * kMaxB;
    const size_t pc = (size_t)p * cb, hg = (size_t)(p + cb) * cb;
    DevBuf<double> dorth, dM, partial;
    dorth.ensure((size_t)16 + 3 * B2 + 7 * (size_t)(p + cb + 4) * kMaxB);
    dM.ensure((size_t)kOrthMaxP * kOrthMaxP);
    partial.ensure(panel_partial_count(nr, p + cb));
    hipStream_t st = nullptr;
    double *Q = d_QW, *Wc = d_QW + (int64_t)p * nr;
    // the device copy of Q'Q as the earlier steps of a solve would have left it (the newest block is folded in again below)
    BSN_HIP(hipMemsetAsync(dM.p, 0, (size_t)kOrthMaxP * kOrthMaxP * 8, st));
    for (int c0 = 0; c0 < p; c0 += 2 * kMaxB)
      panel_gemm_tn(st, Q, nr, p, Q + (int64_t)c0 * nr, nr, std::min(2 * kMaxB, p - c0), nr, dM.p + (size_t)c0 * kOrthMaxP,
                    kOrthMaxP, partial.p);
    // ---- the queue of HipSvdBackend::fused: the same arena, the same order ----
    unsigned long long *mx = (unsigned long long *)dorth.p;
    double *flag = dorth.p + 16, *dRout = flag + 1, *dZtZ = dRout + B2, *X = dZtZ + pc, *HG1 = X + (p > 0 ? hg : 0),
           *HG2 = HG1 + hg, *C = HG2 + hg, *Ct = C + pc, *Ri = Ct + pc;
    const double *A0 = p > 0 ? Q : Wc;
    BSN_HIP(hipMemsetAsync(flag, 0, (size_t)(1 + B2) * 8, st));
    OrthSmall a;
    a.p = p;
    a.cb = cb;
    a.p0 = p0;
    a.QtQ = p > 0 ? X : nullptr;
    a.ldq = p + cb;
    a.M = dM.p;
    a.ldm = kOrthMaxP;
    a.C = C;
    a.Ct = Ct;
    a.Ri = Ri;
    a.Rout = dRout;
    a.flag = flag;
    a.iters = iters;
    a.Cs = a.Gs = a.Rs = a.Ris = a.Ro = a.Dv = a.tmp = nullptr;
    for (int pass = 0; pass < 2; pass++) {
      double *HG = pass == 0 ? HG1 : HG2;
      if (pass == 0 && p > 0)
        panel_gemm_tn(st, Q, nr, p + cb, Q + (int64_t)p0 * nr, nr, 2 * cb, nr, X, p + cb, partial.p);
      else
        panel_gemm_tn(st, A0, nr, p + cb, Wc, nr, cb, nr, HG, p + cb, partial.p);
      a.pass = pass;
      a.HG = HG;
      unsigned long long *mxp = pass == 1 ? mx : nullptr;
      panel_orth2(st, a, mxp);
      panel_update(st, Q, nr, p, C, Ri, cb, Wc, nr, nr, mxp);
    }
    panel_done();
    std::vector<double> h((size_t)1 + B2);
    BSN_HIP(hipMemcpy(h.data(), flag, h.size() * 8, hipMemcpyDeviceToHost));
    *flag_out = h[0];
    for (int t = 0; t < cb * cb; t++) Rout_out[t] = h[1 + (size_t)t];
  });
  return rc != 0 ? rc : (unsupported ? -1 : 0);
}

int bsn_panel_compact_gather(const double *d_full, int64_t n, int32_t cb, int32_t world, int32_t slices, double *d_out) {
  return guarded([&] {
    require_gpu();
    if (!d_full || !d_out) fail("bsn_panel_compact_gather: null pointer");
    if (n < 1 || n > ((int64_t)1 << 31) || cb < 1 || cb > kMaxB || world < 1 || world > 64 || slices < 1 || slices > 4)
      fail("bsn_panel_compact_gather: dimensions (at most %d columns, 64 ranks, 4 slices)", kMaxB);
    const int64_t nr = panel_block_rows(n, world);
    const size_t blk = (size_t)nr * cb, isz = slices <= 2 ? 2 : 4;
    DevBuf<double> Wr, q_all;
    DevBuf<unsigned long long> gmax, mx;
    Wr.ensure(blk * world);
    q_all.ensure((blk * world * isz + 7) / 8);
    gmax.ensure((size_t)world * kMaxB);
    mx.ensure(kMaxB);
    hipStream_t st = nullptr;
    BSN_HIP(hipMemsetAsync(gmax.p, 0, (size_t)world * kMaxB * 8, st));
    for (int r = 0; r < world; r++) {
      panel_take_rows(st, d_full, n, cb, nr, (int64_t)r * nr, Wr.p + blk * r);
      panel_col_absmax(st, Wr.p + blk * r, nr, nr, cb, gmax.p + (size_t)r * cb, false);
    }
    panel_max_over_ranks(st, gmax.p, world, cb, mx.p);
    for (int r = 0; r < world; r++)
      panel_pack_int(st, Wr.p + blk * r, nr, cb, mx.p, slices, (char *)q_all.p + blk * r * isz);
    panel_unpack_int(st, q_all.p, n, cb, nr, mx.p, slices, d_out);
    panel_done();
  });
}

int bsn_panel_block_roundtrip(const double *d_full, int64_t n, int32_t cb, int32_t world, double *d_out, double *d_placed) {
  return guarded([&] {
    require_gpu();
    if (!d_full || !d_out || !d_placed) fail("bsn_panel_block_roundtrip: null pointer");
    if (n < 1 || n > ((int64_t)1 << 31) || cb < 1 || cb > kMaxB || world < 1 || world > 64)
      fail("bsn_panel_block_roundtrip: dimensions (at most %d columns, 64 ranks)", kMaxB);
    const int64_t nr = panel_block_rows(n, world);
    DevBuf<double> blk;
    blk.ensure((size_t)world * cb * nr);
    hipStream_t st = nullptr;
    panel_block(st, d_full, n, cb, nr, world, blk.p);
    panel_unblock(st, blk.p, n, cb, nr, d_out);
    // every rank's chunk (nr x cb) as a received segment into its rows of a panel with world * nr rows
    for (int r = 0; r < world; r++)
      panel_place_rows(st, blk.p + (size_t)r * cb * nr, nr, cb, (int64_t)r * nr, (int64_t)world * nr, d_placed);
    panel_done();
  });
}

}  // extern "C"
