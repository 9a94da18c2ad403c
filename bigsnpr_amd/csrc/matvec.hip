// matvec.hip — the streaming products of the scaled genotype matrix on gfx950.
//
//   op_prod : Y = A~ X   (replaces bed_pMatVec4,  src/bed-prod-vec.cpp:15-54)
//   op_cprod: Z = A~' X  (replaces bed_cpMatVec4, src/bed-prod-vec.cpp:59-97)
//   with A~[i,j] = (g - center_j)/scale_j, missing -> 0 (src/bed-acc.h:98-111).
//
// Design: both products are HBM-bound on the 2-bit image but a
// fp64 VALU formulation needs ~7 lane-ops per genotype, 2x what the chip can issue at
// 6 TB/s.  So the multiply-accumulate is moved to the i8 MFMA pipe, exactly:
//   - the fp64 panel is scaled per vector to a fixed-point integer of 8*S bits and split
//     into S balanced base-256 digits (int8 "slices");
//   - the image holds device codes (bsn_internal.hpp: 0, 1, 2 = allele count, 3 = missing), so
//     the masked 2-bit field IS the int8 operand of the genotype plane `code` in {0,1,2,3}
//     (7 shift/and per 16 genotypes, no look-up); one v_perm_b32 byte look-up per register
//     gives the plane na in {0,1};
//   - v_mfma_i32_16x16x64_i8 accumulates  P' = sum code*digit  and  Q = sum na*digit  in int32,
//     which is exact; the 3 of a missing value leaves through Q (g0 = code - 3 na) and the
//     digits are recombined in fp64 in a finalize kernel together with the centre/scale algebra
//         A~' x = (P - c (Sx - Q)) / s,      P = P' - 3 Q = sum g0 x, Q = sum na x, Sx = sum x
//         A~ x  = sum_j code w_j + sum_j na (c w - 3 w)_j - sum_j (c w)_j,   w = x / s.
//   Results are bit-reproducible (integer sums are order-independent).
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>

#include "bsn_internal.hpp"
#include "byte_plan.hpp"
#include "prod_plan.hpp"
#include "prodt_sparse.hpp"
#include <type_traits>

namespace bsn {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));

// Every launch of a streaming kernel notes WHICH instantiation it was: prof_end files it under the launch's kind and
// bsn_bed_streaming_kernels reports the names, so that a committed counter record (profiles/pmc_traffic.json) can be
// matched against the kernels the running build really launches (bench.py: roofline.traffic).
static thread_local const void *g_last_kernel = nullptr;
#define BSN_KLAUNCH(kern, ...)                 \
  do {                                         \
    g_last_kernel = (const void *)(kern);      \
    hipLaunchKernelGGL(kern, __VA_ARGS__);     \
  } while (0)

// byte look-up: result byte k = lut byte (sel byte k), sel bytes in 0..3.  The LUT is
// given as both sources so the result does not depend on the S0/S1 order of v_perm_b32.
__device__ __forceinline__ uint32_t lut4(uint32_t lut, uint32_t sel) {
  return __builtin_amdgcn_perm(lut, lut, sel);
}
// byte permute of the 8 bytes {hi:lo}; selector k picks lo.byte[k] for k<4, hi.byte[k-4]
// otherwise (verified by bsn_selftest)
__device__ __forceinline__ uint32_t perm8(uint32_t hi, uint32_t lo, uint32_t sel) {
  return __builtin_amdgcn_perm(hi, lo, sel);
}

// device code -> plane value (byte k of the constant = value of code k)
constexpr uint32_t kLutG0 = 0x00020100u;   // {0,1,2,0}
constexpr uint32_t kLutNA = 0x01000000u;   // {0,0,0,1}
constexpr uint32_t kLutHom2 = 0x00010000u; // {0,0,1,0}
constexpr uint32_t kLutHet = 0x00000100u;  // {0,1,0,0}
constexpr uint32_t kLutRaw = 0xFFFFFFFFu;  // marker: the plane is the code itself (no look-up)

// ---- per-vector metadata -------------------------------------------------------
struct VecMeta {
  unsigned long long absmax_bits;  // bits of max |value| (non-negative doubles order like u64)
  long long sum_hi, sum_lo;        // sum of the fixed-point integers, split at bit 24
  long long sum2_hi, sum2_lo;      // same for the second plane (c*w) in op_prod
  unsigned long long nonfinite;    // count of non-finite inputs
  double qscale;                   // fixed-point scale actually used
  double pad;
};
static_assert(sizeof(VecMeta) == 64, "VecMeta layout");

__global__ void k_meta_clear(VecMeta *meta, int nvec) {
  int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < nvec) {
    VecMeta z = {};
    meta[v] = z;
  }
}

// rows scatter: xfull[rows[i], v] += x[i, v]   (duplicates allowed -> atomics)
__global__ void k_scatter_rows(const double *X, int64_t ldx, const int32_t *rows, int64_t n,
                               double *xfull, int64_t ldf) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int v = blockIdx.y;
  if (i >= n) return;
  atomicAdd(&xfull[(int64_t)rows[i] + v * ldf], X[i + v * ldx]);
}

// mode 0 (cprod): value = X[k, v]                       for k < len
// mode 1 (prod) : value a = X[k, v]/scale[k], b = c*a; the digit planes hold a and b - 3a
// mode 2 (prod, raw plane weights): a = X[k, v], b = center[k, v] (a second panel)
// vstep / voff / raw3: the value of a genotype is voff + vstep k (2-bit image: k = allele count, 1 / 0);
// mode 1 quantises a = vstep X / scale and b = (c - voff) X / scale; raw3: the k plane holds 3 for a
// missing value (raw 2-bit codes), so the second digit plane carries b - 3 a
// Writes the maximum (and the number of non-finite inputs) of its slice to part[v][blockIdx.x][2]: k_quant
// combines the slices itself, so the quantisation of a panel is two launches (round 2: five — clear, maximum
// with atomics, scale, memset of the digits, digits).  Workgroup 0 of a vector also clears the sums that
// k_quant accumulates.
__global__ void k_absmax(const double *X, int64_t ldx, int64_t len, const double *center,
                         const double *scale, int mode, VecMeta *meta, double *part, double vstep, double voff,
                         int raw3) {
  int v = blockIdx.y;
  double mx = 0;
  unsigned long long bad = 0;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < len;
       k += (int64_t)gridDim.x * blockDim.x) {
    double a = X[k + v * ldx];
    if (mode == 1) {
      double s = scale ? scale[k] : 1.0, c = center ? center[k] : 0.0;
      a = a / s;
      const double b = (c - voff) * a;
      a *= vstep;
      const double b3 = fabs(b - 3.0 * a);  // the second digit plane (missing-value plane weights)
      if (!(fabs(b) <= 1.79e308)) bad++; else mx = fmax(mx, fabs(b));
      if (raw3 && b3 <= 1.79e308) mx = fmax(mx, b3);
    } else if (mode == 2) {  // raw second plane: center[] is W2 (same shape as X)
      double b = center ? fabs(center[k + v * ldx]) : 0.0;
      if (!(b <= 1.79e308)) bad++; else mx = fmax(mx, b);
    }
    a = fabs(a);
    if (!(a <= 1.79e308)) bad++; else mx = fmax(mx, a);
  }
  for (int off = 32; off > 0; off >>= 1) {
    mx = fmax(mx, __shfl_down(mx, off));
    bad += __shfl_down(bad, off);
  }
  // one atomic per workgroup: thousands of same-address 64-bit atomics cost ~20 ns each
  __shared__ double smx[16];
  __shared__ unsigned long long sbad[16];
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    smx[wave] = mx;
    sbad[wave] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < nw; w++) {
      mx = fmax(mx, smx[w]);
      bad += sbad[w];
    }
    double *pp = part + ((int64_t)v * gridDim.x + blockIdx.x) * 2;
    pp[0] = mx;
    pp[1] = (double)bad;
    if (blockIdx.x == 0) meta[v].sum_hi = meta[v].sum_lo = meta[v].sum2_hi = meta[v].sum2_lo = 0;
  }
}

// One wave quantises 1024 consecutive k of one vector; a thread ends up with 16 of them as S
// digit rows of 16 bytes.
// Layout: q[(k/16) * (nplanes*ncol) + plane*ncol + col][16 B], col = v*S + s.
// PERM = 1 (cprod operand): sample e of the 16 is stored at byte (e%4)*4 + e/4, the
// order in which k_cprod's decode emits them;  PERM = 0 (prod operand): natural.
// PERM = 2 (operand of k_prodT's sparse form, prodt_sparse.hpp; mode 1 only): natural order, the two planes
// byte-interleaved as (A_e, B_e) — row 0 of the pair holds variants 0..7, row 1 variants 8..15 — and the second plane
// holds B itself, not B - 3 A: a missing genotype selects the B slot alone, and 3 A + (B - 3 A) = B.  The sums and the
// scale are those of the other orders (k_absmax keeps the |b - 3 a| term), so qscale and sum2 do not change.
// The values are read coalesced and handed over through LDS (row stride 17 against bank
// conflicts); the digit bytes are packed in registers (S and PERM are compile-time).
template <int S, int PERM>
__global__ __launch_bounds__(64) void k_quant(const double *__restrict__ X, int64_t ldx, int64_t len,
                                              int64_t len_pad, const double *__restrict__ center,
                                              const double *__restrict__ scale, int mode, int ncol,
                                              VecMeta *meta, int8_t *__restrict__ q, double vstep, double voff,
                                              int raw3, const double *__restrict__ part, int gx) {
  __shared__ double sa[64 * 17], sb[64 * 17];
  const int tid = threadIdx.x, v = blockIdx.y;
  const int64_t kb = (int64_t)blockIdx.x * 64 + tid;  // 16-block index of this thread
  const int nplanes = mode >= 1 ? 2 : 1;
  // fixed-point scale of the vector from the slice maxima of k_absmax (gx == 0: the values are
  // integers already, scale 1): the largest power of two with absmax * qs <= 0.99 * 2^(8S-1), so that
  // x * qs is exact and only the rounding to an integer errs
  double qs = 1.0;
  if (gx > 0) {
    double mx = 0, bad = 0;
    for (int t = tid; t < gx; t += 64) {
      mx = fmax(mx, part[((int64_t)v * gx + t) * 2]);
      bad += part[((int64_t)v * gx + t) * 2 + 1];
    }
    for (int off = 32; off > 0; off >>= 1) {
      mx = fmax(mx, __shfl_xor(mx, off));
      bad += __shfl_xor(bad, off);
    }
    qs = 0.0;
    if (mx > 0) {
      int e;
      frexp(ldexp(0.99, 8 * S - 1) / mx, &e);
      qs = ldexp(1.0, e - 1);
    }
    if (blockIdx.x == 0 && tid == 0) {
      meta[v].absmax_bits = (unsigned long long)__double_as_longlong(mx);
      meta[v].nonfinite = (unsigned long long)bad;
    }
  }
  if (blockIdx.x == 0 && tid == 0) meta[v].qscale = qs;
  // all 16 x (1..3) loads of a thread are issued before the first use
  double xa[16], xc[16], xs[16];
#pragma unroll
  for (int it = 0; it < 16; it++) {
    const int64_t k = (int64_t)blockIdx.x * 1024 + it * 64 + tid;
    const bool in = k < len;
    xa[it] = in ? X[k + v * ldx] : 0.0;
    xc[it] = 0.0;
    xs[it] = 1.0;
    if (mode == 1) {
      if (in && scale) xs[it] = scale[k];
      if (in && center) xc[it] = center[k];
    } else if (mode == 2) {
      if (in && center) xc[it] = center[k + v * ldx];
    }
  }
#pragma unroll
  for (int it = 0; it < 16; it++) {
    const int t = it * 64 + tid;
    double a = xa[it], b = 0;
    if (mode == 1) {
      a = a / xs[it];
      b = (xc[it] - voff) * a;
      a *= vstep;
    } else if (mode == 2) {
      b = xc[it];
    }
    if (!(fabs(a) <= 1.79e308)) a = 0;
    if (!(fabs(b) <= 1.79e308)) b = 0;
    sa[t + (t >> 4)] = a * qs;
    sb[t + (t >> 4)] = b * qs;
  }
  __syncthreads();
  long long shi = 0, slo = 0, shi2 = 0, slo2 = 0;
  if (kb * 16 < len_pad) {
    uint32_t pk[2][S][4];
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
      for (int s = 0; s < S; s++)
#pragma unroll
        for (int w = 0; w < 4; w++) pk[p][s][w] = 0;
#pragma unroll
    for (int e = 0; e < 16; e++) {
      long long A = llrint(sa[tid * 17 + e]), B = llrint(sb[tid * 17 + e]);
      shi += A >> 24; slo += A & 0xFFFFFF;
      shi2 += B >> 24; slo2 += B & 0xFFFFFF;
      // scaled product: the genotype plane is the raw code (3 for a missing value), so the
      // missing-value plane carries c w - 3 w, in exact integers: 3 A + (B - 3 A) - B == 0
      if ((raw3 & 1) && PERM != 2) B -= 3 * A;
      const int pos = PERM == 1 ? ((e & 3) * 4 + (e >> 2)) : e;
#pragma unroll
      for (int s = 0; s < S; s++) {
        const int8_t da = (int8_t)(A & 0xFF), db = (int8_t)(B & 0xFF);
        A = (A - da) >> 8;
        B = (B - db) >> 8;
        if constexpr (PERM == 2) {
          const int r = prodt_sparse_row(e), ba = prodt_sparse_byte(e, 0), bb = prodt_sparse_byte(e, 1);
          pk[r][s][ba >> 2] |= (uint32_t)(uint8_t)da << (8 * (ba & 3));
          pk[r][s][bb >> 2] |= (uint32_t)(uint8_t)db << (8 * (bb & 3));
        } else {
          pk[0][s][pos >> 2] |= (uint32_t)(uint8_t)da << (8 * (pos & 3));
          pk[1][s][pos >> 2] |= (uint32_t)(uint8_t)db << (8 * (pos & 3));
        }
      }
    }
    for (int p = 0; p < nplanes; p++)
#pragma unroll
      for (int s = 0; s < S; s++) {
        const int col = v * S + s;
        int8_t *dst = q + ((kb * nplanes + p) * ncol + col) * 16;
        *(uint4 *)dst = p == 0 ? uint4{pk[0][s][0], pk[0][s][1], pk[0][s][2], pk[0][s][3]}
                               : uint4{pk[1][s][0], pk[1][s][1], pk[1][s][2], pk[1][s][3]};
      }
  }
  for (int off = 32; off > 0; off >>= 1) {
    shi += __shfl_down(shi, off); slo += __shfl_down(slo, off);
    shi2 += __shfl_down(shi2, off); slo2 += __shfl_down(slo2, off);
  }
  if (tid == 0) {
    atomicAdd((unsigned long long *)&meta[v].sum_hi, (unsigned long long)shi);
    atomicAdd((unsigned long long *)&meta[v].sum_lo, (unsigned long long)slo);
    if (mode >= 1) {
      atomicAdd((unsigned long long *)&meta[v].sum2_hi, (unsigned long long)shi2);
      atomicAdd((unsigned long long *)&meta[v].sum2_lo, (unsigned long long)slo2);
    }
  }
}

// ---------------------------------------------------------------------------
// k_cprod: contraction over samples.  One wave owns 32 variants (two 16-row MFMA tiles)
// for the whole sample range; the 8 waves of a workgroup share the digit panel of the
// current sample chunk through LDS.  Per 16 B of a variant row a lane does 4 K-steps of
// {decode 15 VALU, NPLANE*NB MFMA, NB ds_read_b128}.
//   A operand: lane l -> variant row (l&15), k-group (l>>4): 16 samples of that variant
//   B operand: lane l -> digit column (l&15), same 16 samples (from LDS)
//   D        : lane l -> column (l&15), rows 4*(l>>4)+r
// RAW0: plane 0 is the device code itself (no look-up).  STATS: the per-variant counts of the
// codes 1, 2 and missing over all samples ride along (popcounts on the raw dwords; the first
// crossproduct pass of a solve, which thereby replaces the separate statistics pass).
// CONTIG: the variants are col0 .. col0+m-1; the genotype loads are then buffer loads with a
// scalar descriptor based at the workgroup's first row, one 32-bit lane offset per tile and a scalar
// chunk offset, so that addressing costs no VALU (global loads spend a 64-bit add on each).
// TAG only changes the kernel's name: the launches of the warm start (a fraction of the variants) run as
// <..., TAG = 1> so that a kernel trace does not average them into the full passes.
// TILED (with CONTIG, col0 a multiple of 64): `img` is the streaming-layout copy (bsn_internal.hpp): variant
// a, byte o of its row at ((a >> 6) * (pitch >> 8) + (o >> 8)) * 16384 + (a & 63) * 256 + (o & 255).
// NASKIP (round 5; RAW0 with two planes): the missing-value plane of a K-step — half its MFMAs and four of its
// decode instructions — is only issued when one of the 64 samples x 16 variants of the step carries a missing code:
// a wave-uniform branch on the ballot of (w & w >> 1 & 0x5555...).  The sums are the same integers (the plane of a
// step without a missing code is zero).  Chosen by the host from the measured share of such steps (op_na_blocks):
// at 1 % scattered missing values no step is free and the branch only costs; on nearly complete or batch-structured
// data most are.
// The grid (CONTIG on the plain image, one or two planes without counting: GEO below): the blocks of variants that fill whole
// rounds of the CUs run as ever — one workgroup, all chunks of samples, sums into acc_out; the blocks beyond the last whole
// round (162 of 1 954 at 1M variants on 256 CUs, where 94 CUs used to idle through the eighth round; all 245 of a warm-start
// launch) are cut along the samples into slabs, launched last, whose int32 sums go to `part_out` and are added by
// k_cprod_final (prod_plan.hpp: plan_cprod, cprod_slab).  BSN_CPROD_ONE_SPLIT=1: every block a whole-round block.
template <int NB, int NPLANE, int KC, bool RAW0, bool STATS, bool CONTIG, int TILES = 2, int WAVES = 8, int MINW = 1,
          int TAG = 0, bool TILED = false, int SGB = 0, bool NASKIP = false>
__global__ __launch_bounds__(64 * WAVES, MINW) void k_cprod(const uint8_t *__restrict__ img, int64_t pitch,
                                               const int32_t *__restrict__ cols, int64_t col0,
                                               int64_t m, const int8_t *__restrict__ xq,
                                               int32_t *__restrict__ acc_out, int64_t m_out,
                                               uint32_t lutA, uint32_t lutB, uint32_t lutC,
                                               int32_t *__restrict__ counts, int32_t n_pad_samples,
                                               const CprodGrid geo, int32_t *__restrict__ part_out) {
  constexpr int NCOL = 16 * NB;
  constexpr int LD = KC / 256;             // 16-B loads per variant row per chunk per lane
  constexpr int XS = KC / 16 * NCOL;       // uint4 entries per LDS buffer
  __shared__ uint4 xs[2][XS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 15, g = lane >> 4;
  constexpr int NT = 64 * WAVES;
  const int nchunks = (int)(pitch * 4 / KC);
  // GEO: the launch runs on the one-dimensional grid of cprod_slab (prod_plan.hpp) — the blocks of variants that fill whole
  // rounds of the CUs first, each over all chunks and into acc_out; then the blocks beyond the last whole round, cut along the
  // samples into slabs whose sums go to part_out[slab][plane][variant - first remainder variant][NCOL] (k_cprod_final adds
  // them).  Every other instance: one workgroup per block, all chunks.
  constexpr bool GEO = CONTIG && !TILED && !STATS && NPLANE < 3 && KC == 512;
  CprodSlab sl{(int)blockIdx.x, 0, 0, nchunks};
  if constexpr (GEO) {
    // (the division of cprod_slab runs on the vector unit: back into scalar registers, the loop has no vector register to spare)
    sl = cprod_slab(geo, blockIdx.x);
    sl.block = __builtin_amdgcn_readfirstlane(sl.block), sl.slab = __builtin_amdgcn_readfirstlane(sl.slab);
    sl.ch_begin = __builtin_amdgcn_readfirstlane(sl.ch_begin), sl.ch_end = __builtin_amdgcn_readfirstlane(sl.ch_end);
  }
  const int ch_begin = sl.ch_begin, ch_end = sl.ch_end;
  if (ch_begin >= ch_end) return;          // an empty slab (never: the planner gives every slab at least one chunk)
  const int64_t wg_base = (int64_t)sl.block * (WAVES * 16 * TILES);
  const int64_t snp_base = wg_base + wave * (16 * TILES);
  const uint8_t *rowp[TILES];
  uint32_t voff[TILES];
#pragma unroll
  for (int t = 0; t < TILES; t++) {
    int64_t j = snp_base + t * 16 + c;
    if (j > m - 1) j = m - 1;
    int64_t col = CONTIG ? col0 + j : (int64_t)cols[j];
    rowp[t] = img + col * pitch + g * 16;
    voff[t] = TILED ? (uint32_t)((((j - wg_base) >> 6) * (pitch >> 8)) * 16384 + (j & 63) * 256 + g * 16)
                    : (uint32_t)((j - wg_base) * pitch + g * 16);
  }
  static_assert(!TILED || (CONTIG && (WAVES * 16 * TILES) % 64 == 0), "streaming layout: whole 64-variant blocks");
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      (void *)(TILED ? img + (((col0 + wg_base) >> 6) * (pitch >> 8)) * 16384
                     : img + (col0 + (CONTIG ? wg_base : 0)) * pitch),
      0, 0x7fffffff, 0x00020000);
  typedef unsigned int v4u __attribute__((ext_vector_type(4)));
  // 16 B of tile t at byte `off` (uniform) of the variant row
  auto gload = [&](const int t, const int off) -> uint4 {
    if constexpr (CONTIG) {
      const int soff = TILED ? ((off >> 8) << 14) + (off & 255) : off;
      const v4u r = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff[t], soff, 0);
      return uint4{r.x, r.y, r.z, r.w};
    } else {
      return *(const uint4 *)(rowp[t] + off);
    }
  };
  // (the digit panel from the slab's first chunk on; the register sets and LDS buffers start at 0 there, whatever its parity)
  const uint4 *xq4 = (const uint4 *)xq;

  v4i acc[TILES][NPLANE][NB];
#pragma unroll
  for (int t = 0; t < TILES; t++)
#pragma unroll
    for (int p = 0; p < NPLANE; p++)
#pragma unroll
      for (int nb = 0; nb < NB; nb++) acc[t][p][nb] = v4i{0, 0, 0, 0};
  uint32_t st_lo[TILES], st_hi[TILES], st_na[TILES];  // popcounts of the low / all / both bits
#pragma unroll
  for (int t = 0; t < TILES; t++) st_lo[t] = st_hi[t] = st_na[t] = 0;

  constexpr int NX = (XS + NT - 1) / NT;   // staged uint4 per thread per chunk
  static_assert(NX <= 4, "staging registers");
  constexpr bool XFULL = (XS % NT == 0);   // every thread stages NX entries
  // Two genotype register sets, chunk ch lives in set ch & 1.  A register is reloaded with the
  // chunk two ahead as soon as its four K-steps are consumed (rolling prefetch): every wave
  // keeps 4 - 8 loads in flight at all times instead of draining to zero at each chunk edge.
  uint4 ga[2][TILES][LD];
  uint4 xr0 = {0, 0, 0, 0}, xr1 = {0, 0, 0, 0}, xr2 = {0, 0, 0, 0}, xr3 = {0, 0, 0, 0};
  // prologue
#pragma unroll
  for (int t = 0; t < TILES; t++)
#pragma unroll
    for (int it = 0; it < LD; it++) ga[0][t][it] = gload(t, ch_begin * (KC / 4) + it * 64);
  // entry x of a thread's staging set exists when the panel is a whole number of workgroups, or below its end
  // (three column blocks shared by 16 waves: 1536 entries for 1024 threads)
  auto staged = [&](const int x) -> bool { return XFULL || tid + x * NT < XS; };
  {
    const uint4 *src = xq4 + (int64_t)ch_begin * XS;
    if (staged(0)) xs[0][tid] = src[tid];
    if constexpr (NX > 1) if (staged(1)) xs[0][tid + NT] = src[tid + NT];
    if constexpr (NX > 2) if (staged(2)) xs[0][tid + 2 * NT] = src[tid + 2 * NT];
    if constexpr (NX > 3) if (staged(3)) xs[0][tid + 3 * NT] = src[tid + 3 * NT];
  }
#pragma unroll
  for (int t = 0; t < TILES; t++)
#pragma unroll
    for (int it = 0; it < LD; it++)
      ga[1][t][it] = gload(t, (ch_end - ch_begin > 1 ? ch_begin + 1 : ch_begin) * (KC / 4) + it * 64);
  __syncthreads();

  auto chunk = [&](auto SETC, const int ch) {
    constexpr int SET = decltype(SETC)::value;
    // No branches around the loads: a conditional load makes the compiler's waitcnt insertion
    // fall back to vmcnt(0) at the join, which drains the prefetch.  Past the end the last
    // chunk is simply loaded again (into registers / an LDS buffer nobody reads).
    const int ch1 = ch + 1 < ch_end ? ch + 1 : ch_end - 1;
    const int ch2 = ch + 2 < ch_end ? ch + 2 : ch_end - 1;
    {
      // the digit panel of the next chunk: into registers now, into LDS after the compute
      const uint4 *src = xq4 + (int64_t)ch1 * XS;
      // (unconditional loads at a clamped index: a branch around a load costs the prefetch its waitcnt, see below)
      auto at = [&](const int x) -> int { return XFULL ? tid + x * NT : (tid + x * NT < XS ? tid + x * NT : XS - 1); };
      xr0 = src[at(0)];
      if constexpr (NX > 1) xr1 = src[at(1)];
      if constexpr (NX > 2) xr2 = src[at(2)];
      if constexpr (NX > 3) xr3 = src[at(3)];
    }
    __builtin_amdgcn_sched_barrier(0);  // keep the digit loads up here, a chunk ahead of their use
    if constexpr (SGB & 2) __builtin_amdgcn_s_setprio(2);  // the MFMA phase outranks waves that are loading
    const int off2 = ch2 * (KC / 4);
    // one K-step of one tile: 16 samples x 16 variants per lane-quad, decode + MFMAs
    auto kstep = [&](const int t, const uint32_t w, const uint4 (&bv)[NB]) {
      uint32_t s0 = w & 0x03030303u, s1 = (w >> 2) & 0x03030303u,
               s2 = (w >> 4) & 0x03030303u, s3 = (w >> 6) & 0x03030303u;
      if constexpr (STATS) {
        // six instructions per dword: the count of the high bits is (all bits) - (low bits), taken at the end
        const uint32_t lo = w & 0x55555555u;
        st_lo[t] += __popc(lo);
        st_hi[t] += __popc(w);              // all bits set (low + high)
        st_na[t] += __popc(lo & (w >> 1));  // both bits of a genotype
      }
      static_assert(!NASKIP || (RAW0 && NPLANE == 2 && !STATS), "the skip is for the missing-value plane of the plain pass");
      bool plane1 = true;
      if constexpr (NASKIP) plane1 = __builtin_amdgcn_ballot_w64(((w & (w >> 1)) & 0x55555555u) != 0u) != 0ull;
#pragma unroll
      for (int p = 0; p < NPLANE; p++) {
        if (NASKIP && p == 1 && !plane1) continue;
        const uint32_t lut = p == 0 ? lutA : p == 1 ? lutB : lutC;
        v4i a;
        if (RAW0 && p == 0) {
          a = v4i{(int)s0, (int)s1, (int)s2, (int)s3};
        } else {
          a = v4i{(int)lut4(lut, s0), (int)lut4(lut, s1), (int)lut4(lut, s2), (int)lut4(lut, s3)};
        }
#pragma unroll
        for (int nb = 0; nb < NB; nb++) {
          v4i b = {(int)bv[nb].x, (int)bv[nb].y, (int)bv[nb].z, (int)bv[nb].w};
          acc[t][p][nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[t][p][nb], 0, 0, 0);
        }
      }
    };
    // (three column blocks: the digit operands of a K-step are read at its start — a second register copy of them,
    // one K-step ahead, does not fit beside 48 accumulators; the other waves' MFMAs cover the LDS latency)
    constexpr bool PFB = NB <= 2;
    uint4 bv[NB], bn[PFB ? NB : 1];
#pragma unroll
    for (int nb = 0; nb < NB; nb++) bv[nb] = xs[SET][(g * 4) * NCOL + nb * 16 + c];
#pragma unroll
    for (int it = 0; it < LD; it++) {
#pragma unroll
      for (int d = 0; d < 4; d++) {
        // prefetch the digit operand of the next K-step so that its LDS latency hides
        // under this step's decode + MFMA
        if constexpr (!PFB) {
          if (it * 4 + d > 0) {
#pragma unroll
            for (int nb = 0; nb < NB; nb++) bv[nb] = xs[SET][(it * 16 + g * 4 + d) * NCOL + nb * 16 + c];
          }
        } else if (it * 4 + d + 1 < LD * 4) {
          const int itn = (it * 4 + d + 1) / 4, dn = (it * 4 + d + 1) % 4;
#pragma unroll
          for (int nb = 0; nb < NB; nb++) bn[nb] = xs[SET][(itn * 16 + g * 4 + dn) * NCOL + nb * 16 + c];
        }
#pragma unroll
        for (int t = 0; t < TILES; t++) {
          const uint32_t w = d == 0 ? ga[SET][t][it].x : d == 1 ? ga[SET][t][it].y
                             : d == 2 ? ga[SET][t][it].z : ga[SET][t][it].w;
          kstep(t, w, bv);
        }
        if constexpr (PFB) {
#pragma unroll
          for (int nb = 0; nb < NB; nb++) bv[nb] = bn[nb];
        }
      }
    }
    // This set is consumed: refill it with the chunk two ahead.  All loads of a tile go out
    // back to back so that both 64-B halves of every 128-B line are requested together
    // (refilling half-way through the chunk, one half at a time, costs 8 % of the bandwidth).
#pragma unroll
    for (int t = 0; t < TILES; t++)
#pragma unroll
      for (int it = 0; it < LD; it++) ga[SET][t][it] = gload(t, off2 + it * 64);
    if constexpr (SGB & 1) {
      // Explicit software pipeline (profiles/r04_sched.txt: 2 % on the two-block kernel): the decode of the following
      // K-steps is slotted into the shadows of the MFMAs — the VALU instructions of a K-step spread evenly behind its
      // MFMAs —, the digit reads one K-step ahead, the refill loads last.  The compiler's own order issues the MFMAs
      // in back-to-back pairs, the second of which stalls its wave for the 12 remaining cycles of the first.
      // masks: 0x008 MFMA, 0x002 VALU, 0x100 DS read, 0x020 VMEM read
      constexpr int VSTEP = TILES * (7 + (NPLANE - (RAW0 ? 1 : 0)) * 4 + (STATS ? 6 : 0));  // VALU per K-step
      constexpr int MSTEP = TILES * NPLANE * NB;                                             // MFMA per K-step
      __builtin_amdgcn_sched_group_barrier(0x100, NB, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 7, 0);
      auto slot = [&](auto IC) {
        constexpr int i = decltype(IC)::value;
        constexpr int nv = VSTEP * (i + 1) / MSTEP - VSTEP * i / MSTEP;
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if constexpr (nv > 0) __builtin_amdgcn_sched_group_barrier(0x002, nv, 0);
      };
      auto slots = [&](auto self, auto IC) {
        constexpr int i = decltype(IC)::value;
        if constexpr (i < MSTEP) {
          slot(IC);
          self(self, std::integral_constant<int, i + 1>{});
        }
      };
#pragma unroll
      for (int stp = 0; stp < LD * 4; stp++) {
        __builtin_amdgcn_sched_group_barrier(0x100, NB, 0);
        slots(slots, std::integral_constant<int, 0>{});
      }
      __builtin_amdgcn_sched_group_barrier(0x020, TILES * LD, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (SGB & 2) __builtin_amdgcn_s_setprio(0);
    {
      if (staged(0)) xs[SET ^ 1][tid] = xr0;
      if constexpr (NX > 1) if (staged(1)) xs[SET ^ 1][tid + NT] = xr1;
      if constexpr (NX > 2) if (staged(2)) xs[SET ^ 1][tid + 2 * NT] = xr2;
      if constexpr (NX > 3) if (staged(3)) xs[SET ^ 1][tid + 3 * NT] = xr3;
    }
    __syncthreads();
  };
  for (int ch = ch_begin; ch < ch_end; ch += 2) {
    chunk(std::integral_constant<int, 0>{}, ch);
    if (ch + 1 < ch_end) chunk(std::integral_constant<int, 1>{}, ch + 1);  // (a slab may have an odd number of chunks)
  }

  // raw accumulators: acc_out[plane][variant][NCOL]; of a remainder block its slab of part_out
  int32_t *out = acc_out;
  int64_t out_m = m_out, out_j0 = 0;
  if constexpr (GEO) {
    if (sl.block >= geo.blocks_whole) {
      out_m = geo.m_rem, out_j0 = m - geo.m_rem;
      out = part_out + (int64_t)sl.slab * NPLANE * out_m * NCOL;
    }
  }
#pragma unroll
  for (int t = 0; t < TILES; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      int64_t j = snp_base + t * 16 + g * 4 + r;
      if (j < m) {
#pragma unroll
        for (int p = 0; p < NPLANE; p++)
#pragma unroll
          for (int nb = 0; nb < NB; nb++)
            out[((int64_t)p * out_m + j - out_j0) * NCOL + nb * 16 + c] = acc[t][p][nb][r];
      }
    }
  if constexpr (STATS) {
    // a variant row is spread over the 4 k-groups of the wave (lanes c, c+16, c+32, c+48)
#pragma unroll
    for (int t = 0; t < TILES; t++) {
      uint32_t lo = st_lo[t], hi = st_hi[t] - st_lo[t], na = st_na[t];
      lo += __shfl_xor(lo, 16); hi += __shfl_xor(hi, 16); na += __shfl_xor(na, 16);
      lo += __shfl_xor(lo, 32); hi += __shfl_xor(hi, 32); na += __shfl_xor(na, 32);
      const int64_t j = snp_base + t * 16 + c;
      if (g == 0 && j < m) {
        const int32_t n1 = (int32_t)(lo - na), n2 = (int32_t)(hi - na);
        *(int4 *)(counts + 4 * j) =
            int4{(int32_t)(pitch * 4) - n1 - n2 - (int32_t)na - n_pad_samples, n1, n2, (int32_t)na};
      }
    }
  }
}

__device__ __forceinline__ double horner(const int32_t *a, int S) {
  double r = 0;
  for (int s = S - 1; s >= 0; s--) r = r * 256.0 + (double)a[s];
  return r;
}
// sum over the slices of a[s] - k q[s] (the genotype plane sum from the raw-code plane sum:
// g0 = code - 3 na, per slice in exact integers)
__device__ __forceinline__ double horner_sub(const int32_t *a, const int32_t *q, int k, int S) {
  double r = 0;
  for (int s = S - 1; s >= 0; s--) r = r * 256.0 + (double)((long long)a[s] - (long long)k * q[s]);
  return r;
}

// z[j, v] = (P - c_j (Sx - Q)) / (s_j qs),  P = P' - 3 Q  (P' = plane sum of the raw codes)
// One thread per variant for ALL vectors of the launch: its 2 x NCOL raw sums are read once, as whole
// 64 / 128-byte rows, and parked in the thread's own LDS row (stride NCOL 2 + 1 words: conflict free), from
// where the digits of vector v are picked with run-time indices.  (Round 2 ran one thread per variant AND
// vector, each reading 2 S of the row's 2 NCOL words: the rows were fetched once per vector — 1.5 ms per
// pass of 16 vectors at 1M variants, as much as all the panel algebra of a solve.)
template <int NCOL>
__global__ __launch_bounds__(128) void k_cprod_final(const int32_t *__restrict__ acc, int64_t m, int S, int nv,
                                                     const VecMeta *__restrict__ meta,
                                                     const double *__restrict__ center,
                                                     const double *__restrict__ scale, double *Z, int64_t ldz,
                                                     int has_q, const int32_t *__restrict__ part, int64_t m_rem,
                                                     int slabs) {
  constexpr int ROW = 2 * NCOL + 1;
  __shared__ int32_t srow[128 * ROW];
  // (the last variants first: those of k_cprod's remainder blocks have slabs to add and should not be the grid's tail)
  const int64_t j = (int64_t)(gridDim.x - 1 - blockIdx.x) * 128 + threadIdx.x;
  if (j >= m) return;
  int32_t *my = srow + threadIdx.x * ROW;
  if (slabs > 0 && j >= m - m_rem) {
    // a variant of a remainder block (k_cprod's grid, prod_plan.hpp): its sums are the slabs' partial sums added — in
    // int64; the total is the int32 one workgroup over all samples would have written (launch_cprod's sample limit).
    // A slab's row is read whole, its NCOL / 4 loads in flight together (as k_prod_final reads its slabs).
    const int nplane = has_q ? 2 : 1;
    for (int p = 0; p < nplane; p++) {
      long long d[NCOL];
#pragma unroll
      for (int c = 0; c < NCOL; c++) d[c] = 0;
      const int4 *row = (const int4 *)(part + ((int64_t)p * m_rem + (j - (m - m_rem))) * NCOL);
      for (int k = 0; k < slabs; k++, row += (int64_t)nplane * m_rem * (NCOL / 4)) {
#pragma unroll
        for (int t = 0; t < NCOL / 4; t++) {
          const int4 v = row[t];
          d[4 * t] += v.x, d[4 * t + 1] += v.y, d[4 * t + 2] += v.z, d[4 * t + 3] += v.w;
        }
      }
#pragma unroll
      for (int c = 0; c < NCOL; c++) my[p * NCOL + c] = (int32_t)d[c];
    }
  } else {
    const int4 *pa = (const int4 *)(acc + j * NCOL), *pq = (const int4 *)(acc + (m + j) * NCOL);
#pragma unroll
    for (int t = 0; t < NCOL / 4; t++) {
      const int4 x = pa[t];
      my[4 * t] = x.x; my[4 * t + 1] = x.y; my[4 * t + 2] = x.z; my[4 * t + 3] = x.w;
    }
    if (has_q) {
#pragma unroll
      for (int t = 0; t < NCOL / 4; t++) {
        const int4 x = pq[t];
        my[NCOL + 4 * t] = x.x; my[NCOL + 4 * t + 1] = x.y; my[NCOL + 4 * t + 2] = x.z; my[NCOL + 4 * t + 3] = x.w;
      }
    }
  }
  const double c = center ? center[j] : 0.0, s = scale ? scale[j] : 1.0;
  for (int v = 0; v < nv; v++) {
    // no missing plane: Q == 0 and P' == P
    const double P = has_q ? horner_sub(my + v * S, my + NCOL + v * S, 3, S) : horner(my + v * S, S);
    const double Q = has_q ? horner(my + NCOL + v * S, S) : 0.0;
    const double Sx = (double)meta[v].sum_hi * 16777216.0 + (double)meta[v].sum_lo;
    const double qs = meta[v].qscale;
    double z = qs > 0 ? (P - c * (Sx - Q)) / (s * qs) : 0.0 / s;
    // a variant with no non-missing genotype contributes only bedAccScaled's NA entry (0),
    // whatever its centre / scale are (src/bed-acc.h:104); P and Sx - Q are exact integers
    if (P == 0.0 && Sx - Q == 0.0 && qs > 0) z = 0.0;
    if (meta[v].nonfinite) z = __longlong_as_double(0x7ff8000000000000LL);
    Z[j + v * ldz] = z;
  }
}

// ---------------------------------------------------------------------------
// k_prod: contraction over variants on the variant-major image.  One wave owns 256
// samples (16 sample groups x 16) and walks a range of variants 64 at a time:
//   16 dword loads/lane (16 variants x 16 samples), four 4x4 byte transposes so that a
//   register holds the same sample quad of 4 variants, then per sample: 2 VALU for the
//   selector, 2 v_perm for the planes, 2 MFMA (g0 x w-digits, na x (c w)-digits) into
//   one accumulator.
//   A operand: lane l -> digit column (l&15), k-group (l>>4): 16 variants' digits
//   B operand: lane l -> sample group (l&15), same 16 variants, sample u of the group
//   D        : lane l -> sample group (l&15), digit columns 4*(l>>4)+r
// RAWP: the P plane is the device code itself (no look-up).
// TILED: `img` is the streaming-layout copy; a step of the workgroup (64 variants x 256 B) is one tile.
// TAG only changes the kernel's name (warm-start launches).
// (Shapes that were measured and dropped — 8-wave workgroups, three register sets, 2 / 4 samples decoded together,
// XCD-aware slab placement, wave pairs / lane halves with 64 accumulators, an explicit MFMA : VALU schedule, the codes as
// the A operand: profiles/r02_ablation.txt, r03_shape_sweeps.txt, r04_two_block_kernels.txt.)
template <int NB, bool CONTIG, bool RAWP, bool HASQ = true, int TAG = 0, bool TILED = false>
__global__ __launch_bounds__(256) void k_prod(const uint8_t *__restrict__ img, int64_t pitch,
                                              const int32_t *__restrict__ cols, int64_t col0,
                                              int64_t m_pad, int64_t mc,
                                              const int8_t *__restrict__ wq,
                                              int32_t *__restrict__ acc_out, int64_t n_pad,
                                              uint32_t lutP, uint32_t lutQ) {
  constexpr int NCOL = 16 * NB, WAVES = 4;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int sg = lane & 15, g = lane >> 4;
  const unsigned bx = blockIdx.x, by = blockIdx.y;
  static_assert(!TILED || CONTIG, "streaming layout: contiguous variants");
  const int64_t wbase = ((int64_t)bx * WAVES + wave) * 256;  // first sample of this wave (n_pad is a multiple of 1024)
  const int64_t wbyte = wbase / 4 + sg * 4;
  const uint32_t lane_off = (uint32_t)(g * 16 * pitch + wbyte);
  const int64_t j0 = (int64_t)by * mc;
  int64_t j1 = j0 + mc;
  if (j1 > m_pad) j1 = m_pad;
  const uint4 *wq4 = (const uint4 *)wq;

  v4i acc[16][NB];
#pragma unroll
  for (int u = 0; u < 16; u++)
#pragma unroll
    for (int nb = 0; nb < NB; nb++) acc[u][nb] = v4i{0, 0, 0, 0};

  // digit operands of one 64-variant step: (4 k-groups) x (2 planes) x NCOL entries of 16 B,
  // contiguous in wq; shared by the 4 waves through LDS, double-buffered
  constexpr int WS = 8 * NCOL;
  __shared__ uint4 ws[2][WS];
  static_assert((WS & (WS - 1)) == 0 && WS <= 64 * WAVES, "digit staging");
  // Two genotype register sets, step s lives in set s & 1 (as in k_cprod): a set is free as
  // soon as its 4x4 byte transposes are done, so it is refilled with the step two ahead
  // right there.  No branches around loads (see k_cprod); past the end the last step is
  // loaded again.
  uint32_t X[2][16];
  uint4 wreg = {0, 0, 0, 0};
  const int wtid = tid & (WS - 1);
  auto load = [&](int64_t jb, uint32_t *dst) {
    if (CONTIG) {
      // buffer loads: scalar descriptor (re-based per step) + scalar row offset + one 32-bit lane
      // offset, so the 16 addresses of a step cost no VALU (global loads took a 64-bit add each)
      if constexpr (TILED) {
        // a wave owns 64 B of a 256-B column block: the four waves of the workgroup cover one tile per step
        const int64_t sbw = (int64_t)bx;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(img + (((col0 + jb) >> 6) * (pitch >> 8) + sbw) * 16384), 0, 0x7fffffff, 0x00020000);
        const int toff = g * 4096 + wave * 64 + sg * 4;
#pragma unroll
        for (int r = 0; r < 16; r++) dst[r] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, toff, r * 256, 0);
      } else {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(img + (col0 + jb) * pitch), 0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int r = 0; r < 16; r++) dst[r] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, (int)lane_off, r * (int)pitch, 0);
      }
    } else {
      const int4 *ip = (const int4 *)(cols + jb + g * 16);
#pragma unroll
      for (int r4 = 0; r4 < 4; r4++) {
        int4 id = ip[r4];
        dst[r4 * 4 + 0] = *(const uint32_t *)(img + (int64_t)id.x * pitch + wbyte);
        dst[r4 * 4 + 1] = *(const uint32_t *)(img + (int64_t)id.y * pitch + wbyte);
        dst[r4 * 4 + 2] = *(const uint32_t *)(img + (int64_t)id.z * pitch + wbyte);
        dst[r4 * 4 + 3] = *(const uint32_t *)(img + (int64_t)id.w * pitch + wbyte);
      }
    }
  };
  // j0 < j1 by the launch geometry of prod_planes (every K-slab has at least one step)
  if (j0 >= j1) return;  // never taken; without it the compiler allocates 144 instead of 80 VGPRs
  const int64_t jlast = j1 - 64;
  ws[0][wtid] = wq4[(j0 / 16) * 2 * NCOL + wtid];
  load(j0, X[0]);
  load(j0 + 64 < j1 ? j0 + 64 : jlast, X[1]);
  __syncthreads();

  auto step = [&](auto SETC, const int64_t jb) {
    constexpr int SET = decltype(SETC)::value;
    const int64_t jn1 = jb + 64 < j1 ? jb + 64 : jlast, jn2 = jb + 128 < j1 ? jb + 128 : jlast;
    wreg = wq4[(jn1 / 16) * 2 * NCOL + wtid];  // next step's digits: registers now, LDS later
    __builtin_amdgcn_sched_barrier(0);
    v4i aw[NB], awc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; nb++) {
      uint4 t0 = ws[SET][(g * 2 + 0) * NCOL + nb * 16 + sg];
      uint4 t1 = ws[SET][(g * 2 + 1) * NCOL + nb * 16 + sg];
      aw[nb] = v4i{(int)t0.x, (int)t0.y, (int)t0.z, (int)t0.w};
      awc[nb] = v4i{(int)t1.x, (int)t1.y, (int)t1.z, (int)t1.w};
    }
    // T[q][r4]: byte b = byte q of X[4*r4 + b]
    uint32_t T[4][4];
#pragma unroll
    for (int r4 = 0; r4 < 4; r4++) {
      const uint32_t x0 = X[SET][4 * r4], x1 = X[SET][4 * r4 + 1], x2 = X[SET][4 * r4 + 2], x3 = X[SET][4 * r4 + 3];
      const uint32_t lo01 = perm8(x1, x0, 0x05010400u);  // x0.b0 x1.b0 x0.b1 x1.b1
      const uint32_t hi01 = perm8(x1, x0, 0x07030602u);  // x0.b2 x1.b2 x0.b3 x1.b3
      const uint32_t lo23 = perm8(x3, x2, 0x05010400u);
      const uint32_t hi23 = perm8(x3, x2, 0x07030602u);
      T[0][r4] = perm8(lo23, lo01, 0x05040100u);  // lo01.b0 lo01.b1 lo23.b0 lo23.b1
      T[1][r4] = perm8(lo23, lo01, 0x07060302u);
      T[2][r4] = perm8(hi23, hi01, 0x05040100u);
      T[3][r4] = perm8(hi23, hi01, 0x07060302u);
    }
    __builtin_amdgcn_sched_barrier(0);
    load(jn2, X[SET]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int u0 = 0; u0 < 4; u0++) {
        v4i g0, na;
#pragma unroll
        for (int r4 = 0; r4 < 4; r4++) {
          const uint32_t sel = (T[q][r4] >> (2 * u0)) & 0x03030303u;
          g0[r4] = RAWP ? (int)sel : (int)lut4(lutP, sel);
          if (HASQ) na[r4] = (int)lut4(lutQ, sel);
        }
#pragma unroll
        for (int nb = 0; nb < NB; nb++) {
          acc[q * 4 + u0][nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aw[nb], g0, acc[q * 4 + u0][nb], 0, 0, 0);
          if (HASQ)
            acc[q * 4 + u0][nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(awc[nb], na, acc[q * 4 + u0][nb], 0, 0, 0);
        }
      }
    ws[SET ^ 1][wtid] = wreg;
    __syncthreads();
  };
  for (int64_t jb = j0; jb < j1; jb += 128) {
    step(std::integral_constant<int, 0>{}, jb);
    if (jb + 64 < j1) step(std::integral_constant<int, 1>{}, jb + 64);
  }
  // raw accumulators: acc_out[ky][sample][NCOL], lane holds columns nb*16 + 4g .. +3
#pragma unroll
  for (int u = 0; u < 16; u++) {
    const int64_t i = wbase + sg * 16 + u;
#pragma unroll
    for (int nb = 0; nb < NB; nb++)
      *(v4i *)(acc_out + (((int64_t)by * n_pad + i) * NCOL + nb * 16 + 4 * g)) = acc[u][nb];
  }
}

// ---------------------------------------------------------------------------
// k_prodT: Y = A~ X on the SAMPLE-MAJOR copy of the image (bsn_bed::d_smaj): the contraction index — the variants —
// is the contiguous one there, so the kernel is k_cprod with the roles of samples and variants exchanged: one wave
// owns 32 samples (two 16-row MFMA tiles) and walks its slab of variants 512 at a time, the 16 waves of a workgroup
// share the digit panel of the chunk through LDS (double-buffered).  Against k_prod on the variant-major image: no
// 4 x 4 byte transposes (11 instead of 13.3 VALU instructions per 4 MFMAs), 16 instead of 128 accumulator registers,
// four waves per SIMD instead of two.  Same integer sums -> bit-identical results.
//   A operand: lane l -> sample row (l & 15), k-group (l >> 4): 16 variants of that sample (one decoded dword)
//   B operand: lane l -> digit column (l & 15), the same 16 variants: w-digits for the code plane, (c w - 3 w)-digits
//              for the missing-value plane (k_quant mode 1 with the cprod byte order), BOTH into one accumulator
//   D        : lane l -> digit column (l & 15), sample rows 4 * (l >> 4) + r
// The variants are split into slabs of chunks (int32 partial sums per slab, added by k_prod_final in exact int64 like
// k_prod's) because 782 workgroups of 512 samples alone would fill 3.05 rounds of 256 CUs — but only for the sample blocks
// beyond the last whole round (14 of the 782, 18 slabs); the blocks of the whole rounds take the planner's ky_whole slabs
// (prod_plan.hpp: plan_prod, and prodt_slab for the workgroup's place in the one-dimensional grid).
// The copy is CHUNK-MAJOR (bsn_bed::d_smaj): byte of the operator's first variant in a sample row (col0 / 4, a multiple of 16).
// NASKIP: as in k_cprod — the missing-value plane of a K-step (16 samples x 64 variants) only when it has a missing code.
// SPARSE (prodt_sparse.hpp): both planes in ONE v_smfmac_i32_16x16x128_i8 per tile and column block.  Of a genotype's
// code term and missing term at most one is non-zero, so with the digit rows interleaved as (A_e, B_e) (k_quant, PERM = 2)
// the 16 variants of a decoded dword are 16 compressed values over 32 dense K: half the matrix instructions, the same
// integer per sample (3 A + (B - 3 A) = B) -> bit-identical.  The LDS panel has the same bytes, rows and addressing.
// (Reading the digit operands one K-step ahead with three column blocks as well, now that 4 + 1 operand registers
// replace 8, measured level in the skeleton of tools/ubench/smfmac_parts.hip — 26.5 ms either way — and is not built.)
template <int NB, bool HASQ, int TILES = 2, int WAVES = 16, int TAG = 0, int SGB = 3, bool NASKIP = false, bool SPARSE = false>
__global__ __launch_bounds__(64 * WAVES) void k_prodT(const uint8_t *__restrict__ simg, int64_t rows_t, int64_t chunk0,
                                                      const ProdTGrid geo,
                                                      const int8_t *__restrict__ wq, int32_t *__restrict__ acc_out,
                                                      int64_t n_pad, uint32_t lutQ, int seg_bs, int seg_stride, int seg_off) {
  constexpr int KC = 512, NCOL = 16 * NB, LD = KC / 256;
  constexpr int XS = KC / 16 * 2 * NCOL;   // uint4 entries of one chunk's digit panel (two planes)
  constexpr int NT = 64 * WAVES, NX = XS / NT;
  static_assert(XS % NT == 0 && NX >= 1 && NX <= 4, "digit staging");
  __shared__ uint4 xs[2][XS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 15, g = lane >> 4;
  // seg_bs > 0 (a segment of the sharded solve's product pass, op_prod_segments): the launch covers blocks
  // [seg_off, seg_off + seg_bs) of every piece of seg_stride blocks
  // ... in a grid of (pieces x seg_bs) x geo.ky; every other launch is the one-dimensional grid of prodt_slab (prod_plan.hpp)
  ProdTSlab sl;
  if (seg_bs > 0) {
    sl.bx = (int)((blockIdx.x / (unsigned)seg_bs) * (unsigned)seg_stride + (unsigned)seg_off + blockIdx.x % (unsigned)seg_bs);
    sl.slab = (int)blockIdx.y;
    sl.ch_begin = sl.slab * geo.cps;
    sl.ch_end = sl.ch_begin + geo.cps < geo.nchunks ? sl.ch_begin + geo.cps : geo.nchunks;
  } else {
    sl = prodt_slab(geo, blockIdx.x);
  }
  const unsigned bx = (unsigned)sl.bx;
  const int64_t wg_base = (int64_t)bx * (WAVES * 16 * TILES);
  const int64_t row_base = wg_base + wave * (16 * TILES);
  uint32_t voff[TILES];
#pragma unroll
  for (int t = 0; t < TILES; t++) {
    int64_t i = row_base + t * 16 + c;
    if (i > rows_t - 1) i = rows_t - 1;
    voff[t] = (uint32_t)((i - wg_base) * (KC / 4) + g * 16);
  }
  const int ch_begin = sl.ch_begin, ch_end = sl.ch_end;
  if (ch_begin >= ch_end) return;  // (never: the launch geometry gives every slab at least one chunk)
  if (wg_base >= rows_t) return;    // a workgroup wholly past the copy's rows (a segment's padding blocks): nothing to read or write
  // chunk ch of the slab: the workgroup's 512 sample rows x 128 B are ONE contiguous 64-KB run of the copy
  const int64_t chunk_stride = rows_t * (KC / 4);
  const uint8_t *const base0 = simg + ((chunk0 + ch_begin) * rows_t + wg_base) * (KC / 4);
  typedef unsigned int v4u __attribute__((ext_vector_type(4)));
  auto gload = [&](const int t, const int ch, const int off) -> uint4 {
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void *)(base0 + (int64_t)ch * chunk_stride), 0, 0x7fffffff, 0x00020000);
    const v4u r = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff[t], off, 0);
    return uint4{r.x, r.y, r.z, r.w};
  };
  const int nch = ch_end - ch_begin;
  const uint4 *xq4 = (const uint4 *)wq + (int64_t)ch_begin * XS;

  v4i acc[TILES][NB];
#pragma unroll
  for (int t = 0; t < TILES; t++)
#pragma unroll
    for (int nb = 0; nb < NB; nb++) acc[t][nb] = v4i{0, 0, 0, 0};
  uint4 ga[2][TILES][LD];
  uint4 xr0 = {0, 0, 0, 0}, xr1 = {0, 0, 0, 0}, xr2 = {0, 0, 0, 0}, xr3 = {0, 0, 0, 0};   // (scalars: an array captured by the lambda below ends up in scratch)
#pragma unroll
  for (int t = 0; t < TILES; t++)
#pragma unroll
    for (int it = 0; it < LD; it++) ga[0][t][it] = gload(t, 0, it * 64);
#pragma unroll
  for (int x = 0; x < NX; x++) xs[0][tid + x * NT] = xq4[tid + x * NT];
#pragma unroll
  for (int t = 0; t < TILES; t++)
#pragma unroll
    for (int it = 0; it < LD; it++) ga[1][t][it] = gload(t, nch > 1 ? 1 : 0, it * 64);
  __syncthreads();

  auto chunk = [&](auto SETC, const int ch) {
    constexpr int SET = decltype(SETC)::value;
    // branch-free prefetch as in k_cprod: past the end of the slab its last chunk is loaded again
    const int ch1 = ch + 1 < nch ? ch + 1 : nch - 1;
    const int ch2 = ch + 2 < nch ? ch + 2 : nch - 1;
    xr0 = xq4[(int64_t)ch1 * XS + tid];
    if constexpr (NX > 1) xr1 = xq4[(int64_t)ch1 * XS + tid + NT];
    if constexpr (NX > 2) xr2 = xq4[(int64_t)ch1 * XS + tid + 2 * NT];
    if constexpr (NX > 3) xr3 = xq4[(int64_t)ch1 * XS + tid + 3 * NT];
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (SGB & 2) __builtin_amdgcn_s_setprio(2);
    constexpr int NP = HASQ ? 2 : 1;
    static_assert(!SPARSE || (HASQ && !NASKIP), "the sparse form replaces the two planes of the plain pass");
    constexpr bool PFB = NB <= 2;   // (as in k_cprod: no second register copy of the digit operands with three column blocks)
    uint4 bv[NP][NB], bn[PFB ? NP : 1][PFB ? NB : 1];
    // 16-byte row of the panel that register p of the lane's digit operand takes in K-step kb (= it * 16 + d).  Dense: row p
    // (the plane) of the lane group's own block of 16 variants.  Sparse: the instruction's B operand holds dense K
    // 64 p + 16 g .. + 15 in register half p of lane group g, and its A operand of lane group ga the compressed values of
    // dense K 32 ga .. 32 ga + 31 (tools/ubench/smfmac_parts.hip) — so half p is row (g & 1), variants 8 (g & 1) .. + 7 with
    // their (A_e, B_e) pairs, of the block that lane group 2 p + (g >> 1) decodes.
    auto xrow = [&](const int kb, const int p) -> int {
      return SPARSE ? (kb + (2 * p + (g >> 1)) * 4) * 2 + (g & 1) : (kb + g * 4) * 2 + p;
    };
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
      for (int nb = 0; nb < NB; nb++) {
        bv[p][nb] = xs[SET][xrow(0, p) * NCOL + nb * 16 + c];
        if constexpr (PFB) bn[p][nb] = bv[p][nb];
      }
#pragma unroll
    for (int it = 0; it < LD; it++) {
#pragma unroll
      for (int d = 0; d < 4; d++) {
        if constexpr (!PFB) {
          if (it * 4 + d > 0) {
#pragma unroll
            for (int p = 0; p < NP; p++)
#pragma unroll
              for (int nb = 0; nb < NB; nb++) bv[p][nb] = xs[SET][xrow(it * 16 + d, p) * NCOL + nb * 16 + c];
          }
        } else if (it * 4 + d + 1 < LD * 4) {
          const int itn = (it * 4 + d + 1) / 4, dn = (it * 4 + d + 1) % 4;
#pragma unroll
          for (int p = 0; p < NP; p++)
#pragma unroll
            for (int nb = 0; nb < NB; nb++) bn[p][nb] = xs[SET][xrow(itn * 16 + dn, p) * NCOL + nb * 16 + c];
        }
#pragma unroll
        for (int t = 0; t < TILES; t++) {
          const uint32_t w = d == 0 ? ga[SET][t][it].x : d == 1 ? ga[SET][t][it].y
                             : d == 2 ? ga[SET][t][it].z : ga[SET][t][it].w;
          if constexpr (SPARSE) {
            uint32_t av[4], idx;
            prodt_sparse_decode(w, av, idx);
            const v4i a = {(int)av[0], (int)av[1], (int)av[2], (int)av[3]};
#pragma unroll
            for (int nb = 0; nb < NB; nb++) {
              const v8i b = {(int)bv[0][nb].x, (int)bv[0][nb].y, (int)bv[0][nb].z, (int)bv[0][nb].w,
                             (int)bv[1][nb].x, (int)bv[1][nb].y, (int)bv[1][nb].z, (int)bv[1][nb].w};
              acc[t][nb] = __builtin_amdgcn_smfmac_i32_16x16x128_i8(a, b, acc[t][nb], (int)idx, 0, 0);
            }
            continue;
          }
          const uint32_t s0 = w & 0x03030303u, s1 = (w >> 2) & 0x03030303u, s2 = (w >> 4) & 0x03030303u,
                         s3 = (w >> 6) & 0x03030303u;
          const v4i a0 = {(int)s0, (int)s1, (int)s2, (int)s3};
#pragma unroll
          for (int nb = 0; nb < NB; nb++) {
            const v4i b = {(int)bv[0][nb].x, (int)bv[0][nb].y, (int)bv[0][nb].z, (int)bv[0][nb].w};
            acc[t][nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b, acc[t][nb], 0, 0, 0);
          }
          if constexpr (HASQ) {
            static_assert(!NASKIP || HASQ, "the skip is for the missing-value plane");
            bool plane1 = true;
            if constexpr (NASKIP) plane1 = __builtin_amdgcn_ballot_w64(((w & (w >> 1)) & 0x55555555u) != 0u) != 0ull;
            if (plane1) {
              const v4i a1 = {(int)lut4(lutQ, s0), (int)lut4(lutQ, s1), (int)lut4(lutQ, s2), (int)lut4(lutQ, s3)};
#pragma unroll
              for (int nb = 0; nb < NB; nb++) {
                const v4i b = {(int)bv[1][nb].x, (int)bv[1][nb].y, (int)bv[1][nb].z, (int)bv[1][nb].w};
                acc[t][nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b, acc[t][nb], 0, 0, 0);
              }
            }
          }
        }
        if constexpr (PFB) {
#pragma unroll
          for (int p = 0; p < NP; p++)
#pragma unroll
            for (int nb = 0; nb < NB; nb++) bv[p][nb] = bn[p][nb];
        }
      }
    }
#pragma unroll
    for (int t = 0; t < TILES; t++)
#pragma unroll
      for (int it = 0; it < LD; it++) ga[SET][t][it] = gload(t, ch2, it * 64);
    if constexpr (SGB & 1) {
      // the explicit MFMA / decode pipeline of k_cprod (0x008 MFMA, 0x002 VALU, 0x100 DS read, 0x020 VMEM read)
      // (sparse: 18 VALU — prodt_sparse_decode as compiled — against NB matrix instructions per tile)
      constexpr int VSTEP = TILES * (SPARSE ? 18 : 7 + (HASQ ? 4 : 0)), MSTEP = TILES * (SPARSE ? NB : NP * NB);
      __builtin_amdgcn_sched_group_barrier(0x100, NP * NB, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, SPARSE ? 9 : 7, 0);
      auto slots = [&](auto self, auto IC) {
        constexpr int i = decltype(IC)::value;
        if constexpr (i < MSTEP) {
          constexpr int nv = VSTEP * (i + 1) / MSTEP - VSTEP * i / MSTEP;
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          if constexpr (nv > 0) __builtin_amdgcn_sched_group_barrier(0x002, nv, 0);
          self(self, std::integral_constant<int, i + 1>{});
        }
      };
#pragma unroll
      for (int stp = 0; stp < LD * 4; stp++) {
        __builtin_amdgcn_sched_group_barrier(0x100, NP * NB, 0);
        slots(slots, std::integral_constant<int, 0>{});
      }
      __builtin_amdgcn_sched_group_barrier(0x020, TILES * LD, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (SGB & 2) __builtin_amdgcn_s_setprio(0);
    xs[SET ^ 1][tid] = xr0;
    if constexpr (NX > 1) xs[SET ^ 1][tid + NT] = xr1;
    if constexpr (NX > 2) xs[SET ^ 1][tid + 2 * NT] = xr2;
    if constexpr (NX > 3) xs[SET ^ 1][tid + 3 * NT] = xr3;
    __syncthreads();
  };
  for (int ch = 0; ch < nch; ch += 2) {
    chunk(std::integral_constant<int, 0>{}, ch);
    if (ch + 1 < nch) chunk(std::integral_constant<int, 1>{}, ch + 1);
  }
  // raw accumulators: acc_out[slab][sample][NCOL] (k_prod's layout, read by k_prod_final)
#pragma unroll
  for (int t = 0; t < TILES; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int64_t i = row_base + t * 16 + g * 4 + r;
      if (i < n_pad) {
#pragma unroll
        for (int nb = 0; nb < NB; nb++)
          acc_out[((int64_t)sl.slab * n_pad + i) * NCOL + nb * 16 + c] = acc[t][nb][r];
      }
    }
}

// y[i, v] = (sum_ky value(i) - C_v) / qs_v, gathered through rows[].  One thread per output
// row reads its NCOL contiguous int32 per K-chunk (16 B loads, consecutive rows adjacent).
// blk_rows > 0: blocked output for the reduce-scatter of a segment (op_prod_segments) — row i belongs to piece
// i / blk_rows and goes to Y[(piece * nv + v) * blk_rows + i % blk_rows]; rows[i] < 0 is padding (zero).
// Image rows below rows_whole (k_prodT's whole-round blocks, prod_plan.hpp) have ky_whole slabs, the others ky.
template <int NCOL>
__global__ __launch_bounds__(256) void k_prod_final(const int32_t *__restrict__ acc, int64_t n_pad, int ky, int64_t rows_whole,
                             int ky_whole, int S, int nv,
                             const VecMeta *meta, const int32_t *rows, int64_t n, double *Y,
                             int64_t ldy, int sub_const, double beta, int64_t blk_rows = 0) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int64_t i2 = rows ? (int64_t)rows[i] : i;
  if (i2 < 0) {
    for (int v = 0; v < nv; v++) Y[(i / blk_rows * nv + v) * blk_rows + i % blk_rows] = 0.0;
    return;
  }
  long long d[NCOL];
#pragma unroll
  for (int c = 0; c < NCOL; c++) d[c] = 0;
  const int slabs = i2 < rows_whole ? ky_whole : ky;
  for (int k = 0; k < slabs; k++) {
    const int4 *a = (const int4 *)(acc + ((int64_t)k * n_pad + i2) * NCOL);
#pragma unroll
    for (int c4 = 0; c4 < NCOL / 4; c4++) {
      int4 t = a[c4];
      d[4 * c4 + 0] += t.x;
      d[4 * c4 + 1] += t.y;
      d[4 * c4 + 2] += t.z;
      d[4 * c4 + 3] += t.w;
    }
  }
  // Column v S + s is slice s of vector v: ONE walk down the columns (the registers are indexed by the unrolled loop, v and s
  // are uniform counters), r = r 256 + d from a vector's top slice down to its slice 0 — the operations, in the order, of a
  // loop over v and s that picks d[v S + s] out of the registers with NCOL selects per slice (which it was: 4 608 selects per
  // row at 16 vectors x 3 slices, most of the launch once the rows have two slabs to add — profiles/prodt_whole_rounds_ab.txt).
  int v = (NCOL - 1) / S, s = (NCOL - 1) - v * S;
  double r = 0;
#pragma unroll
  for (int c = NCOL - 1; c >= 0; c--) {
    if (v < nv) {   // (columns nv S and beyond are unused)
      if (s == S - 1) r = 0;
      r = r * 256.0 + (double)d[c];
      if (s == 0) {
        double C = sub_const ? (double)meta[v].sum2_hi * 16777216.0 + (double)meta[v].sum2_lo : 0.0;
        double qs = meta[v].qscale;
        double y = qs > 0 ? (r - C) / qs : 0.0;
        if (meta[v].nonfinite) y = __longlong_as_double(0x7ff8000000000000LL);
        if (blk_rows > 0)
          Y[(i / blk_rows * nv + v) * blk_rows + i % blk_rows] = y;
        else
          Y[i + v * ldy] = beta != 0.0 ? beta * Y[i + v * ldy] + y : y;
      }
    }
    if (s == 0) s = S - 1, v--;
    else s--;
  }
}

// ---------------------------------------------------------------------------
// Byte image (bsn_bed::bits == 8): one int8 grid index k per genotype, 0x80 = missing.  The loaded
// bytes ARE the MFMA operand (after zeroing the missing marker when the data has any); 1 B per genotype
// makes both products plainly HBM-bound (1 - 2 MFMA per 16 B instead of 8).
__device__ __forceinline__ uint32_t val8m(uint32_t w, uint32_t &na) {
  const uint32_t t = w ^ 0x80808080u;
  const uint32_t y = (t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
  const uint32_t z = ~(y | t | 0x7F7F7F7Fu);  // 0x80 iff the byte of w is 0x80
  na = z >> 7;
  return w & ~(z | (z - na));
}

// k_cprod8: contraction over samples.  One wave owns 16 variants for the sample range of its slice; the 8 waves
// of a workgroup share the digit panel of the current 256-sample chunk through LDS (double-buffered).
//   A operand: lane l -> variant row (l&15), k-group (l>>4): 16 B = 16 samples;  B: digit column (l&15)
// |k| <= 127 times a digit in [-128, 127]: one int32 accumulator holds at most 131 072 samples (byte_plan.hpp), so
// blockIdx.y is the slice: `slice_chunks` chunks of the row from chunk blockIdx.y * slice_chunks on, summed into
// block blockIdx.y of acc_out ([slice][plane][variant][column]); k_cprod_final8 adds the slices in 64 bits.
template <int NB, bool HASNA, bool CONTIG>
__global__ __launch_bounds__(512) void k_cprod8(const uint8_t *__restrict__ img, int64_t pitch,
                                                const int32_t *__restrict__ cols, int64_t col0, int64_t m,
                                                const int8_t *__restrict__ xq, int32_t *__restrict__ acc_out,
                                                int64_t m_out, int slice_chunks) {
  constexpr int KC = 256, LD = KC / 64, NCOL = 16 * NB, XS = KC / 16 * NCOL, WAVES = 8, NT = 64 * WAVES;
  constexpr int NPL = HASNA ? 2 : 1;
  __shared__ uint4 xs[2][XS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int64_t snp_base = ((int64_t)blockIdx.x * WAVES + wave) * 16;
  int64_t j = snp_base + c;
  if (j > m - 1) j = m - 1;
  const int64_t col = CONTIG ? col0 + j : (int64_t)cols[j];
  const int ch0 = (int)blockIdx.y * slice_chunks;   // (one slice: 0, and nchunks is the whole row)
  const int nchunks = min((int)(pitch / KC) - ch0, slice_chunks);
  const uint8_t *rowp = img + col * pitch + (int64_t)ch0 * KC + g * 16;
  const uint4 *xq4 = (const uint4 *)xq + (int64_t)ch0 * XS;
  acc_out += (int64_t)blockIdx.y * NPL * m_out * NCOL;
  v4i acc[NPL][NB];
#pragma unroll
  for (int p = 0; p < NPL; p++)
#pragma unroll
    for (int nb = 0; nb < NB; nb++) acc[p][nb] = v4i{0, 0, 0, 0};
  static_assert(XS <= NT, "digit staging");
  uint4 ga[2][LD], xr = {0, 0, 0, 0};
#pragma unroll
  for (int it = 0; it < LD; it++) ga[0][it] = *(const uint4 *)(rowp + it * 64);
  if (tid < XS) xs[0][tid] = xq4[tid];
#pragma unroll
  for (int it = 0; it < LD; it++) ga[1][it] = *(const uint4 *)(rowp + (nchunks > 1 ? KC : 0) + it * 64);
  __syncthreads();
  auto chunk = [&](auto SETC, const int ch) {
    constexpr int SET = decltype(SETC)::value;
    const int ch1 = ch + 1 < nchunks ? ch + 1 : nchunks - 1, ch2 = ch + 2 < nchunks ? ch + 2 : nchunks - 1;
    if (tid < XS) xr = xq4[(int64_t)ch1 * XS + tid];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int it = 0; it < LD; it++) {
      const uint4 w = ga[SET][it];
      v4i val, na;
      if constexpr (HASNA) {
        uint32_t n0, n1, n2, n3;
        val = v4i{(int)val8m(w.x, n0), (int)val8m(w.y, n1), (int)val8m(w.z, n2), (int)val8m(w.w, n3)};
        na = v4i{(int)n0, (int)n1, (int)n2, (int)n3};
      } else {
        val = v4i{(int)w.x, (int)w.y, (int)w.z, (int)w.w};
      }
#pragma unroll
      for (int nb = 0; nb < NB; nb++) {
        const uint4 bv = xs[SET][(it * 4 + g) * NCOL + nb * 16 + c];
        const v4i b = {(int)bv.x, (int)bv.y, (int)bv.z, (int)bv.w};
        acc[0][nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(val, b, acc[0][nb], 0, 0, 0);
        if constexpr (HASNA) acc[1][nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(na, b, acc[1][nb], 0, 0, 0);
      }
    }
#pragma unroll
    for (int it = 0; it < LD; it++) ga[SET][it] = *(const uint4 *)(rowp + (int64_t)ch2 * KC + it * 64);
    __builtin_amdgcn_sched_barrier(0);
    if (tid < XS) xs[SET ^ 1][tid] = xr;
    __syncthreads();
  };
  for (int ch = 0; ch < nchunks; ch += 2) {
    chunk(std::integral_constant<int, 0>{}, ch);
    if (ch + 1 < nchunks) chunk(std::integral_constant<int, 1>{}, ch + 1);
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int64_t jo = snp_base + g * 4 + r;
    if (jo < m) {
#pragma unroll
      for (int p = 0; p < NPL; p++)
#pragma unroll
        for (int nb = 0; nb < NB; nb++) acc_out[((int64_t)p * m_out + jo) * NCOL + nb * 16 + c] = acc[p][nb][r];
    }
  }
}

// horner over the digit columns of k_cprod8, each summed over its `nslice` sample slices (`stride` int32 apart) in 64 bits
__device__ __forceinline__ double horner_slices(const int32_t *a, int S, int nslice, int64_t stride) {
  double r = 0;
  for (int s = S - 1; s >= 0; s--) {
    long long d = 0;
    for (int t = 0; t < nslice; t++) d += a[t * stride + s];
    r = r * 256.0 + (double)d;
  }
  return r;
}
// z[j, v] = (vstep P + (voff - c_j) (Sx - Q)) / (s_j qs):  value = voff + vstep k on non-missing genotypes
__global__ void k_cprod_final8(const int32_t *acc, int64_t m, int ncol, int S, const VecMeta *meta,
                               const double *center, const double *scale, double *Z, int64_t ldz, int has_q,
                               double vstep, double voff, int nslice) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int v = blockIdx.y;
  if (j >= m) return;
  const int64_t stride = (has_q ? 2 : 1) * m * ncol;
  const double P = horner_slices(acc + j * ncol + v * S, S, nslice, stride);
  const double Q = has_q ? horner_slices(acc + (m + j) * ncol + v * S, S, nslice, stride) : 0.0;
  const double Sx = (double)meta[v].sum_hi * 16777216.0 + (double)meta[v].sum_lo;
  const double c = center ? center[j] : 0.0, s = scale ? scale[j] : 1.0, qs = meta[v].qscale;
  double z = qs > 0 ? (vstep * P + (voff - c) * (Sx - Q)) / (s * qs) : 0.0 / s;
  if (meta[v].nonfinite) z = __longlong_as_double(0x7ff8000000000000LL);
  Z[j + v * ldz] = z;
}

// k_prod8: contraction over variants on the variant-major byte image.  One wave owns 64 samples
// (16 sample groups x 4) and walks a range of variants 64 at a time: 16 dword loads per lane (16 variants
// x 4 samples), four 4x4 byte transposes, then per sample one operand of 16 variants.
template <int NB, bool HASNA, bool CONTIG>
__global__ __launch_bounds__(256) void k_prod8(const uint8_t *__restrict__ img, int64_t pitch,
                                               const int32_t *__restrict__ cols, int64_t col0, int64_t m_pad,
                                               int64_t mc, const int8_t *__restrict__ wq,
                                               int32_t *__restrict__ acc_out, int64_t n_pad) {
  constexpr int NCOL = 16 * NB, WS = 8 * NCOL;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, sg = lane & 15, g = lane >> 4;
  const int64_t wbase = ((int64_t)blockIdx.x * 4 + wave) * 64;  // first sample of this wave
  const int64_t wbyte = wbase + sg * 4;
  const int64_t j0 = (int64_t)blockIdx.y * mc;
  int64_t j1 = j0 + mc;
  if (j1 > m_pad) j1 = m_pad;
  if (j0 >= j1) return;
  const uint4 *wq4 = (const uint4 *)wq;
  v4i acc[4][NB];
#pragma unroll
  for (int u = 0; u < 4; u++)
#pragma unroll
    for (int nb = 0; nb < NB; nb++) acc[u][nb] = v4i{0, 0, 0, 0};
  __shared__ uint4 ws[2][WS];
  static_assert(WS <= 256, "digit staging");
  const int wtid = tid & (WS - 1);
  uint32_t X[2][16];
  auto load = [&](int64_t jb, uint32_t *dst) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int64_t jj = jb + g * 16 + r;
      const int64_t col = CONTIG ? col0 + jj : (int64_t)cols[jj];
      dst[r] = *(const uint32_t *)(img + col * pitch + wbyte);
    }
  };
  const int64_t jlast = j1 - 64;
  uint4 wreg = {0, 0, 0, 0};
  ws[0][wtid] = wq4[(j0 / 16) * 2 * NCOL + wtid];
  load(j0, X[0]);
  load(j0 + 64 < j1 ? j0 + 64 : jlast, X[1]);
  __syncthreads();
  auto step = [&](auto SETC, const int64_t jb) {
    constexpr int SET = decltype(SETC)::value;
    const int64_t jn1 = jb + 64 < j1 ? jb + 64 : jlast, jn2 = jb + 128 < j1 ? jb + 128 : jlast;
    wreg = wq4[(jn1 / 16) * 2 * NCOL + wtid];
    v4i aw[NB], awc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; nb++) {
      const uint4 t0 = ws[SET][(g * 2 + 0) * NCOL + nb * 16 + sg], t1 = ws[SET][(g * 2 + 1) * NCOL + nb * 16 + sg];
      aw[nb] = v4i{(int)t0.x, (int)t0.y, (int)t0.z, (int)t0.w};
      awc[nb] = v4i{(int)t1.x, (int)t1.y, (int)t1.z, (int)t1.w};
    }
    uint32_t T[4][4];  // T[q][r4]: byte b = sample q of variant 4 r4 + b
#pragma unroll
    for (int r4 = 0; r4 < 4; r4++) {
      const uint32_t x0 = X[SET][4 * r4], x1 = X[SET][4 * r4 + 1], x2 = X[SET][4 * r4 + 2], x3 = X[SET][4 * r4 + 3];
      const uint32_t lo01 = perm8(x1, x0, 0x05010400u), hi01 = perm8(x1, x0, 0x07030602u);
      const uint32_t lo23 = perm8(x3, x2, 0x05010400u), hi23 = perm8(x3, x2, 0x07030602u);
      T[0][r4] = perm8(lo23, lo01, 0x05040100u);
      T[1][r4] = perm8(lo23, lo01, 0x07060302u);
      T[2][r4] = perm8(hi23, hi01, 0x05040100u);
      T[3][r4] = perm8(hi23, hi01, 0x07060302u);
    }
    load(jn2, X[SET]);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      v4i val, na;
      if constexpr (HASNA) {
        uint32_t n0, n1, n2, n3;
        val = v4i{(int)val8m(T[q][0], n0), (int)val8m(T[q][1], n1), (int)val8m(T[q][2], n2), (int)val8m(T[q][3], n3)};
        na = v4i{(int)n0, (int)n1, (int)n2, (int)n3};
      } else {
        val = v4i{(int)T[q][0], (int)T[q][1], (int)T[q][2], (int)T[q][3]};
      }
#pragma unroll
      for (int nb = 0; nb < NB; nb++) {
        acc[q][nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aw[nb], val, acc[q][nb], 0, 0, 0);
        if constexpr (HASNA) acc[q][nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(awc[nb], na, acc[q][nb], 0, 0, 0);
      }
    }
    ws[SET ^ 1][wtid] = wreg;
    __syncthreads();
  };
  for (int64_t jb = j0; jb < j1; jb += 128) {
    step(std::integral_constant<int, 0>{}, jb);
    if (jb + 64 < j1) step(std::integral_constant<int, 1>{}, jb + 64);
  }
  if (wbase < n_pad) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int64_t i = wbase + sg * 4 + u;
#pragma unroll
      for (int nb = 0; nb < NB; nb++)
        *(v4i *)(acc_out + (((int64_t)blockIdx.y * n_pad + i) * NCOL + nb * 16 + 4 * g)) = acc[u][nb];
    }
  }
}

void require_bits(const bsn_bed *b, int bits, const char *what) {
  if (b->bits != bits)
    fail("%s is not available for this handle: it needs %s", what,
         bits == 2 ? "a 2-bit genotype image (.bed, or an FBM.code256 whose codes decode to 0 / 1 / 2 / NA)"
                   : "a byte (dosage) image");
}

// ---------------------------------------------------------------------------
// more = true: a further piece of the launch begun before (a product pass in segments: the kernels of its segments are
// timed one by one — what lies between them, finalize kernels and the collective's hand-over, is not streaming time — and
// count as ONE launch)
void prof_begin(bsn_op *op, int kind, bool more) {
  if (!op->profile) return;
  if (op->prof_kind_override >= 0) kind = op->prof_kind_override;
  op->ev_more.push_back(more);
  hipEvent_t a, b;
  BSN_HIP(hipEventCreate(&a));
  BSN_HIP(hipEventCreate(&b));
  op->ev_begin.push_back(a);
  op->ev_end.push_back(b);
  op->ev_kind.push_back(kind);
  BSN_HIP(hipEventRecord(a, op->bed->stream));
}
void prof_end(bsn_op *op) {
  if (!op->profile) return;
  BSN_HIP(hipEventRecord(op->ev_end.back(), op->bed->stream));
  op->prof_kernel[op->ev_kind.back() % kProfKinds] = g_last_kernel;
}
void prof_collect(bsn_op *op, double ms[kProfKinds], int count[kProfKinds]) {
  for (int k = 0; k < kProfKinds; k++) ms[k] = 0, count[k] = 0;
  for (size_t i = 0; i < op->ev_begin.size(); i++) {
    float t = 0;
    // (a pair whose end was never recorded — a launch that failed, a solve that was aborted — is dropped, not an error)
    if (hipEventSynchronize(op->ev_end[i]) == hipSuccess &&
        hipEventElapsedTime(&t, op->ev_begin[i], op->ev_end[i]) == hipSuccess) {
      ms[op->ev_kind[i]] += t;
      if (!op->ev_more[i]) count[op->ev_kind[i]]++;
    }
    (void)hipEventDestroy(op->ev_begin[i]);
    (void)hipEventDestroy(op->ev_end[i]);
  }
  (void)hipGetLastError();
  op->ev_begin.clear();
  op->ev_end.clear();
  op->ev_kind.clear();
  op->ev_more.clear();
}

// (kMaxCols, kMetaVecs, pick_nb: prod_plan.hpp)
static VecMeta *meta_buffer(bsn_op *op) {
  return (VecMeta *)op->d_meta.ensure((size_t)kMetaVecs * 8 + (size_t)kMetaVecs * 256 * 2);
}
// samples a variant row is padded to (the digit panels and partial buffers are that long)
static inline int64_t n_padded(const bsn_bed *b) { return b->bits == 8 ? b->pitch : b->pitch * 4; }

static void quantise(bsn_op *op, const double *d_X, int64_t ldx, int64_t len, int64_t len_pad,
                     int nvec, int mode, int S, int ncol, int permute, int exact_int,
                     VecMeta *meta, int8_t *q, const double *d_W2 = nullptr) {
  hipStream_t st = op->bed->stream;
  const bool bytes = op->bed->bits == 8;
  const double vstep = bytes ? op->bed->v_step : 1.0, voff = bytes ? op->bed->v_off : 0.0;
  const int raw3 = (!bytes && mode == 1) ? 1 : 0;
  if (bytes) permute = 0;  // the byte image holds the samples of a 16-block in natural order
  if (permute == 2 && !(mode == 1 && (raw3 & 1))) fail("internal: the interleaved digit rows are the scaled product's");
  // meta: kMetaVecs records, then the slice maxima of k_absmax (kMetaVecs x 256 x 2 doubles)
  double *part = (double *)(meta + kMetaVecs);
  int gx = 0;
  if (exact_int) {
    hipLaunchKernelGGL(k_meta_clear, dim3(1), dim3(64), 0, st, meta, nvec);
  } else {
    gx = (int)((len + 1023) / 1024);
    if (gx > 256) gx = 256;
    hipLaunchKernelGGL(k_absmax, dim3(gx, nvec), dim3(1024), 0, st, d_X, ldx, len,
                       mode == 1 ? op->d_center.p : mode == 2 ? d_W2 : nullptr,
                       mode == 1 ? op->d_scale.p : nullptr, mode, meta, part, vstep, voff, raw3);
  }
  // (no memset of q: k_quant writes every digit row of the columns in use, zeros past `len`; the columns
  // of a column block that no vector uses keep stale bytes, which only reach accumulator columns that no
  // finalize kernel reads)
  int64_t nblk = len_pad / 16;
  const double *qc = mode == 1 ? op->d_center.p : mode == 2 ? d_W2 : nullptr;
  const double *qsc = mode == 1 ? op->d_scale.p : nullptr;
  const dim3 qgrid((unsigned)((nblk + 63) / 64), nvec);
#define BSN_QUANT(SV)                                                                                  \
  case SV:                                                                                             \
    if (permute == 2)                                                                                  \
      hipLaunchKernelGGL((k_quant<SV, 2>), qgrid, dim3(64), 0, st, d_X, ldx, len, len_pad, qc, qsc, mode, \
                         ncol, meta, q, vstep, voff, raw3, part, gx);                                  \
    else if (permute)                                                                                  \
      hipLaunchKernelGGL((k_quant<SV, 1>), qgrid, dim3(64), 0, st, d_X, ldx, len, len_pad, qc, qsc, mode, \
                         ncol, meta, q, vstep, voff, raw3, part, gx);                                  \
    else                                                                                               \
      hipLaunchKernelGGL((k_quant<SV, 0>), qgrid, dim3(64), 0, st, d_X, ldx, len, len_pad, qc, qsc, mode, \
                         ncol, meta, q, vstep, voff, raw3, part, gx);                                  \
    break;
  switch (S) {
    BSN_QUANT(1) BSN_QUANT(2) BSN_QUANT(3) BSN_QUANT(4) BSN_QUANT(5) BSN_QUANT(6) BSN_QUANT(7) BSN_QUANT(8)
    default: fail("slices must be in 1..8");
  }
#undef BSN_QUANT
  BSN_HIP(hipGetLastError());
}

static const double *scatter_rows_if_needed(bsn_op *op, const double *d_X, int64_t *ldx,
                                            int nvec) {
  if (op->rows_identity) return d_X;
  bsn_bed *b = op->bed;
  double *xf = op->d_xfull.ensure((size_t)b->n * nvec);
  BSN_HIP(hipMemsetAsync(xf, 0, (size_t)b->n * nvec * sizeof(double), b->stream));
  hipLaunchKernelGGL(k_scatter_rows, dim3((unsigned)((op->n + 255) / 256), nvec), dim3(256), 0,
                     b->stream, d_X, *ldx, op->d_rows.p, op->n, xf, b->n);
  BSN_HIP(hipGetLastError());
  *ldx = b->n;
  return xf;
}

// binomial scaling from the code counts (R/binom-scaling.R:133-142 on the sums of
// src/bed-fun.cpp:22-38: sumX = n1 + 2 n2, nb_nona = n - nNA), same operations in the same order
#pragma clang fp contract(off)
__global__ void k_binom_scale(const int32_t *counts, int64_t m, double *center, double *scale) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int4 c = *(const int4 *)(counts + 4 * j);
  const double sumX = (double)(c.y + 2 * c.z);
  const double nona = (double)(c.x + c.y + c.z);
  const double af = sumX / (2.0 * nona);
  center[j] = 2.0 * af;
  scale[j] = sqrt(2.0 * af * (1.0 - af));
}
#pragma clang fp contract(on)

// by-products of the counting pass, all on the device: the total number of missing genotypes (decides
// whether the solve may drop the missing-value plane), the number of variants with more than 50 % missing
// (the warning of bed_colstats, src/bed-fun.cpp:40-41) and the per-variant missing counts the handle keeps.
// Integer atomics: exact and order-independent.  out[0] = total, out[1] = n_bad (both cleared by the caller).
__global__ __launch_bounds__(256) void k_stats_summary(const int32_t *counts, int64_t m, int64_t n, int32_t *na,
                                                       unsigned long long *out) {
  long long s = 0, bad = 0;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < m; j += (int64_t)gridDim.x * 256) {
    const int4 c = *(const int4 *)(counts + 4 * j);
    s += c.w;
    na[j] = c.w;
    if (2 * ((int64_t)c.x + c.y + c.z) < n) bad++;
  }
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off);
    bad += __shfl_down(bad, off);
  }
  __shared__ long long sw[4], sb[4];
  if ((threadIdx.x & 63) == 0) {
    sw[threadIdx.x >> 6] = s;
    sb[threadIdx.x >> 6] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s = sw[0] + sw[1] + sw[2] + sw[3];
    bad = sb[0] + sb[1] + sb[2] + sb[3];
    if (s) atomicAdd(&out[0], (unsigned long long)s);
    if (bad) atomicAdd(&out[1], (unsigned long long)bad);
  }
}

// the streaming-layout copy serves an operator over a 64-aligned contiguous range of variants
static bool use_tiled(const bsn_op *op) {
  return op->bed->d_tiled != nullptr && op->cols_contig && (op->col0 & 63) == 0;
}

// compute units of the device (the slab rules of k_prodT and k_cprod fill whole rounds of them)
static int device_cus() {
  static const int ncu = [] {
    hipDeviceProp_t pr;
    int dev = 0;
    return (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0)
               ? pr.multiProcessorCount : 256;
  }();
  return ncu;
}

// The grid of a k_cprod launch that takes the geometry (prod_plan.hpp: plan_cprod).  How many workgroups of the instance a CU
// holds is the runtime's answer, asked once per instance.  BSN_PLAN_CUS=<n>: the CU count assumed, as for k_prodT
// (tests/test_gpu_cprod_whole.py; same sums, read on every call).
static thread_local CprodGridFacts g_cprod_facts;   // what the last plan was made from (op_cprod_grid)
static CprodGrid cprod_geometry(bsn_op *op, const void *kern, int per_wg, int threads, int NB, int nplane) {
  static std::mutex mu;
  static std::map<const void *, int> held;
  int resident;
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = held.find(kern);
    if (it == held.end()) {
      int nb = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, threads, 0) != hipSuccess || nb < 1) nb = 1;
      it = held.emplace(kern, nb).first;
    }
    resident = it->second;
  }
  CprodGridFacts f;
  f.m = op->m, f.per_wg = per_wg, f.nchunks = (int)(op->bed->pitch * 4 / 512), f.pitch = op->bed->pitch;
  f.NB = NB, f.nplane = nplane, f.ncu = device_cus(), f.resident = resident;
  if (const char *e = getenv("BSN_PLAN_CUS")) f.ncu = std::max(1, atoi(e));
  // BSN_CPROD_SLABS=<c>: that many slabs for the remainder blocks instead of the rule's count (same sums, read on every call)
  if (const char *e = getenv("BSN_CPROD_SLABS")) f.slabs = std::max(1, atoi(e));
  g_cprod_facts = f;
  return plan_cprod(f);
}

// One crossproduct launch: the instance that choose_cprod (prod_plan.hpp) names, on the image it reads.  The list below is
// the instances that exist — the counting and the three-plane pass have no three-block kernel, only the plain pass has
// skipping ones; tiles per wave on the tiled copy: 4, the counting pass 2.
// geo (op_cprod): null — one workgroup per block of variants, the instance's old grid.  Otherwise the call either PLANS
// (acc == nullptr: *geo becomes the grid of cprod_slab for the instance this launch takes, from what the runtime says a CU
// holds of it; the caller sizes d_acc by it) or LAUNCHES on *geo, the partial sums of the remainder blocks going to `part`.
template <int NPLANE, bool RAW0, bool STATS>
static void launch_cprod(bsn_op *op, int NB, const int8_t *q, int32_t *acc, uint32_t l0,
                         uint32_t l1, uint32_t l2, int32_t *counts = nullptr, CprodGrid *geo = nullptr,
                         int32_t *part = nullptr) {
  bsn_bed *b = op->bed;
  constexpr int KC = 512, TT = STATS ? 2 : 4;
  constexpr bool PLAIN = NPLANE == 2 && RAW0 && !STATS;
  // int32 accumulators over the whole sample range: a plane adds at most 4 * 128 per sample
  if (b->pitch * 4 > 4000000) fail("more than 4e6 samples are not supported by the crossproduct kernel");
  const int32_t *cols = op->cols_contig ? nullptr : op->d_cols.p;
  const int32_t npad = (int32_t)(b->pitch * 4 - b->n);
  CprodFacts f;
  f.NB = NB, f.plain = PLAIN, f.stats = STATS, f.cols_contig = op->cols_contig, f.tiled = use_tiled(op);
  f.warm = op->prof_kind_override == 3, f.na_skip = op->na_skip_c;
  const CprodKernel k = choose_cprod(f);
  const uint8_t *image = k.tiled ? b->d_tiled : b->d_img;
  const int per_wg = 16 * k.tiles * k.waves;   // variants of a workgroup
  // the instances that take the geometry (k_cprod: GEO); BSN_CPROD_ONE_SPLIT=1: none (A/B switch, bit-identical; read on every call)
  const bool geo_ok = geo && k.contig && !k.tiled && !STATS && NPLANE < 3 && !getenv("BSN_CPROD_ONE_SPLIT");
  CprodGrid one;   // the old grid in the new terms: every block a whole-round block
  one.blocks = one.blocks_whole = (int)((op->m + per_wg - 1) / per_wg), one.nchunks = (int)(b->pitch * 4 / KC);
  const bool planning = geo && !acc;
  if (planning && !geo_ok) {
    *geo = one;
    return;
  }
  const CprodGrid g = geo && !planning ? *geo : one;
  const dim3 grid((unsigned)cprod_workgroups(g)), block(64 * k.waves);
#define BSN_CPROD(NBV, CONTIGV, TV, WV, TAGV, TILEDV, SGBV, NASKIPV)                                                   \
  if (k == CprodKernel{NBV, CONTIGV, TV, WV, TAGV, TILEDV, SGBV, NASKIPV}) {                                           \
    auto kern = k_cprod<NBV, NPLANE, KC, RAW0, STATS, CONTIGV, TV, WV, 1, TAGV, TILEDV, SGBV, NASKIPV>;                \
    if (planning) {                                                                                                    \
      *geo = cprod_geometry(op, (const void *)kern, per_wg, 64 * k.waves, NB, NPLANE);                                 \
      return;                                                                                                          \
    }                                                                                                                  \
    BSN_KLAUNCH(kern, grid, block, 0, b->stream, image, b->pitch, cols, op->col0, op->m, q, acc, op->m, l0, l1, l2,    \
                counts, npad, g, part);                                                                                \
    BSN_HIP(hipGetLastError());                                                                                        \
    return;                                                                                                            \
  }
  BSN_CPROD(1, false, 2, 8, 0, false, 0, false)
  BSN_CPROD(1, true, 2, 8, 0, false, 0, false)
  BSN_CPROD(1, true, 2, 8, 1, false, 0, false)
  BSN_CPROD(1, true, TT, 8, 0, true, 0, false)
  BSN_CPROD(1, true, TT, 8, 1, true, 0, false)
  BSN_CPROD(2, false, 2, 16, 0, false, 0, false)
  BSN_CPROD(2, true, 2, 16, 0, false, 3, false)
  BSN_CPROD(2, true, 2, 16, 0, true, 3, false)
  if constexpr (!STATS && NPLANE < 3) {
    BSN_CPROD(3, false, 2, 16, 0, false, 0, false)
    BSN_CPROD(3, true, 2, 16, 0, false, 3, false)
  }
  if constexpr (PLAIN) {
    BSN_CPROD(2, false, 2, 16, 0, false, 0, true)
    BSN_CPROD(2, true, 2, 16, 0, false, 0, true)
    BSN_CPROD(3, false, 2, 16, 0, false, 0, true)
    BSN_CPROD(3, true, 2, 16, 0, false, 0, true)
  }
#undef BSN_CPROD
  fail("internal: no crossproduct kernel with %d column blocks for this pass", NB);
}

// z = finalize of a crossproduct launch of NB column blocks
// (geo.slabs > 0: the variants of k_cprod's remainder blocks have their sums in the slabs of `part`)
static void launch_cprod_final(bsn_op *op, int NB, const int32_t *acc, int S, int nv, const VecMeta *meta, double *Z,
                               int64_t ldz, bool has_q, const CprodGrid &geo, const int32_t *part) {
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)((op->m + 127) / 128)), dim3(128), 0, op->bed->stream, acc, op->m, S, nv, meta,
                       op->d_center.p, op->d_scale.p, Z, ldz, has_q ? 1 : 0, part, geo.m_rem, geo.slabs);
  };
  if (NB == 1) go(k_cprod_final<16>);
  else if (NB == 2) go(k_cprod_final<32>);
  else go(k_cprod_final<48>);
  BSN_HIP(hipGetLastError());
}

// The scaling statistics of a solve ride along its first crossproduct pass: counts of the codes
// -> centre / scale on the device, before the finalize kernel needs them.
static void finish_fused_stats(bsn_op *op) {
  bsn_bed *b = op->bed;
  hipLaunchKernelGGL(k_binom_scale, dim3((unsigned)((op->m + 255) / 256)), dim3(256), 0, b->stream,
                     op->d_counts.p, op->m, op->d_center.p, op->d_scale.p);
  BSN_HIP(hipGetLastError());
  op->stats_pending = false;
  // missing-value total (and the > 50 % missing count) -> pinned host words, picked up by op_poll_stats at the
  // caller's next sync
  if (!op->h_na_total) BSN_HIP(hipHostMalloc((void **)&op->h_na_total, 2 * sizeof(long long), hipHostMallocDefault));
  op->h_na_total[0] = -1;
  op->h_na_total[1] = -1;
  unsigned long long *d_tot = (unsigned long long *)(op->d_counts.p + 4 * op->m);  // four spare words behind the counts
  BSN_HIP(hipMemsetAsync(d_tot, 0, 16, b->stream));
  int gx = (int)((op->m + 1023) / 1024);
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(k_stats_summary, dim3(gx), dim3(256), 0, b->stream, op->d_counts.p, op->m, op->n,
                     op->d_na.ensure((size_t)op->m), d_tot);
  BSN_HIP(hipGetLastError());
  BSN_HIP(hipMemcpyAsync(op->h_na_total, d_tot, 16, hipMemcpyDeviceToHost, b->stream));
  op->na_poll = true;
}

void op_poll_stats(bsn_op *op) {
  if (!op->na_poll || !op->h_na_total) return;
  const long long t = *(volatile long long *)op->h_na_total;
  if (t < 0) return;
  op->na_poll = false;
  if (t == 0 && !getenv("BSN_FORCE_NA_PLANE")) op->no_na = true;  // complete data: skip the missing-value plane from now on
}

// ---------------------------------------------------------------------------
// How many K-steps of the streaming products carry no missing code?  (round 5, VERDICT r4 #5b)  The missing-value plane
// is half the MFMAs of k_cprod / k_prodT; a K-step whose 1 024 genotypes hold no missing code adds zeros through it.
// At 1 % scattered missing values no step is free (0.99^1024); on nearly complete data (1e-4: 90 %) or on data whose
// missing values come in batches (arrays merged over sample sets) most are.  k_na_blocks tests a SAMPLE of steps with
// exactly the kernels' test, in the kernels' two step shapes, on the variant-major image:
//   crossproduct  wave = 16 variants (lane & 15) x one 64-byte segment (4 x 16 B, lane >> 4): dword d of every lane is
//                 K-step d — four steps per wave
//   product       wave = one dword column (16 samples) x 256 variants of one half chunk: lane (c, g), step d reads
//                 variant j0 + 64 g + 16 d + c — four steps per wave
// out: {free, sampled} steps of the two shapes, then 1 (the arrival flag of the pinned copy).
__device__ __forceinline__ uint32_t hash32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
__global__ __launch_bounds__(64) void k_na_blocks(const uint8_t *__restrict__ img, int64_t pitch, int64_t m,
                                                  unsigned long long *out) {
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const uint32_t h = hash32((uint32_t)blockIdx.x * 0x9E3779B1u + 0x7F4A7C15u), h2 = hash32(h ^ 0x85EBCA6Bu);
  const int64_t nseg = pitch / 64, ngrp = m / 16, nhalf = m / 256, ndw = pitch / 4;
  int free_c = 0, free_p = 0, tot_c = 0, tot_p = 0;
  if (ngrp > 0 && nseg > 0) {
    const int64_t grp = (int64_t)(((uint64_t)h * (uint64_t)ngrp) >> 32), seg = (int64_t)(((uint64_t)h2 * (uint64_t)nseg) >> 32);
    const uint4 w = *(const uint4 *)(img + (grp * 16 + c) * pitch + seg * 64 + g * 16);
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int d = 0; d < 4; d++)
      free_c += __builtin_amdgcn_ballot_w64(((ws[d] & (ws[d] >> 1)) & 0x55555555u) != 0u) == 0ull;
    tot_c = 4;
  }
  if (nhalf > 0 && ndw > 0) {
    const int64_t hc = (int64_t)(((uint64_t)h2 * (uint64_t)nhalf) >> 32), dw = (int64_t)(((uint64_t)h * (uint64_t)ndw) >> 32);
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const uint32_t w = *(const uint32_t *)(img + (hc * 256 + 64 * g + 16 * d + c) * pitch + dw * 4);
      free_p += __builtin_amdgcn_ballot_w64(((w & (w >> 1)) & 0x55555555u) != 0u) == 0ull;
    }
    tot_p = 4;
  }
  if (lane == 0) {
    atomicAdd(&out[0], (unsigned long long)free_c);
    atomicAdd(&out[1], (unsigned long long)tot_c);
    atomicAdd(&out[2], (unsigned long long)free_p);
    atomicAdd(&out[3], (unsigned long long)tot_p);
  }
}

// BSN_NA_SKIP=0 / 1: never / always the skipping kernels (A/B runs and tests; results are the same integers either
// way); BSN_NA_SKIP_MIN: the share of free steps from which they are used (default 0.30: they cost 4 VALU and a
// branch per step and do without the explicit MFMA / decode schedule, profiles/r05_power.txt).
void op_na_blocks(bsn_op *op, int digit_cols) {
  bsn_bed *b = op->bed;
  op->na_skip_c = op->na_skip_p = false;
  // (one column block — the one-shot products, 8-vector solves — has no skipping kernel: nothing to measure for)
  if (b->bits != 2 || b->generic || op->no_na || !b->d_img || digit_cols <= 16) return;
  const char *fe = getenv("BSN_NA_SKIP");   // (read at every call: the tests switch it between two products)
  const int force = fe ? atoi(fe) : -1;
  if (force == 0) return;
  if (force == 1) {
    op->na_skip_c = op->na_skip_p = true;
    return;
  }
  const char *me = getenv("BSN_NA_SKIP_MIN");
  const double min_free = me ? atof(me) : 0.30;
  if (b->na_blocks_state == 0) {
    if (!b->h_na_blocks) BSN_HIP(hipHostMalloc((void **)&b->h_na_blocks, 5 * sizeof(long long), hipHostMallocDefault));
    if (!b->d_na_blocks) BSN_HIP(hipMalloc((void **)&b->d_na_blocks, 5 * sizeof(long long)));
    for (int i = 0; i < 5; i++) b->h_na_blocks[i] = -1;   // [4] stays -1 until the second copy below has landed
    BSN_HIP(hipMemsetAsync(b->d_na_blocks, 0, 5 * sizeof(long long), b->stream));
    constexpr int kSamples = 8192;   // waves = 32 768 steps of each shape: the share to about half a percent
    hipLaunchKernelGGL(k_na_blocks, dim3(kSamples), dim3(64), 0, b->stream, b->d_img, b->pitch, b->m,
                       (unsigned long long *)b->d_na_blocks);
    BSN_HIP(hipGetLastError());
    // the counts first, the flag word (one byte set to 1) in a copy of its own behind them: it arrives last
    BSN_HIP(hipMemsetAsync((uint8_t *)b->d_na_blocks + 4 * sizeof(long long), 1, 1, b->stream));
    BSN_HIP(hipMemcpyAsync(b->h_na_blocks, b->d_na_blocks, 4 * sizeof(long long), hipMemcpyDeviceToHost, b->stream));
    BSN_HIP(hipMemcpyAsync(b->h_na_blocks + 4, b->d_na_blocks + 4, sizeof(long long), hipMemcpyDeviceToHost, b->stream));
    b->na_blocks_state = 1;
    return;
  }
  if (b->na_blocks_state == 1) {
    if (*(volatile long long *)(b->h_na_blocks + 4) != 1) return;   // not there yet: the plain kernels meanwhile
    const long long *v = b->h_na_blocks;
    b->na_free[0] = v[1] > 0 ? (double)v[0] / (double)v[1] : 0.0;
    b->na_free[1] = v[3] > 0 ? (double)v[2] / (double)v[3] : 0.0;
    b->na_blocks_state = 2;
  }
  op->na_skip_c = b->na_free[0] >= min_free;
  op->na_skip_p = b->na_free[1] >= min_free;
}

static int cprod_vmax(const bsn_op *op, int S) { return cprod_vmax(op->bed->bits, op->stats_pending, S); }

void op_cprod_prequant(bsn_op *op, const double *d_X, int64_t ldx, int nvec) {
  bsn_bed *b = op->bed;
  const int S = op->slices;
  op->preq_X = nullptr;
  if (nvec <= 0 || nvec > cprod_vmax(op, S) || !op->rows_identity) return;
  const int64_t npad = n_padded(b);
  quantise(op, d_X, ldx, b->n, npad, nvec, 0, S, 16 * pick_nb(nvec * S), 1, 0, meta_buffer(op),
           op->d_q.ensure((size_t)npad * kMaxCols * 2));
  op->preq_X = d_X;
  op->preq_ldx = ldx;
  op->preq_nvec = nvec;
  op->preq_S = S;
}

// The crossproduct launch on the 2-bit image, by what the operator knows: counting along / complete data / the plain pass
// (acc == nullptr: only the grid of that launch, into *geo — see launch_cprod)
static void cprod_on_image(bsn_op *op, int NB, const int8_t *q, int32_t *acc, CprodGrid *geo, int32_t *part) {
  if (op->stats_pending) {
    if (!op->rows_identity) fail("internal: fused scaling statistics need all samples");
    launch_cprod<2, true, true>(op, NB, q, acc, kLutRaw, kLutNA, 0, op->d_counts.ensure((size_t)4 * op->m + 8), geo, part);
  } else if (op->no_na) {
    launch_cprod<1, true, false>(op, NB, q, acc, kLutRaw, 0, 0, nullptr, geo, part);  // complete variants: code == genotype
  } else {
    launch_cprod<2, true, false>(op, NB, q, acc, kLutRaw, kLutNA, 0, nullptr, geo, part);
  }
}

// The grid the first launch of op_cprod over nvec vectors would take now (tests: the geometry of a case is asserted before the
// GPU runs it).  out: blocks, blocks_whole, slabs, cps, nchunks, m_rem, then what the plan was made from — variants per
// workgroup, CUs, workgroups of the instance a CU holds (0, 0, 0: an instance without the geometry, or the switch).
void op_cprod_grid(bsn_op *op, int nvec, int64_t *out) {
  require_bits(op->bed, 2, "the grid of k_cprod");
  if (nvec <= 0) fail("op_cprod_grid: no vectors");
  CprodGrid g;
  g_cprod_facts = CprodGridFacts();
  g_cprod_facts.per_wg = g_cprod_facts.ncu = g_cprod_facts.resident = 0;
  const int S = op->slices;
  op_na_blocks(op, nvec * S);
  cprod_on_image(op, pick_nb(std::min(nvec, cprod_vmax(op, S)) * S), nullptr, nullptr, &g, nullptr);
  out[0] = g.blocks, out[1] = g.blocks_whole, out[2] = g.slabs, out[3] = g.cps, out[4] = g.nchunks, out[5] = g.m_rem;
  out[6] = g_cprod_facts.per_wg, out[7] = g_cprod_facts.ncu, out[8] = g_cprod_facts.resident;
}
void op_cprod(bsn_op *op, const double *d_X, int64_t ldx, int nvec, double *d_Z, int64_t ldz) {
  bsn_bed *b = op->bed;
  refuse_generic(b, "this function (it needs the streaming products)");
  const int S = op->slices;
  if (nvec <= 0) return;
  if (b->bits == 8 && byte_slices(b->pitch) > kByteMaxSlices)
    fail("the crossproduct on a dosage FBM supports at most %lld samples", (long long)(kByteMaxSlices * kSliceBytes));
  op_na_blocks(op, nvec * S);
  const bool have_digits = op->preq_X == d_X && op->preq_ldx == ldx && op->preq_nvec == nvec && d_X != nullptr &&
                           op->preq_S == S && nvec <= cprod_vmax(op, S);
  op->preq_X = nullptr;
  const double *xsrc = scatter_rows_if_needed(op, d_X, &ldx, nvec);
  const int64_t npad = n_padded(b);
  VecMeta *meta = meta_buffer(op);
  for (int v0 = 0, vmax = 0; v0 < nvec; v0 += vmax) {
    vmax = cprod_vmax(op, S);  // vectors of this launch (the launch that counts the codes is limited to two column blocks)
    int nv = nvec - v0 < vmax ? nvec - v0 : vmax;
    int NB = pick_nb(nv * S), ncol = 16 * NB;
    int8_t *q = op->d_q.ensure((size_t)npad * kMaxCols * 2);
    // (byte image: one block of partial sums per 131 072-sample slice)
    const int nslice = b->bits == 8 ? byte_slices(b->pitch) : 1;
    CprodGrid geo;   // the grid of the launch, before the accumulators are sized
    if (b->bits == 2) cprod_on_image(op, NB, q, nullptr, &geo, nullptr);
    // (behind the accumulators of the largest launch: the partial sums of the remainder blocks, prod_plan.hpp)
    const size_t acc_words = std::max((size_t)2 * op->m * kMaxCols, (size_t)nslice * 2 * op->m * ncol);
    const size_t part_words = (size_t)cprod_partial_words(geo, op->stats_pending || !op->no_na ? 2 : 1, NB);
    int32_t *acc = op->d_acc.ensure(acc_words + part_words);
    int32_t *part = acc + acc_words;
    if (!have_digits) quantise(op, xsrc + (int64_t)v0 * ldx, ldx, b->n, npad, nv, 0, S, ncol, 1, 0, meta, q);
    prof_begin(op, op->stats_pending ? 2 : NB == 3 ? 4 : 0);  // the pass that carries the code counts is timed apart
    if (b->bits == 8) {
      const dim3 grid8((unsigned)((op->m + 127) / 128), (unsigned)nslice);
      const int32_t *cols8 = op->cols();
#define BSN_CPROD8(NBV, NAV, CV)                                                                          \
  BSN_KLAUNCH((k_cprod8<NBV, NAV, CV>), grid8, dim3(512), 0, b->stream, b->d_img, b->pitch, cols8, \
                     op->col0, op->m, q, acc, op->m, (int)(kSliceBytes / 256))
      if (NB == 1) {
        if (op->no_na) { if (op->cols_contig) BSN_CPROD8(1, false, true); else BSN_CPROD8(1, false, false); }
        else { if (op->cols_contig) BSN_CPROD8(1, true, true); else BSN_CPROD8(1, true, false); }
      } else {
        if (op->no_na) { if (op->cols_contig) BSN_CPROD8(2, false, true); else BSN_CPROD8(2, false, false); }
        else { if (op->cols_contig) BSN_CPROD8(2, true, true); else BSN_CPROD8(2, true, false); }
      }
#undef BSN_CPROD8
      BSN_HIP(hipGetLastError());
      prof_end(op);
      op->passes++;
      hipLaunchKernelGGL(k_cprod_final8, dim3((unsigned)((op->m + 255) / 256), nv), dim3(256), 0, b->stream, acc,
                         op->m, ncol, S, meta, op->d_center.p, op->d_scale.p, d_Z + (int64_t)v0 * ldz, ldz,
                         op->no_na ? 0 : 1, b->v_step, b->v_off, nslice);
      BSN_HIP(hipGetLastError());
      continue;
    }
    cprod_on_image(op, NB, q, acc, &geo, part);
    prof_end(op);
    op->passes++;
    if (op->late_center || op->late_scale) {
      // staged and sent while the streaming kernel runs; the finalize kernel waits for them
      hipStream_t up = upload_stream(b);
      if (op->late_center) copy_h2d(b, op->d_center.p, op->late_center, (size_t)op->m * 8, up);
      if (op->late_scale) copy_h2d(b, op->d_scale.p, op->late_scale, (size_t)op->m * 8, up);
      BSN_HIP(hipEventRecord(b->ev_up, up));
      BSN_HIP(hipStreamWaitEvent(b->stream, b->ev_up, 0));
      op->late_center = op->late_scale = nullptr;
    }
    const bool has_q = op->stats_pending || !op->no_na;
    if (op->stats_pending) finish_fused_stats(op);
    launch_cprod_final(op, NB, acc, S, nv, meta, d_Z + (int64_t)v0 * ldz, ldz, has_q, geo, part);
  }
}

// One launch of k_prod: the instance that choose_prod (prod_plan.hpp) names, on the variant-major image or its tiled copy
// (same arithmetic, contiguous 16-KB steps)
static void launch_prod(bsn_op *op, int NB, dim3 grid, int64_t m_pad, int64_t mc, const int8_t *q, int32_t *acc,
                        int64_t npad, uint32_t lutP, uint32_t lutQ, bool has_q) {
  bsn_bed *b = op->bed;
  const int32_t *cols = op->d_cols.p;
  const ProdKernel k = choose_prod(NB, op->cols_contig, use_tiled(op), lutP == kLutRaw, has_q, op->prof_kind_override == 3);
  const uint8_t *image = k.tiled ? b->d_tiled : b->d_img;
#define BSN_PROD(NBV, CV, RAWP, HASQ, TAGV, TILEDV)                                                                  \
  if (k == ProdKernel{NBV, CV, RAWP, HASQ, TAGV, TILEDV}) {                                                          \
    BSN_KLAUNCH((k_prod<NBV, CV, RAWP, HASQ, TAGV, TILEDV>), grid, dim3(256), 0, b->stream, image, b->pitch, cols,   \
                op->col0, m_pad, mc, q, acc, npad, lutP, lutQ);                                                      \
    BSN_HIP(hipGetLastError());                                                                                      \
    return;                                                                                                          \
  }
  // with / without the second plane, each with its warm-start name, on the raw codes; the same through a look-up
#define BSN_PROD6(NBV, CV, TILEDV)                                                                \
  BSN_PROD(NBV, CV, true, true, 0, TILEDV) BSN_PROD(NBV, CV, true, true, 1, TILEDV)               \
  BSN_PROD(NBV, CV, true, false, 0, TILEDV) BSN_PROD(NBV, CV, true, false, 1, TILEDV)             \
  BSN_PROD(NBV, CV, false, true, 0, TILEDV) BSN_PROD(NBV, CV, false, false, 0, TILEDV)
  BSN_PROD6(1, true, false) BSN_PROD6(1, true, true) BSN_PROD6(1, false, false)
  BSN_PROD6(2, true, false) BSN_PROD6(2, true, true) BSN_PROD6(2, false, false)
#undef BSN_PROD6
#undef BSN_PROD
  fail("internal: no product kernel with %d column blocks", NB);
}

// One launch of k_prodT on the sample-major copy: the instance that choose_prodT (prod_plan.hpp) names.
// (workgroup shapes 4 x 8 / 4 x 4 / 2 x 8 / 4 x 16 tiles x waves, chunks of 256 variants: all slower, profiles/r04_sample_major.txt)
// seg_bs > 0: a segment's two-dimensional grid `seg_grid`; otherwise the one-dimensional grid of `geo` (prodt_slab)
static void launch_prodT(bsn_op *op, const ProdTKernel &k, const ProdTGrid &geo, dim3 seg_grid, const int8_t *q, int32_t *acc,
                         int64_t npad, uint32_t lutQ, int seg_bs, int seg_stride, int seg_off) {
  bsn_bed *b = op->bed;
  const dim3 grid = seg_bs > 0 ? seg_grid : dim3((unsigned)prodt_workgroups(geo));
#define BSN_PRODT(NBV, HASQV, TAGV, SGBV, NASKIPV, SPARSEV)                                                           \
  if (k == ProdTKernel{NBV, HASQV, TAGV, SGBV, NASKIPV, SPARSEV}) {                                                   \
    BSN_KLAUNCH((k_prodT<NBV, HASQV, 2, 16, TAGV, SGBV, NASKIPV, SPARSEV>), grid, dim3(1024), 0, b->stream, b->d_smaj, \
                b->rows_smaj, op->col0 / 512, geo, q, acc, npad, lutQ, seg_bs, seg_stride, seg_off);                  \
    BSN_HIP(hipGetLastError());                                                                                       \
    return;                                                                                                           \
  }
  BSN_PRODT(2, true, 0, 3, false, false) BSN_PRODT(2, true, 1, 3, false, false)
  BSN_PRODT(2, false, 0, 3, false, false) BSN_PRODT(2, false, 1, 3, false, false)
  BSN_PRODT(3, true, 0, 3, false, false) BSN_PRODT(3, false, 0, 3, false, false)
  BSN_PRODT(2, true, 0, 0, true, false) BSN_PRODT(3, true, 0, 0, true, false)
  BSN_PRODT(3, true, 0, 3, false, true) BSN_PRODT(3, true, 1, 3, false, true)
#undef BSN_PRODT
  fail("internal: no sample-major product kernel with %d column blocks", k.NB);
}

// y = finalize of a product launch of NB column blocks over `rows` output rows (blk_rows > 0: a segment's blocked output)
// (rows_whole > 0: the image rows of k_prodT's whole-round blocks, which have ky_whole slabs)
static void launch_prod_final(bsn_bed *b, int NB, const int32_t *acc, int64_t npad, int ky, int64_t rows_whole, int ky_whole, int S,
                              int nv, const VecMeta *meta,
                              const int32_t *d_rows, int64_t rows, double *Y, int64_t ldy, int sub_const, double beta,
                              int64_t blk_rows) {
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, b->stream, acc, npad, ky, rows_whole, ky_whole, S,
                       nv, meta, d_rows, rows, Y, ldy, sub_const, beta, blk_rows);
  };
  if (NB == 1) go(k_prod_final<16>);
  else if (NB == 2) go(k_prod_final<32>);
  else go(k_prod_final<48>);
  BSN_HIP(hipGetLastError());
}

// Y (+)= sum_j P[code_ij] W1[j, v] + sum_j lutQ[code_ij] W2[j, v]  (- sum_j W2[j, v] if sub_const)
// P = lutP look-up, or the code itself when lutP == kLutRaw.
// mode 1: W1 = X / scale, W2 = center * W1 derived from the operator's centre / scale (the
// scaled product A~ X; lutP must be kLutRaw and lutQ kLutNA: the quantiser then stores W2 - 3 W1
// in the second plane, see k_quant); mode 2: W1 = d_X, W2 = d_W2 given directly (raw plane weights).
struct ProdSegments {   // op_prod_segments
  int pieces, stride, nseg;
  const ProdSegment *segs;
  const std::function<void(int)> *after;
  bool done = false;
};
static void prod_planes(bsn_op *op, const double *d_X, const double *d_W2, int64_t ldx, int nvec,
                        double *d_Y, int64_t ldy, int mode, uint32_t lutP, uint32_t lutQ, int sub_const,
                        double beta, int S, ProdSegments *sg = nullptr) {
  bsn_bed *b = op->bed;
  refuse_generic(b, "this function (it needs the streaming products)");
  if (nvec <= 0) return;
  op->preq_X = nullptr;
  op_na_blocks(op, nvec * S);
  if (b->smaj_job) (void)image_smaj_poll(b);   // a copy being made beside this solve: has it arrived?
  // complete variants: the missing-value plane is all zero, skip its look-ups and MFMAs
  const bool has_q = lutQ != 0u && !(op->no_na && lutQ == kLutNA);
  // the geometry of the pass (prod_plan.hpp): k_prodT on the sample-major copy or k_prod, vectors per launch, slabs
  ProdFacts f;
  f.bits = b->bits, f.n = b->n, f.m = op->m, f.pitch = b->pitch, f.col0 = op->col0, f.cols_contig = op->cols_contig;
  f.have_smaj = b->d_smaj != nullptr && !getenv("BSN_NO_SMAJ");
  f.mode = mode, f.raw_na = lutP == kLutRaw && lutQ == kLutNA, f.has_q = has_q;
  f.no_sparse = getenv("BSN_NO_SPARSE_PROD") != nullptr;   // (A/B switch, bit-identical; read on every call)
  f.nvec = nvec, f.S = S, f.segmented = sg != nullptr;
  if (f.have_smaj) f.ncu = device_cus();
  // BSN_PLAN_CUS=<n>: the CU count the planner assumes (small shapes never fill a round of 256 CUs: with 4 they take
  // k_prodT's whole-round geometry, tests/test_gpu_prodt_whole.py; same sums, read on every call)
  if (const char *e = getenv("BSN_PLAN_CUS")) f.ncu = std::max(1, atoi(e));
#ifdef BSN_ABLATION
  if (const char *e = getenv("BSN_KY")) f.ky = std::max(1, atoi(e));      // slab sweeps (correct results)
  if (const char *e = getenv("BSN_KY_T")) f.ky_t = std::max(1, atoi(e));
  if (const char *e = getenv("BSN_KY_WHOLE")) f.ky_whole = std::max(1, atoi(e));
#endif
  const ProdPlan pl = plan_prod(f);
  if (pl.refuse == ProdRefusal::pitch_limit) fail("more than 6.7e7 samples are not supported by the product kernel");
  if (pl.refuse == ProdRefusal::nothing_queued) return;   // (the caller takes the plain pass)
  const bool smaj = pl.smaj;
  const int vmax = pl.vmax, ky = pl.ky, smaj_cps = pl.smaj_cps;
  const int64_t npad = n_padded(b), m_pad = pl.m_pad, mc = pl.mc;
  if (smaj && (int64_t)ky * smaj_cps < m_pad / 512) fail("internal: the slabs of k_prodT do not cover the variants");
  if (smaj && pl.wgx_whole > 0 && (int64_t)pl.ky_whole * pl.cps_whole < m_pad / 512)
    fail("internal: the slabs of k_prodT's whole rounds do not cover the variants");
  // (k_prodT: image rows below rows_whole have ky_whole slabs; k_prod's launches have no such rows)
  const int64_t rows_whole = smaj ? pl.wgx_whole * 512 : 0;
  const int ky_whole = smaj ? pl.ky_whole : 0;
  VecMeta *meta = meta_buffer(op);
  const bool warm = op->prof_kind_override == 3;   // warm-start launches run under their own kernel name (TAG = 1)
  for (int v0 = 0; v0 < nvec; v0 += vmax) {
    int nv = nvec - v0 < vmax ? nvec - v0 : vmax;
    int NB = pick_nb(nv * S), ncol = 16 * NB;
    const ProdTKernel kt = choose_prodT(NB, has_q, warm, op->na_skip_p, pl.sparse_ok);   // (read where smaj && NB >= 2)
    int8_t *q = op->d_q.ensure((size_t)(npad > m_pad ? npad : m_pad) * kMaxCols * 2);
    size_t acc_need = (size_t)std::max(ky, ky_whole) * npad * ncol;
    if (acc_need < (size_t)2 * op->m * kMaxCols) acc_need = (size_t)2 * op->m * kMaxCols;
    int32_t *acc = op->d_acc.ensure(acc_need);
    // (k_prodT decodes like k_cprod: its digit rows take the crossproduct's byte order; the sparse form its own)
    quantise(op, d_X + (int64_t)v0 * ldx, ldx, op->m, m_pad, nv, mode, S, ncol, smaj && NB >= 2 ? (kt.sparse ? 2 : 1) : 0, 0, meta, q,
             d_W2 ? d_W2 + (int64_t)v0 * ldx : nullptr);
    dim3 grid((unsigned)pl.wgx, (unsigned)ky);
    prof_begin(op, NB == 3 ? 5 : 1);
    if (smaj && NB >= 2) {
      const ProdTGrid geo = prodt_grid(pl);
      if (sg) {
        // the pass in segments of sample blocks: kernel + finalize of a segment, then the caller's hook (svd.hip queues the
        // segment's reduce-scatter on its second stream) while the next segment's kernel is queued behind on this one
        for (int sidx = 0; sidx < sg->nseg; sidx++) {
          const ProdSegment &sgm = sg->segs[sidx];
          const dim3 gs((unsigned)(sg->pieces * sgm.bs), (unsigned)ky);
          if (sidx > 0) prof_begin(op, NB == 3 ? 5 : 1, true);
          launch_prodT(op, kt, geo, gs, q, acc, npad, lutQ, sgm.bs, sg->stride, sgm.off);
          prof_end(op);
          const int64_t rows_s = (int64_t)sgm.bs * 512, tot = rows_s * sg->pieces;
          launch_prod_final(b, NB, acc, npad, ky, 0, 0, S, nv, meta, sgm.d_rows, tot, sgm.d_out, 0, sub_const, 0.0, rows_s);
          (*sg->after)(sidx);
        }
        op->passes++;
        sg->done = true;
        continue;
      }
      launch_prodT(op, kt, geo, dim3(), q, acc, npad, lutQ, 0, 0, 0);
    } else if (NB > 2) {
      fail("internal: three column blocks without the sample-major copy");
    } else if (b->bits == 8) {
      if (mode != 1) fail("internal: plane products are not defined on a byte image");
      const int32_t *cols8 = op->d_cols.p;
#define BSN_PROD8(NBV, NAV, CV)                                                                          \
  BSN_KLAUNCH((k_prod8<NBV, NAV, CV>), grid, dim3(256), 0, b->stream, b->d_img, b->pitch, cols8, \
                     op->col0, m_pad, mc, q, acc, npad)
      if (NB == 1) {
        if (op->no_na) { if (op->cols_contig) BSN_PROD8(1, false, true); else BSN_PROD8(1, false, false); }
        else { if (op->cols_contig) BSN_PROD8(1, true, true); else BSN_PROD8(1, true, false); }
      } else {
        if (op->no_na) { if (op->cols_contig) BSN_PROD8(2, false, true); else BSN_PROD8(2, false, false); }
        else { if (op->cols_contig) BSN_PROD8(2, true, true); else BSN_PROD8(2, true, false); }
      }
#undef BSN_PROD8
      BSN_HIP(hipGetLastError());
    } else {
      launch_prod(op, NB, grid, m_pad, mc, q, acc, npad, lutP, lutQ, has_q);
    }
    prof_end(op);
    op->last_kernel = g_last_kernel;
    op->passes++;
    launch_prod_final(b, NB, acc, npad, ky, rows_whole, ky_whole, S, nv, meta, op->rows(), op->n,
                      d_Y + (int64_t)v0 * ldy, ldy, sub_const, beta, 0);
  }
}

// raw plane sums of the cprod kernel: P[j, v] = sum_i g0_ij x_iv, Q[j, v] = sum_i na_ij x_iv
__global__ void k_cprod_raw_final(const int32_t *acc, int64_t m, int ncol, int S, const VecMeta *meta,
                                  double *P, double *Q, int64_t ld) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int v = blockIdx.y;
  if (j >= m) return;
  const double qs = meta[v].qscale;
  const double inv = qs > 0 ? 1.0 / qs : 0.0;
  double p = horner_sub(acc + j * ncol + v * S, acc + (m + j) * ncol + v * S, 3, S) * inv,
         q = horner(acc + (m + j) * ncol + v * S, S) * inv;
  if (meta[v].nonfinite) p = q = __longlong_as_double(0x7ff8000000000000LL);
  P[j + v * ld] = p;
  Q[j + v * ld] = q;
}

void op_cprod_raw(bsn_op *op, const double *d_X, int64_t ldx, int nvec, double *d_P, double *d_Q,
                  int64_t ld) {
  require_bits(op->bed, 2, "the plane sums of multLinReg");
  op->preq_X = nullptr;
  bsn_bed *b = op->bed;
  const int S = op->slices;
  const int vmax = 32 / S;
  if (nvec <= 0) return;
  const double *xsrc = scatter_rows_if_needed(op, d_X, &ldx, nvec);
  const int64_t npad = n_padded(b);
  VecMeta *meta = meta_buffer(op);
  for (int v0 = 0; v0 < nvec; v0 += vmax) {
    int nv = nvec - v0 < vmax ? nvec - v0 : vmax;
    int NB = pick_nb(nv * S), ncol = 16 * NB;
    int8_t *q = op->d_q.ensure((size_t)npad * kMaxCols * 2);
    int32_t *acc = op->d_acc.ensure((size_t)2 * op->m * kMaxCols);
    quantise(op, xsrc + (int64_t)v0 * ldx, ldx, b->n, npad, nv, 0, S, ncol, 1, 0, meta, q);
    launch_cprod<2, true, false>(op, NB, q, acc, kLutRaw, kLutNA, 0);
    op->passes++;
    hipLaunchKernelGGL(k_cprod_raw_final, dim3((unsigned)((op->m + 255) / 256), nv), dim3(256), 0,
                       b->stream, acc, op->m, ncol, S, meta, d_P + (int64_t)v0 * ld,
                       d_Q + (int64_t)v0 * ld, ld);
    BSN_HIP(hipGetLastError());
  }
}

void op_prod(bsn_op *op, const double *d_X, int64_t ldx, int nvec, double *d_Y, int64_t ldy) {
  prod_planes(op, d_X, nullptr, ldx, nvec, d_Y, ldy, 1, kLutRaw, kLutNA, 1, 0.0, op->slices);
}

void op_prod_acc(bsn_op *op, const double *d_X, int64_t ldx, int nvec, double *d_Y, int64_t ldy, double beta) {
  prod_planes(op, d_X, nullptr, ldx, nvec, d_Y, ldy, 1, kLutRaw, kLutNA, 1, beta, op->slices);
}

bool op_prod_segments(bsn_op *op, const double *d_X, int64_t ldx, int nvec, int pieces, int stride, int nseg,
                      const ProdSegment *segs, const std::function<void(int)> &after) {
  if (!op->rows_identity || op->prof_kind_override == 3) return false;
  ProdSegments sg{pieces, stride, nseg, segs, &after};
  prod_planes(op, d_X, nullptr, ldx, nvec, nullptr, 0, 1, kLutRaw, kLutNA, 1, 0.0, op->slices, &sg);
  return sg.done;
}

// rowSumsSq[i] = sum_j A~[i, j]^2 over the non-missing genotypes (src/bed-fun.cpp:121-123):
//   ((g - c) / s)^2 = g^2 a + g b + d,  a = 1/s^2, b = -2c/s^2, d = c^2/s^2
// = X2 . a + X . b + M . d with the planes X2 = g^2, X = g, M = non-missing: two passes.
__global__ void k_rowsq_weights(const double *center, const double *scale, int64_t m, double *a,
                                double *b, double *d) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const double c = center[j], s = scale[j];
  a[j] = 1.0 / (s * s);
  b[j] = -2.0 * c / (s * s);
  d[j] = c * c / (s * s);
}

void op_row_sums_sq(bsn_op *op, double *d_out) {
  require_bits(op->bed, 2, "prod_and_rowSumsSq");
  bsn_bed *bed = op->bed;
  DevBuf<double> w;
  double *a = w.ensure((size_t)3 * op->m), *b2 = a + op->m, *d = b2 + op->m;
  hipLaunchKernelGGL(k_rowsq_weights, dim3((unsigned)((op->m + 255) / 256)), dim3(256), 0, bed->stream,
                     op->d_center.p, op->d_scale.p, op->m, a, b2, d);
  BSN_HIP(hipGetLastError());
  constexpr uint32_t kLutX2 = 0x00040100u;  // code 0,1,2,3 -> 0, 1, 4, 0
  constexpr uint32_t kLutM = 0x00010101u;   //               -> 1, 1, 1, 0
  prod_planes(op, a, b2, op->m, 1, d_out, op->n, 2, kLutX2, kLutG0, 0, 0.0, 7);
  prod_planes(op, d, nullptr, op->m, 1, d_out, op->n, 2, kLutM, 0u, 0, 1.0, 7);
  BSN_HIP(hipStreamSynchronize(bed->stream));  // `w` is released on return
}

// per-sample counts of the codes over the selected variants (bed_row_counts_cpp,
// src/bed-fun.cpp:72-99): three single-plane passes against a vector of ones — exact, the
// fixed-point image of 1.0 is a power of two and the plane sums are integers < 2^31.
// d_out: 3 x n doubles (n2, n1, nNA per selected row).
void op_row_counts(bsn_op *op, double *d_out) {
  require_bits(op->bed, 2, "bed_counts(byrow = TRUE)");
  bsn_bed *bed = op->bed;
  std::vector<double> ones((size_t)op->m, 1.0);
  DevBuf<double> w;
  copy_h2d(bed, w.ensure((size_t)op->m), ones.data(), (size_t)op->m * 8);
  prod_planes(op, w.p, nullptr, op->m, 1, d_out, op->n, 2, kLutHom2, 0u, 0, 0.0, 7);
  prod_planes(op, w.p, nullptr, op->m, 1, d_out + op->n, op->n, 2, kLutHet, 0u, 0, 0.0, 7);
  prod_planes(op, w.p, nullptr, op->m, 1, d_out + 2 * op->n, op->n, 2, kLutNA, 0u, 0, 0.0, 7);
  BSN_HIP(hipStreamSynchronize(bed->stream));  // `w` and `ones` are released on return
}

// counts of codes weighted by integer row multiplicities (general ind_row):
// three planes (hom2, het, na) against the multiplicity vector, exact.
__global__ void k_counts_final(const int32_t *acc, int64_t m, int ncol, int S, int64_t n_sub,
                               int32_t *counts) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  long long n2 = (long long)horner(acc + j * ncol, S);
  long long n1 = (long long)horner(acc + (m + j) * ncol, S);
  long long na = (long long)horner(acc + (2 * m + j) * ncol, S);
  counts[4 * j + 0] = (int32_t)(n_sub - n1 - n2 - na);
  counts[4 * j + 1] = (int32_t)n1;
  counts[4 * j + 2] = (int32_t)n2;
  counts[4 * j + 3] = (int32_t)na;
}

void counts_weighted(bsn_op *op, const double *d_w, int64_t n_sub, int32_t *d_counts) {
  require_bits(op->bed, 2, "bed_counts");
  op->preq_X = nullptr;
  bsn_bed *b = op->bed;
  const int S = 4;
  const int64_t npad = n_padded(b);
  VecMeta *meta = meta_buffer(op);
  int8_t *q = op->d_q.ensure((size_t)npad * 64);
  int32_t *acc = op->d_acc.ensure((size_t)3 * op->m * 16);
  quantise(op, d_w, b->n, b->n, npad, 1, 0, S, 16, 1, 1, meta, q);
  launch_cprod<3, false, false>(op, 1, q, acc, kLutHom2, kLutHet, kLutNA);
  hipLaunchKernelGGL(k_counts_final, dim3((unsigned)((op->m + 255) / 256)), dim3(256), 0, b->stream,
                     acc, op->m, 16, S, n_sub, d_counts);
  BSN_HIP(hipGetLastError());
}

// ---- counts of the codes per GROUP of rows (bsn_bed_group_counts) ----------------------------------------
// The counting pass above fills one of the 16 digit columns of a column block; here every column carries a group: the
// n_file x G panel of row multiplicities (how often file row k was selected under group g) takes the place of the one
// multiplicity vector, one int8 digit per group while no multiplicity exceeds 127 (16 groups per column block, 32 per
// two-block launch), the four digits of counts_weighted otherwise (4 and 8).
//
// mult[v * n_file + rows[i]] += 1 for every selected row i whose group is g0 + v, v < gb.  Integer atomics: exact and
// order-independent.  (rows == NULL: row i itself)
__global__ void k_group_scatter(const int32_t *__restrict__ rows, const int32_t *__restrict__ group, int64_t n, int g0, int gb,
                                int64_t n_file, int32_t *mult) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int v = group[i] - g0;
  if (v < 0 || v >= gb) return;
  const int64_t k = rows ? (int64_t)rows[i] : i;
  if (k < 0 || k >= n_file) return;   // (the host has checked the list; a store outside the panel must not happen)
  atomicAdd(&mult[(int64_t)v * n_file + k], 1);
}

// The digit panel of `gb` groups in the layout k_cprod reads (k_quant, PERM = 1, one plane): the 16 samples of block kb
// under digit column col = v * S + s are the 16 bytes at q[(kb * ncol + col) * 16], sample e at byte (e % 4) * 4 + e / 4.
// Signed base-256 digits, as k_quant cuts them.  One thread per (16-block, group); samples at or past n_file are zero.
template <int S>
__global__ __launch_bounds__(256) void k_group_digits(const int32_t *__restrict__ mult, int64_t n_file, int64_t nblk, int gb,
                                                      int ncol, int8_t *__restrict__ q) {
  const int64_t kb = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int v = blockIdx.y;
  if (kb >= nblk || v >= gb) return;
  uint32_t pk[S][4];
#pragma unroll
  for (int s = 0; s < S; s++)
#pragma unroll
    for (int w = 0; w < 4; w++) pk[s][w] = 0;
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int64_t k = kb * 16 + e;
    long long A = k < n_file ? (long long)mult[(int64_t)v * n_file + k] : 0;
    const int pos = (e & 3) * 4 + (e >> 2);
#pragma unroll
    for (int s = 0; s < S; s++) {
      const int8_t da = (int8_t)(A & 0xFF);
      A = (A - da) >> 8;
      pk[s][pos >> 2] |= (uint32_t)(uint8_t)da << (8 * (pos & 3));
    }
  }
#pragma unroll
  for (int s = 0; s < S; s++)
    *(uint4 *)(q + ((kb * ncol) + v * S + s) * 16) = uint4{pk[s][0], pk[s][1], pk[s][2], pk[s][3]};
}

// table[4 * (G * j + g0 + v) + c] from the three plane sums of group column v (Horner over its digits, as in
// k_counts_final); code 0 is the group's size less the other three.  One thread per (variant, group of the launch).
__global__ void k_group_counts_final(const int32_t *acc, int64_t m, int ncol, int S, int g0, int gb, int G,
                                     const int32_t *__restrict__ gsize, int32_t *table) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m * gb) return;
  const int64_t j = idx / gb;
  const int v = (int)(idx - j * gb);
  const long long n2 = (long long)horner(acc + j * ncol + v * S, S);
  const long long n1 = (long long)horner(acc + (m + j) * ncol + v * S, S);
  const long long na = (long long)horner(acc + (2 * m + j) * ncol + v * S, S);
  *(int4 *)(table + 4 * ((int64_t)G * j + g0 + v)) =
      int4{(int32_t)((long long)gsize[g0 + v] - n1 - n2 - na), (int32_t)n1, (int32_t)n2, (int32_t)na};
}

void counts_grouped(bsn_op *op, const int32_t *d_rows, const int32_t *d_group, int64_t n, int32_t G, const int32_t *d_gsize,
                    bool one_digit, int32_t *d_table, double ms_out[3]) {
  require_bits(op->bed, 2, "bed_counts_by_group");
  op->preq_X = nullptr;
  bsn_bed *b = op->bed;
  hipStream_t st = b->stream;
  const int S = one_digit ? 1 : 4, per_block = 16 / S;
  const int64_t npad = n_padded(b), nblk = npad / 16;
  const int gmax = G < 2 * per_block ? G : 2 * per_block;   // groups of the largest launch
  DevBuf<int32_t> mult;
  mult.ensure((size_t)b->n * gmax);
  int8_t *q = op->d_q.ensure((size_t)npad * 32);
  int32_t *acc = op->d_acc.ensure((size_t)3 * op->m * 32);
  std::unique_ptr<EventMarks<4>> ev(ms_out ? new EventMarks<4>() : nullptr);   // (no events unless the times are asked for)
  for (int g0 = 0; g0 < G;) {
    const int left = G - g0;
    const int NB = left > per_block ? 2 : 1;   // two column blocks where they save a launch
    const int gb = left < NB * per_block ? left : NB * per_block, ncol = 16 * NB;
    if (ev) ev->mark(0, st);
    BSN_HIP(hipMemsetAsync(mult.p, 0, (size_t)b->n * gb * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_group_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_rows, d_group, n, g0, gb,
                       b->n, mult.p);
    const dim3 qgrid((unsigned)((nblk + 255) / 256), (unsigned)gb);
    if (S == 1) hipLaunchKernelGGL(k_group_digits<1>, qgrid, dim3(256), 0, st, mult.p, b->n, nblk, gb, ncol, q);
    else hipLaunchKernelGGL(k_group_digits<4>, qgrid, dim3(256), 0, st, mult.p, b->n, nblk, gb, ncol, q);
    BSN_HIP(hipGetLastError());
    if (ev) ev->mark(1, st);
    launch_cprod<3, false, false>(op, NB, q, acc, kLutHom2, kLutHet, kLutNA);
    if (ev) ev->mark(2, st);
    hipLaunchKernelGGL(k_group_counts_final, dim3((unsigned)((op->m * gb + 255) / 256)), dim3(256), 0, st, acc, op->m, ncol,
                       S, g0, gb, G, d_gsize, d_table);
    BSN_HIP(hipGetLastError());
    if (ev) {
      ev->mark(3, st);
      BSN_HIP(hipEventSynchronize(ev->e[3]));
      for (int k = 0; k < 3; k++) ms_out[k] += ev->ms(k, k + 1);
    }
    g0 += gb;
  }
  BSN_HIP(hipStreamSynchronize(st));   // `mult` is released on return
}

// ---------------------------------------------------------------------------
// Instruction-level self test: v_perm_b32 source order and i8 MFMA layouts.
__global__ void k_selftest(int *out) {
  int lane = threadIdx.x;
  // perm8: selector 0..3 must pick from `lo`, 4..7 from `hi`
  uint32_t r = perm8(0x77665544u, 0x33221100u, 0x07040300u);
  int ok_perm = (r == 0x77443300u);
  // mfma: A[row=l&15][k], B[k][col=l&15], k-slots paired by (lane>>4, byte)
  // A[i][k] = (i + 1) if k == 5*i+3 (mod 64) else 0 ; B[k][j] = (k % 7) - 3 + j
  v4i a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
  int i = lane & 15, gq = lane >> 4;
  for (int e = 0; e < 16; e++) {
    int k = gq * 16 + e;
    int av = (k == (5 * i + 3) % 64) ? (i + 1) : 0;
    int bv = (k % 7) - 3 + i;  // column index of B is also lane&15
    a[e >> 2] |= (av & 0xFF) << (8 * (e & 3));
    b[e >> 2] |= (bv & 0xFF) << (8 * (e & 3));
  }
  v4i c = {0, 0, 0, 0};
  c = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
  int ok_mfma = 1;
  for (int rr = 0; rr < 4; rr++) {
    int row = 4 * gq + rr, col = lane & 15;
    int k = (5 * row + 3) % 64;
    int want = (row + 1) * ((k % 7) - 3 + col);
    if (c[rr] != want) ok_mfma = 0;
  }
  int all_perm = __all(ok_perm), all_mfma = __all(ok_mfma);
  if (lane == 0) {
    out[0] = all_perm;
    out[1] = all_mfma;
    out[2] = (int)r;
  }
}

void selftest() {
  DevBuf<int> d;
  d.ensure(4);
  hipLaunchKernelGGL(k_selftest, dim3(1), dim3(64), 0, 0, d.p);
  BSN_HIP(hipGetLastError());
  int h[4] = {0, 0, 0, 0};
  BSN_HIP(hipMemcpy(h, d.p, sizeof(h), hipMemcpyDeviceToHost));
  if (!h[0]) fail("selftest: v_perm_b32 byte order differs from the assumed {hi:lo} (got %08x)", h[2]);
  if (!h[1]) fail("selftest: v_mfma_i32_16x16x64_i8 operand/accumulator layout differs");
}

}  // namespace bsn
