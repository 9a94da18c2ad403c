// gwas.hip — big_univLinReg and big_univLogReg (bigstatsr): one regression per variant, y ~ x + 1 + covar.
//
// Linear scan (bsn_univ_linreg): with U an orthonormal basis of [1, covar] and y~ = y - U U' y, everything a variant
// needs is x' y~, U' x and x' x: one crossproduct pass over the panel [y~, U] (op_cprod_raw at 56 bits; op_cprod on a
// byte image) plus the exact code counts (the integer sums of stats8 on a byte image), then k_ulr_final.
//
// Logistic scan (bsn_univ_logreg): k_logreg, DESIGN.md 3.5f.  One wave owns one variant and iterates in the kernel;
// a lane takes one sample of a 64-sample step (decode, eta, w, w z: irls_step.hpp), and the weighted Gram matrix
// [C | z]' W [C | z] accumulates in v_mfma_f64_16x16x4_f64 tiles with A = the rows of C and B = w times them (w z in
// the extra column), so that no square root and no division by a weight is needed.  The four waves of a workgroup
// share each tile of covariate rows through LDS; the variant's wave solves its system out of LDS by irls_step.hpp's
// packed Cholesky.  The null model is the same kernel without the variant column.
#include <cmath>
#include <cstring>
#include <limits>

#include "bsn_internal.hpp"
#include "irls_step.hpp"

namespace bsn {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kWaves = 4;                       // variants per workgroup
constexpr int kThreads = 64 * kWaves;
// per wave in LDS: the packed Gram matrix (33 * 34 / 2 = 561 doubles), beta (32), the solve's work space (64) and the
// step's x, w, w z (3 * 64)
constexpr int kGramDoubles = 576;
constexpr int kWaveDoubles = kGramDoubles + 32 + 64 + 3 * 64;

struct LogregArgs {
  const uint8_t *img;
  int64_t pitch;
  int bits;
  double v_off, v_step;
  const int32_t *rows, *cols;   // gather lists (NULL: file order / col0 + j)
  int64_t col0, n, m;
  const double *covar, *y;      // n x q column-major, n
  int q, has_x;
  const double *beta0;          // with the variant: the covariates-only fit (q + 1), where every fit starts
  double tol;
  int maxiter, ts;              // ts: samples per LDS tile (a multiple of 64)
  double *estim, *se, *beta_out;
  int32_t *niter;
};

// (no contraction: v_off + v_step k must round like the host's decode table does, 1.0 - 0.01 * 100 = 0 exactly)
#pragma clang fp contract(off)
__device__ __forceinline__ double decode(const uint8_t *colp, int bits, int64_t r, double v_off, double v_step, bool &na) {
  if (bits == 2) {
    const uint32_t c = (colp[r >> 2] >> (2 * (int)(r & 3))) & 3u;
    na |= c == 3u;
    return c == 3u ? 0.0 : (double)c;
  }
  const int k = (int8_t)colp[r];
  na |= k == -128;
  return k == -128 ? 0.0 : v_off + v_step * (double)k;
}
#pragma clang fp contract(on)

// NT = number of 16-column operand tiles of [C | z]: 1 (P + 1 <= 16), 2 (<= 32), 3 (P = 32: z alone in the third)
template <int NT>
__global__ __launch_bounds__(kThreads) void k_logreg(LogregArgs a) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q1 = a.q + 1, rowlen = a.q + 2, xoff = a.has_x ? 1 : 0, P = q1 + xoff;
  double *tile = lds;                            // ts rows of (1, covar_1 .. covar_q, y); rows past n are zero
  double *wv = lds + (size_t)a.ts * rowlen + (size_t)wave * kWaveDoubles;
  double *G = wv, *beta = G + kGramDoubles, *work = beta + 32, *sx = work + 64, *sw = sx + 64, *swz = sw + 64;
  int *status = (int *)(lds + (size_t)a.ts * rowlen + (size_t)kWaves * kWaveDoubles);

  const int64_t j = (int64_t)blockIdx.x * kWaves + wave;
  bool active = a.has_x ? j < a.m : wave == 0;
  const uint8_t *colp = nullptr;
  if (active && a.has_x) colp = a.img + (a.cols ? (int64_t)a.cols[j] : a.col0 + j) * a.pitch;
  if (lane < P) beta[lane] = a.has_x ? (lane == 0 ? 0.0 : a.beta0[lane - 1]) : 0.0;
  if (lane == 0) status[wave] = active ? 1 : 0;

  // what this lane feeds into operand tile T: column g = 16 T + (lane & 15) of [C | z]
  int kind[NT], tcol[NT];                        // 0: nothing, 1: the variant, 2: column tcol of the LDS tile, 3: z
  for (int T = 0; T < NT; T++) {
    const int g = 16 * T + (lane & 15);
    kind[T] = (g == 0 && a.has_x) ? 1 : g < P ? 2 : g == P ? 3 : 0;
    tcol[T] = kind[T] == 2 ? g - xoff : 0;
  }

  const int ts_shift = a.ts == 256 ? 8 : 7;
  bool has_na = false, varies = false;
  double xref = 0.0;
  if (active && a.has_x) {
    bool na0 = false;
    xref = decode(colp, a.bits, a.rows ? (int64_t)a.rows[0] : 0, a.v_off, a.v_step, na0);
  }

  for (int it = 1;; it++) {
    constexpr int NACC = NT == 1 ? 1 : NT == 2 ? 3 : 5;
    f64x4 acc[NACC];
    for (int t = 0; t < NACC; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};

    for (int64_t t0 = 0; t0 < a.n; t0 += a.ts) {
      __syncthreads();                           // the previous tile is consumed (first turn: beta is in place)
      for (int idx = threadIdx.x; idx < a.ts * rowlen; idx += kThreads) {
        const int c = idx >> ts_shift, r = idx & (a.ts - 1);
        const int64_t i = t0 + r;
        double v = 0.0;
        if (i < a.n) v = c == 0 ? 1.0 : c <= a.q ? a.covar[i + (int64_t)(c - 1) * a.n] : a.y[i];
        tile[r * rowlen + c] = v;
      }
      __syncthreads();
      if (!active) continue;
      const int64_t left = a.n - t0;
      const int rows_here = left < a.ts ? (int)left : a.ts;
      for (int s0 = 0; s0 < rows_here; s0 += 64) {
        const int r = s0 + lane;
        const int64_t i = t0 + r;
        double x = 0.0, w = 0.0, wz = 0.0;       // a sample at or beyond n carries weight exactly 0
        if (i < a.n) {
          if (a.has_x) {
            x = decode(colp, a.bits, a.rows ? (int64_t)a.rows[i] : i, a.v_off, a.v_step, has_na);
            varies |= x != xref;
          }
          const double *row = tile + r * rowlen;
          irls::sample_map(irls::eta_of(beta, a.has_x, x, row, q1), row[q1], w, wz);
        }
        sx[lane] = x;
        sw[lane] = w;
        swz[lane] = wz;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 4
        for (int t = 0; t < 16; t++) {           // four samples per MFMA: sample 4 t + (lane >> 4) of the step
          const int sl = 4 * t + (lane >> 4);
          const double xs = sx[sl], ws = sw[sl], wzs = swz[sl];
          const double *srow = tile + (s0 + sl) * rowlen;
          double av[NT], bv[NT];
#pragma unroll
          for (int T = 0; T < NT; T++) {
            av[T] = kind[T] == 1 ? xs : kind[T] == 2 ? srow[tcol[T]] : 0.0;
            bv[T] = kind[T] == 3 ? wzs : ws * av[T];
          }
          acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0], bv[0], acc[0], 0, 0, 0);
          if constexpr (NT >= 2) {
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0], bv[1], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1], bv[1], acc[2], 0, 0, 0);
          }
          if constexpr (NT == 3) {
            acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0], bv[2], acc[3], 0, 0, 0);
            acc[4] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1], bv[2], acc[4], 0, 0, 0);
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();         // the step's x, w, w z are read before the next step overwrites them
      }
    }

    // accumulator tiles -> the packed upper triangle; D has its column on lane & 15 and row (lane >> 4) + 4 reg
    if (active) {
#pragma unroll
      for (int t = 0; t < NACC; t++) {
        const int Ti = (t == 2 || t == 4) ? 1 : 0, Tj = t == 0 ? 0 : t <= 2 ? 1 : 2;
        const int gc = 16 * Tj + (lane & 15);
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
          const int gr = 16 * Ti + (lane >> 4) + 4 * reg;
          if (gr <= gc && gc <= P) G[irls::packed(gr, gc)] = acc[t][reg];
        }
      }
    }
    const bool bad = a.has_x && it == 1 && (__any(has_na) || !__any(varies));
    __syncthreads();
    if (active && lane == 0) {
      double inv00 = 0.0;
      const int st = bad ? -1 : irls::solve_step(G, P, beta, a.tol, &inv00, work);
      const bool stop = st != 0 || it >= a.maxiter;
      if (stop) {
        const int64_t o = a.has_x ? j : 0;
        if (a.estim) a.estim[o] = st < 0 ? irls::qnan() : beta[0];
        if (a.se) a.se[o] = st < 0 ? irls::qnan() : sqrt(inv00);
        a.niter[o] = st < 0 ? 0 : st == 1 ? it : -1;
        if (a.beta_out)
          for (int k = 0; k < P; k++) a.beta_out[k] = beta[k];
        status[wave] = 0;
      }
    }
    __syncthreads();
    active = status[wave] != 0;
    int any = 0;
    for (int w2 = 0; w2 < kWaves; w2++) any |= status[w2];
    if (!any) break;
  }
}

void launch_logreg(hipStream_t st, LogregArgs a) {
  const int P = a.q + 1 + (a.has_x ? 1 : 0), NT = (P + 1 + 15) / 16;
  a.ts = a.q + 2 <= 16 ? 256 : 128;             // 32 KB of covariate rows either way
  const size_t lds = ((size_t)a.ts * (a.q + 2) + (size_t)kWaves * kWaveDoubles) * 8 + 16;
  const dim3 grid((unsigned)(a.has_x ? (a.m + kWaves - 1) / kWaves : 1));
  if (NT == 1)
    hipLaunchKernelGGL(k_logreg<1>, grid, dim3(kThreads), lds, st, a);
  else if (NT == 2)
    hipLaunchKernelGGL(k_logreg<2>, grid, dim3(kThreads), lds, st, a);
  else
    hipLaunchKernelGGL(k_logreg<3>, grid, dim3(kThreads), lds, st, a);
  BSN_HIP(hipGetLastError());
}

// estim, std_err per variant from num = x' y~, t_k = u_k' x (columns 1 .. K of Z) and x' x.  counts: 4 x m code counts of a
// 2-bit image; st8: (S1, S2, nNA) x m of a byte image with v = v_off + v_step k.
#pragma clang fp contract(off)
__global__ void k_ulr_final(const double *Z, int64_t ld, int K, const int32_t *counts, const long long *st8, double v_off,
                            double v_step, int64_t n, int64_t m, double yy, double df, double *estim, double *se) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  double xx;
  bool bad;
  if (counts) {
    const int4 c = *(const int4 *)(counts + 4 * j);
    xx = (double)c.y + 4.0 * c.z;
    bad = c.w > 0 || c.x == n || c.y == n || c.z == n;
  } else {
    const double s1 = (double)st8[3 * j], s2 = (double)st8[3 * j + 1];
    xx = (double)n * v_off * v_off + 2.0 * v_off * v_step * s1 + v_step * v_step * s2;
    // no variance: n S2 = S1^2 exactly (Cauchy-Schwarz with equality only for a constant column)
    bad = st8[3 * j + 2] > 0 || (__int128)n * st8[3 * j + 1] == (__int128)st8[3 * j] * st8[3 * j];
  }
  double proj = 0.0;
  for (int k = 1; k <= K; k++) {
    const double t = Z[j + (int64_t)k * ld];
    proj = proj + t * t;
  }
  const double num = Z[j], den = xx - proj;
  if (bad || !(den > irls::kPivotTol * xx)) {
    estim[j] = se[j] = irls::qnan();
    return;
  }
  const double est = num / den;
  estim[j] = est;
  se[j] = sqrt((yy - est * num) / (den * df));
}
#pragma clang fp contract(on)

void check_common(bsn_bed *bed, const char *what) {
  if (!bed) fail("%s: no handle", what);
  refuse_generic(bed, what);
  require_resident(bed, what);
}

}  // namespace
}  // namespace bsn

using namespace bsn;

extern "C" {

int bsn_univ_linreg(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const double *y,
                    const double *U, int64_t K, double *estim, double *std_err) {
  return guarded([&] {
    const char *what = "big_univLinReg";
    check_common(bed, what);
    if (K < 0 || K > irls::kMaxP - 1) fail("%s: 'covar.train' has more than 30 columns.", what);
    if (n - K - 1 <= 0) fail("%s: no degrees of freedom left (n = %lld, K = %lld).", what, (long long)n, (long long)K);
    if (m <= 0 || n <= 0) fail("'ind.row' and 'ind.col' can't be empty.");
    // the panel [y~, U], y~ = y - U U' y
    const int nvec = (int)K + 1;
    std::vector<double> X((size_t)n * nvec), c((size_t)K, 0.0);
    for (int64_t k = 0; k < K; k++)
      for (int64_t i = 0; i < n; i++) c[(size_t)k] += U[i + k * n] * y[i];
    double yy = 0.0;
    for (int64_t i = 0; i < n; i++) {
      double r = y[i];
      for (int64_t k = 0; k < K; k++) r -= U[i + k * n] * c[(size_t)k];
      X[(size_t)i] = r;
      yy += r * r;
    }
    if (K) std::memcpy(X.data() + n, U, (size_t)n * K * 8);
    bsn_op op;
    fill_op(&op, bed, ind_row, n, ind_col, m, nullptr, nullptr);
    op.slices = 7;
    DevBuf<double> d_X, d_Z, d_Q, d_out;
    DevBuf<int32_t> d_counts;
    DevBuf<long long> d_st;
    copy_h2d(bed, d_X.ensure(X.size()), X.data(), X.size() * 8);
    d_Z.ensure((size_t)m * nvec);
    if (bed->bits == 2) {
      counts_device(&op, ind_row, n, d_counts.ensure((size_t)4 * m));
      op_cprod_raw(&op, d_X.p, n, nvec, d_Z.p, d_Q.ensure((size_t)m * nvec), m);
    } else {
      stats8(bed, op.rows(), n, op.cols(), op.col0, m, d_st.ensure((size_t)3 * m));
      op_cprod(&op, d_X.p, n, nvec, d_Z.p, m);
    }
    d_out.ensure((size_t)2 * m);
    hipLaunchKernelGGL(k_ulr_final, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, bed->stream, d_Z.p, m, (int)K,
                       d_counts.p, d_st.p, bed->v_off, bed->v_step, n, m, yy, (double)(n - K - 1), d_out.p, d_out.p + m);
    BSN_HIP(hipGetLastError());
    copy_d2h(bed, estim, d_out.p, (size_t)m * 8);
    copy_d2h(bed, std_err, d_out.p + m, (size_t)m * 8);
    BSN_HIP(hipStreamSynchronize(bed->stream));
  });
}

int bsn_univ_logreg(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const double *y01,
                    const double *covar, int64_t q, double tol, int32_t maxiter, double *estim, double *std_err,
                    int32_t *niter) {
  return guarded([&] {
    const char *what = "big_univLogReg";
    check_common(bed, what);
    if (q < 0 || q > irls::kMaxP - 2) fail("%s: 'covar.train' has more than 30 columns.", what);
    if (maxiter < 1) fail("%s: 'maxiter' must be at least 1.", what);
    if (m <= 0 || n <= 0) fail("'ind.row' and 'ind.col' can't be empty.");
    for (int64_t i = 0; i < n; i++)
      if (y01[i] != 0.0 && y01[i] != 1.0) fail("%s: 'y01.train' should be composed of 0s and 1s.", what);
    bsn_op op;
    fill_op(&op, bed, ind_row, n, ind_col, m, nullptr, nullptr);   // (for its row and column lists and their checks)
    DevBuf<double> d_y, d_cov, d_beta0, d_out;
    DevBuf<int32_t> d_niter;
    copy_h2d(bed, d_y.ensure((size_t)n), y01, (size_t)n * 8);
    if (q) copy_h2d(bed, d_cov.ensure((size_t)n * q), covar, (size_t)n * q * 8);
    d_beta0.ensure((size_t)q + 1);
    d_out.ensure((size_t)2 * m);
    d_niter.ensure((size_t)m + 1);
    LogregArgs a{};
    a.img = bed->d_img;
    a.pitch = bed->pitch;
    a.bits = bed->bits;
    a.v_off = bed->v_off;
    a.v_step = bed->v_step;
    a.rows = op.rows();
    a.cols = op.cols();
    a.col0 = op.col0;
    a.n = n;
    a.covar = d_cov.p;
    a.y = d_y.p;
    a.q = (int)q;
    // the null model: covariates only, from beta = 0
    LogregArgs a0 = a;
    a0.has_x = 0;
    a0.m = 1;
    a0.tol = irls::kNullTol;
    a0.maxiter = irls::kNullMaxIter;
    a0.beta_out = d_beta0.p;
    a0.niter = d_niter.p + m;
    launch_logreg(bed->stream, a0);
    int32_t null_iter = 0;
    copy_d2h(bed, &null_iter, d_niter.p + m, 4);
    BSN_HIP(hipStreamSynchronize(bed->stream));
    if (null_iter == 0) fail("%s: the model without a variant is singular ('covar.train' has collinear columns).", what);
    a.has_x = 1;
    a.m = m;
    a.beta0 = d_beta0.p;
    a.tol = tol;
    a.maxiter = maxiter;
    a.estim = d_out.p;
    a.se = d_out.p + m;
    a.niter = d_niter.p;
    launch_logreg(bed->stream, a);
    copy_d2h(bed, estim, d_out.p, (size_t)m * 8);
    copy_d2h(bed, std_err, d_out.p + m, (size_t)m * 8);
    copy_d2h(bed, niter, d_niter.p, (size_t)m * 4);
    BSN_HIP(hipStreamSynchronize(bed->stream));
  });
}

}  // extern "C"
