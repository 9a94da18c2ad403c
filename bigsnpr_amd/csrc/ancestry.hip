// ancestry.hip — ancestry proportions from allele frequencies on the device (snp_ancestry_summary of
// R/ancestry-summary.R:31-74, for B frequency columns or for every selected sample of a resident genotype image):
// bsn_qp_simplex, bsn_ancestry_moments, bsn_ancestry_summary, bsn_bed_ancestry.  The rule (the quadratic program, the
// correlations, the row slabs) is stated in qp_step.hpp, shared with the CPU statement.  DESIGN.md 3.5s.
//
// k_anc_moments: the tall-skinny fp64 pass over P (M x L), X0 (M x K) and F (M x B): T = [P | X0 | 1]'[X0 | F] and the
// sums of squares of the right-hand columns.  Rows are cut into slabs (qp::kSlabRows rows, or BSN_ANC_SLABS slabs), one
// workgroup per slab; a workgroup stages tiles of kTileRows rows of every column in LDS (each input element is read once
// from HBM) and thread (ty, tx) of its 16 x 16 threads keeps the entries (ty + 16 i, tx + 16 j) of T in registers, adding
// row after row.  The per-slab partial sums go to a buffer and k_anc_moments_sum adds them in ascending slab order: no
// atomics, the same bits in every run.  One launch takes L + K + B' <= 128 columns and K + B' <= 64 right-hand columns;
// more frequency columns go in chunks of B' (P and X0 are then read once per chunk).
//
// k_anc_qp<W>: one group of W lanes of a wave per problem, W the smallest of 8, 16, 32, 64 that is >= K, the work space
// (qp::work_doubles(K) + K doubles) in LDS, 64 / W problems per workgroup of one wave — the launch arithmetic of k_oadp
// (project.hip).  Per problem: d = X'(l o correction), the program, w, cor_each, cor_pred, the step count.
#include <algorithm>
#include <cstring>

#include "bsn_internal.hpp"
#include "lane_group.hpp"
#include "qp_step.hpp"

namespace bsn {
namespace {

// device milliseconds of the last call of this process (bsn_ancestry_last_ms): genotype pass, moment pass, program kernel
double g_last_ms[3] = {0.0, 0.0, 0.0};

constexpr int kWave = kLaneGroupWave;
constexpr int kTileRows = 32;            // rows of one LDS tile
constexpr int kTilePitch = kTileRows + 1;
constexpr int kMaxCols = 128;            // columns of one launch: L + K + B'
constexpr int kMaxRight = 64;            // right-hand columns of one launch: K + B'
static_assert((size_t)kMaxCols * kTilePitch * 8 <= 65536, "the tile exceeds the default LDS limit");
static_assert(qp::kMaxL + qp::kMaxK < kMaxCols && qp::kMaxK < kMaxRight, "no room for a frequency column");

// the columns of one launch of k_anc_moments.  Left-hand rows of T: the L + K columns of P and X0, then the ones, then the
// row of the sums of squares (L + K + 2 in all); right-hand columns: X0 and the B' columns of F from b0 on.
struct MomentCols {
  const double *P, *X0, *F;
  int64_t ldp, ldx, ldf, M;
  int L, K, Bc;
};

template <int RA, int RB>
__global__ __launch_bounds__(256) void k_anc_moments(MomentCols c, int64_t slab_len, double *__restrict__ partial) {
  extern __shared__ double tile[];
  const int tid = (int)threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int nleft = c.L + c.K, ncol = nleft + c.Bc, nright = c.K + c.Bc, nrow = nleft + 2;
  const int64_t lo = (int64_t)blockIdx.x * slab_len, hi = min(c.M, lo + slab_len);
  double acc[RA][RB];
#pragma unroll
  for (int i = 0; i < RA; i++)
#pragma unroll
    for (int j = 0; j < RB; j++) acc[i][j] = 0.0;

  for (int64_t r0 = lo; r0 < hi; r0 += kTileRows) {
    const int nr = (int)min((int64_t)kTileRows, hi - r0);
    for (int idx = tid; idx < ncol * kTileRows; idx += 256) {
      const int col = idx / kTileRows, r = idx % kTileRows;
      if (r < nr) {
        const double *src = col < c.L ? c.P + (int64_t)col * c.ldp : col < nleft ? c.X0 + (int64_t)(col - c.L) * c.ldx : c.F + (int64_t)(col - nleft) * c.ldf;
        tile[col * kTilePitch + r] = src[r0 + r];
      }
    }
    __syncthreads();
    for (int r = 0; r < nr; r++) {
      double rb[RB];
#pragma unroll
      for (int j = 0; j < RB; j++) {
        const int b = tx + 16 * j;
        rb[j] = b < nright ? tile[(c.L + b) * kTilePitch + r] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < RA; i++) {
        const int a = ty + 16 * i;
        const double la = a < nleft ? tile[a * kTilePitch + r] : 1.0;
#pragma unroll
        for (int j = 0; j < RB; j++) acc[i][j] += (a == nleft + 1 ? rb[j] : la) * rb[j];
      }
    }
    __syncthreads();
  }
  double *out = partial + (size_t)blockIdx.x * nrow * nright;
#pragma unroll
  for (int i = 0; i < RA; i++)
#pragma unroll
    for (int j = 0; j < RB; j++) {
      const int a = ty + 16 * i, b = tx + 16 * j;
      if (a < nrow && b < nright) out[(size_t)b * nrow + a] = acc[i][j];
    }
}

// where the sums of one launch go: compact column-major results, frequency columns from b0 on
struct MomentOut {
  double *PtX0, *PtF, *G0, *X0tF, *csX0, *csF, *sqF;
  int64_t b0;
  int first;   // the launch that files the X0 columns
};

// entry (a, b) of T: the partial sums of the S slabs in ascending order
__global__ void k_anc_moments_sum(const double *__restrict__ partial, int64_t S, int L, int K, int Bc, MomentOut o) {
  const int nleft = L + K, nrow = nleft + 2, nright = K + Bc;
  const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e >= nrow * nright) return;
  const int a = e % nrow, b = e / nrow;
  double s = 0.0;
  for (int64_t t = 0; t < S; t++) s += partial[(size_t)t * nrow * nright + e];
  if (b < K) {
    if (!o.first) return;
    if (a < L) {
      if (o.PtX0) o.PtX0[a + (size_t)b * L] = s;
    } else if (a < nleft) {
      if (o.G0) o.G0[(a - L) + (size_t)b * K] = s;
    } else if (a == nleft) {
      if (o.csX0) o.csX0[b] = s;
    }
    return;
  }
  const int64_t bb = o.b0 + (b - K);
  if (a < L)
    o.PtF[a + (size_t)bb * L] = s;
  else if (a < nleft)
    o.X0tF[(a - L) + (size_t)bb * K] = s;
  else if (a == nleft)
    o.csF[bb] = s;
  else
    o.sqF[bb] = s;
}

void check_shape(int64_t M, int64_t L, int64_t K, int64_t B) {
  if (const char *why = qp::check_k(K)) fail("%s", why);
  if (L < 1) fail("snp_ancestry_summary: 'projection' must have at least one column.");
  if (L > qp::kMaxL) fail("snp_ancestry_summary: more than %d columns of 'projection' are not supported.", qp::kMaxL);
  if (M < 1) fail("snp_ancestry_summary: no variant");
  if (B < 0) fail("snp_ancestry_summary: negative number of frequency columns");
}

// The moment pass on device matrices, queued on `st`; the results (device pointers, compact; the F results may be NULL
// when B = 0, the X0 results may be NULL when not wanted) are complete when the stream has run.
void moments_device(const double *P, int64_t ldp, const double *X0, int64_t ldx, const double *F, int64_t ldf, int64_t M, int L, int K,
                    int64_t B, MomentOut out, DevBuf<double> &d_partial, hipStream_t st) {
  if (ldp < M || ldx < M || (B > 0 && ldf < M)) fail("snp_ancestry_summary: Incompatibility between dimensions (leading dimension).");
  const char *env = getenv("BSN_ANC_SLABS");
  const int64_t forced = env ? atoll(env) : 0;
  const int64_t len = qp::slab_len(M, forced), S = qp::slab_count(M, forced);
  if (S > 0x7fffffffLL) fail("snp_ancestry_summary: too many slabs for one launch.");
  const int bmax = std::min(kMaxRight - K, kMaxCols - L - K);
  int64_t b0 = 0;
  do {
    const int Bc = (int)std::min<int64_t>(B - b0, bmax);
    MomentCols c{P, X0, B > 0 ? F + b0 * ldf : nullptr, ldp, ldx, ldf, M, L, K, Bc};
    const int nrow = L + K + 2, nright = K + Bc;
    d_partial.ensure((size_t)S * nrow * nright);
    const size_t lds = (size_t)(L + K + Bc) * kTilePitch * 8;
    const dim3 grid((unsigned)S), block(256);
    const bool tall = nrow > 64, wide = nright > 32;
    if (tall && wide)
      hipLaunchKernelGGL((k_anc_moments<8, 4>), grid, block, lds, st, c, len, d_partial.p);
    else if (tall)
      hipLaunchKernelGGL((k_anc_moments<8, 2>), grid, block, lds, st, c, len, d_partial.p);
    else if (wide)
      hipLaunchKernelGGL((k_anc_moments<4, 4>), grid, block, lds, st, c, len, d_partial.p);
    else
      hipLaunchKernelGGL((k_anc_moments<4, 2>), grid, block, lds, st, c, len, d_partial.p);
    BSN_HIP(hipGetLastError());
    out.b0 = b0;
    out.first = b0 == 0;
    hipLaunchKernelGGL(k_anc_moments_sum, dim3((unsigned)((nrow * nright + 255) / 256)), dim3(256), 0, st, d_partial.p, S, L, K, Bc, out);
    BSN_HIP(hipGetLastError());
    b0 += Bc;
  } while (b0 < B);
}

// ---- the program kernel ----------------------------------------------------------------------------------------------
// Where problem b finds its numbers.  l (the projection P'f, L values) at l[j * l_ldj + b * l_ldb] (+ l_off[j]); X0'f (K)
// at xf[k * xf_ldk + b * xf_ldb] (+ xf_off[k]); sum f = fs[b] + fs_off; sum f^2 = fq[b] (+ 2 dc[b]) + fq_off.  The offsets
// serve bed_ancestry, whose product pass yields the moments of g / 2 - c.  dq != NULL (bsn_qp_simplex): d is read from
// dq[k + b * K], and no correlation is computed.
struct QpArgs {
  int K, L, sum_to_one;
  int64_t B;
  double M;
  const double *D, *J0, *X, *corr, *G0, *c0, *dq;
  const double *l, *l_off;
  int64_t l_ldj, l_ldb;
  const double *xf, *xf_off;
  int64_t xf_ldk, xf_ldb;
  const double *fs, *fq, *dc;
  double fs_off, fq_off;
  double *w, *cor_each, *cor_pred;
  int32_t *steps;
};

template <int W>
__global__ __launch_bounds__(kWave) void k_anc_qp(QpArgs a) {
  extern __shared__ double qp_lds[];
  const int grp = (int)threadIdx.x / W, K = a.K;
  const int64_t b = (int64_t)blockIdx.x * (kWave / W) + grp;
  if (b >= a.B) return;   // the whole group leaves: nothing below waits for it
  const LaneGroup<W> g{(int)threadIdx.x % W};
  double *ws = qp_lds + (size_t)grp * (qp::work_doubles(K) + K), *d = ws + qp::work_doubles(K);
  for (int k = g.lane; k < K; k += W) {
    double acc = 0.0;
    if (a.dq) {
      acc = a.dq[k + b * K];
    } else {
      for (int j = 0; j < a.L; j++) {
        const double lj = a.l[j * a.l_ldj + b * a.l_ldb] + (a.l_off ? a.l_off[j] : 0.0);
        acc += a.X[(size_t)k * a.L + j] * (lj * a.corr[j]);
      }
    }
    d[k] = acc;
  }
  g.sync();
  const int steps = qp::solve_one(g, K, a.D, a.J0, d, 1, a.sum_to_one != 0, ws, a.w + b, a.B);
  if (g.lane == 0) a.steps[b] = steps;
  if (a.dq) return;
  // X0'f into d (lane k its own entry), then the correlations
  for (int k = g.lane; k < K; k += W) d[k] = a.xf[k * a.xf_ldk + b * a.xf_ldb] + (a.xf_off ? a.xf_off[k] : 0.0);
  g.sync();
  const double sf = a.fs[b] + a.fs_off, sff = a.fq[b] + (a.dc ? 2.0 * a.dc[b] : 0.0) + a.fq_off;
  const double cp = qp::cor_one(g, K, a.M, a.G0, a.c0, d, 1, sf, sff, ws, a.cor_each + b, a.B);
  if (g.lane == 0) a.cor_pred[b] = cp;
}

int group_width(int K) { return K <= 8 ? 8 : K <= 16 ? 16 : K <= 32 ? 32 : 64; }

// queues the launch on `st`
void qp_launch(const QpArgs &a, hipStream_t st) {
  const int W = group_width(a.K);
  const int per_wg = kWave / W;
  const int64_t blocks = (a.B + per_wg - 1) / per_wg;
  if (blocks > 0x7fffffffLL) fail("snp_ancestry_summary: too many problems for one launch.");
  if (blocks < 1) return;
  const size_t lds = (size_t)per_wg * (qp::work_doubles(a.K) + a.K) * 8;
  const dim3 grid((unsigned)blocks), block(kWave);
  switch (W) {
    case 8: hipLaunchKernelGGL(k_anc_qp<8>, grid, block, lds, st, a); break;
    case 16: hipLaunchKernelGGL(k_anc_qp<16>, grid, block, lds, st, a); break;
    case 32: hipLaunchKernelGGL(k_anc_qp<32>, grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL(k_anc_qp<64>, grid, block, lds, st, a); break;
  }
  BSN_HIP(hipGetLastError());
}

// D checked and factored on the host: [D | J0], as the kernel takes it.  Before any device work.
std::vector<double> factor_checked(int64_t K, const double *D, const char *who) {
  if (const char *why = qp::check_k(K)) fail("%s", why);
  if (!D) fail("%s: no matrix", who);
  std::vector<double> h((size_t)2 * K * K, 0.0);
  std::memcpy(h.data(), D, (size_t)K * K * 8);
  if (!qp::factor((int)K, D, h.data() + (size_t)K * K))
    fail("%s: 'Dmat' is not positive definite (its Cholesky factorisation fails).", who);
  return h;
}

void upload(const std::vector<double> &h, DevBuf<double> &d) {
  BSN_HIP(hipMemcpy(d.ensure(h.size()), h.data(), h.size() * 8, hipMemcpyHostToDevice));
}

void qp_host(const double *D, int64_t K, const double *dvec, int64_t B, int sum_to_one, double *w_out, int32_t *steps_out,
             int64_t *n_failed) {
  if (const char *why = qp::check_k(K)) fail("%s", why);
  if (B < 0) fail("qp_simplex: negative number of problems");
  if (!n_failed) fail("qp_simplex: no buffer");
  *n_failed = 0;
  if (B > 0 && (!dvec || !w_out || !steps_out)) fail("qp_simplex: no buffer");
  const std::vector<double> DJ = factor_checked(K, D, "qp_simplex");
  require_gpu();
  g_last_ms[0] = g_last_ms[1] = g_last_ms[2] = 0.0;
  if (B == 0) return;
  DevBuf<double> d_DJ, d_d, d_w;
  DevBuf<int32_t> d_steps;
  upload(DJ, d_DJ);
  BSN_HIP(hipMemcpy(d_d.ensure((size_t)K * B), dvec, (size_t)K * B * 8, hipMemcpyHostToDevice));
  d_w.ensure((size_t)K * B);
  d_steps.ensure((size_t)B);
  QpArgs a{};
  a.K = (int)K, a.sum_to_one = sum_to_one, a.B = B;
  a.D = d_DJ.p, a.J0 = d_DJ.p + K * K, a.dq = d_d.p, a.w = d_w.p, a.steps = d_steps.p;
  EventMarks<2> ev;
  ev.mark(0, nullptr);
  qp_launch(a, nullptr);
  ev.mark(1, nullptr);
  BSN_HIP(hipStreamSynchronize(nullptr));
  BSN_HIP(hipMemcpy(w_out, d_w.p, (size_t)K * B * 8, hipMemcpyDeviceToHost));
  BSN_HIP(hipMemcpy(steps_out, d_steps.p, (size_t)B * 4, hipMemcpyDeviceToHost));
  g_last_ms[2] = ev.ms(0, 1);
  for (int64_t b = 0; b < B; b++) *n_failed += steps_out[b] == qp::kNotSolved;
}

// a host matrix of `rows` rows and `cols` columns (leading dimension ld) compact on the device; or the device matrix itself
const double *on_device(const double *src, int64_t ld, int64_t rows, int64_t cols, bool is_device, DevBuf<double> &buf, int64_t *ld_out) {
  *ld_out = ld;
  if (is_device || cols == 0) return src;
  buf.ensure((size_t)rows * cols);
  BSN_HIP(hipMemcpy2D(buf.p, (size_t)rows * 8, src, (size_t)ld * 8, (size_t)rows * 8, (size_t)cols, hipMemcpyHostToDevice));
  *ld_out = rows;
  return buf.p;
}

// the device results of a moment pass, one allocation: PtX0 (L K), G0 (K K), csX0 (K), PtF (L B), X0tF (K B), csF, sqF (B)
struct MomentBufs {
  DevBuf<double> all, partial;
  MomentOut o{};
  void alloc(int L, int K, int64_t B) {
    double *p = all.ensure((size_t)L * K + (size_t)K * K + K + (size_t)(L + K + 2) * B);
    o.PtX0 = p, p += (size_t)L * K;
    o.G0 = p, p += (size_t)K * K;
    o.csX0 = p, p += K;
    o.PtF = p, p += (size_t)L * B;
    o.X0tF = p, p += (size_t)K * B;
    o.csF = p, p += B;
    o.sqF = p;
  }
};

void fetch(double *dst, const double *d_src, size_t count) {
  if (dst && count) BSN_HIP(hipMemcpy(dst, d_src, count * 8, hipMemcpyDeviceToHost));
}

void moments_entry(const double *P, int64_t ldp, const double *X0, int64_t ldx, const double *F, int64_t ldf, int64_t M, int64_t L,
                   int64_t K, int64_t B, int is_device, double *PtX0, double *PtF, double *G0, double *X0tF, double *csX0, double *csF,
                   double *sqF) {
  check_shape(M, L, K, B);
  if (!P || !X0 || (B > 0 && !F)) fail("snp_ancestry_summary: no matrix");
  if (ldp < M || ldx < M || (B > 0 && ldf < M)) fail("snp_ancestry_summary: Incompatibility between dimensions (leading dimension).");
  require_gpu();
  g_last_ms[0] = g_last_ms[1] = g_last_ms[2] = 0.0;
  DevBuf<double> b_P, b_X0, b_F;
  const double *d_P = on_device(P, ldp, M, L, is_device, b_P, &ldp), *d_X0 = on_device(X0, ldx, M, K, is_device, b_X0, &ldx),
               *d_F = on_device(F, ldf, M, B, is_device, b_F, &ldf);
  MomentBufs mb;
  mb.alloc((int)L, (int)K, B);
  EventMarks<2> ev;
  ev.mark(0, nullptr);
  moments_device(d_P, ldp, d_X0, ldx, d_F, ldf, M, (int)L, (int)K, B, mb.o, mb.partial, nullptr);
  ev.mark(1, nullptr);
  BSN_HIP(hipStreamSynchronize(nullptr));
  g_last_ms[1] = ev.ms(0, 1);
  fetch(PtX0, mb.o.PtX0, (size_t)L * K);
  fetch(G0, mb.o.G0, (size_t)K * K);
  fetch(csX0, mb.o.csX0, (size_t)K);
  fetch(PtF, mb.o.PtF, (size_t)L * B);
  fetch(X0tF, mb.o.X0tF, (size_t)K * B);
  fetch(csF, mb.o.csF, (size_t)B);
  fetch(sqF, mb.o.sqF, (size_t)B);
}

void summary_entry(const double *F, int64_t ldf, int64_t B, const double *X0, int64_t ldx, const double *P, int64_t ldp,
                   const double *correction, int64_t M, int64_t L, int64_t K, const double *Dmat, int sum_to_one, int is_device,
                   double *w, double *cor_each, double *cor_pred, int32_t *steps) {
  check_shape(M, L, K, B);
  if (!P || !X0 || !correction || (B > 0 && (!F || !w || !cor_each || !cor_pred || !steps))) fail("snp_ancestry_summary: no buffer");
  if (ldp < M || ldx < M || (B > 0 && ldf < M)) fail("snp_ancestry_summary: Incompatibility between dimensions (leading dimension).");
  const std::vector<double> DJ = factor_checked(K, Dmat, "snp_ancestry_summary");
  DevBuf<double> d_DJ;
  require_gpu();
  upload(DJ, d_DJ);
  g_last_ms[0] = g_last_ms[1] = g_last_ms[2] = 0.0;
  if (B == 0) return;
  DevBuf<double> b_P, b_X0, b_F, d_corr, d_res;
  DevBuf<int32_t> d_steps;
  const double *d_P = on_device(P, ldp, M, L, is_device, b_P, &ldp), *d_X0 = on_device(X0, ldx, M, K, is_device, b_X0, &ldx),
               *d_F = on_device(F, ldf, M, B, is_device, b_F, &ldf);
  BSN_HIP(hipMemcpy(d_corr.ensure((size_t)L), correction, (size_t)L * 8, hipMemcpyHostToDevice));
  MomentBufs mb;
  mb.alloc((int)L, (int)K, B);
  double *res = d_res.ensure((size_t)(2 * K + 1) * B);
  d_steps.ensure((size_t)B);
  EventMarks<3> ev;
  ev.mark(0, nullptr);
  moments_device(d_P, ldp, d_X0, ldx, d_F, ldf, M, (int)L, (int)K, B, mb.o, mb.partial, nullptr);
  ev.mark(1, nullptr);
  QpArgs a{};
  a.K = (int)K, a.L = (int)L, a.sum_to_one = sum_to_one, a.B = B, a.M = (double)M;
  a.D = d_DJ.p, a.J0 = d_DJ.p + K * K, a.X = mb.o.PtX0, a.corr = d_corr.p, a.G0 = mb.o.G0, a.c0 = mb.o.csX0;
  a.l = mb.o.PtF, a.l_ldj = 1, a.l_ldb = L;
  a.xf = mb.o.X0tF, a.xf_ldk = 1, a.xf_ldb = K;
  a.fs = mb.o.csF, a.fq = mb.o.sqF;
  a.w = res, a.cor_each = res + K * B, a.cor_pred = res + 2 * K * B, a.steps = d_steps.p;
  qp_launch(a, nullptr);
  ev.mark(2, nullptr);
  BSN_HIP(hipStreamSynchronize(nullptr));
  g_last_ms[1] = ev.ms(0, 1);
  g_last_ms[2] = ev.ms(1, 2);
  fetch(w, a.w, (size_t)K * B);
  fetch(cor_each, a.cor_each, (size_t)K * B);
  fetch(cor_pred, a.cor_pred, (size_t)B);
  BSN_HIP(hipMemcpy(steps, d_steps.p, (size_t)B * 4, hipMemcpyDeviceToHost));
}

void bed_ancestry(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const double *X0, const double *P,
                  const double *correction, int64_t L, int64_t K, const double *Dmat, const double *Xproj, int sum_to_one, double *w,
                  double *cor_each, double *cor_pred, int32_t *steps) {
  if (!bed) fail("bed_ancestry: no handle");
  check_shape(m, L, K, n);
  if (!X0 || !P || !correction || !Xproj || (n > 0 && (!w || !cor_each || !cor_pred || !steps))) fail("bed_ancestry: no buffer");
  require_bits(bed, 2, "bed_ancestry");
  const std::vector<double> DJ = factor_checked(K, Dmat, "bed_ancestry");
  DevBuf<double> d_DJ;
  require_gpu();
  BSN_HIP(hipSetDevice(bed->device));
  upload(DJ, d_DJ);
  g_last_ms[0] = g_last_ms[1] = g_last_ms[2] = 0.0;
  if (n == 0) return;

  // V = [P | X0 | c | 1], c_j = mean_k X0[j, k]; the operator A~ = (g - 2 c) / 2, a missing genotype is 0 in it
  const int64_t nv = L + K + 2;
  std::vector<double> V((size_t)m * nv), center((size_t)m), scale((size_t)m, 2.0);
  std::memcpy(V.data(), P, (size_t)m * L * 8);
  std::memcpy(V.data() + (size_t)m * L, X0, (size_t)m * K * 8);
  double *cc = V.data() + (size_t)m * (L + K), *ones = cc + m;
  for (int64_t j = 0; j < m; j++) {
    double s = 0.0;
    for (int64_t k = 0; k < K; k++) s += X0[j + k * m];
    cc[j] = s / (double)K;
    center[(size_t)j] = 2.0 * cc[j];
    ones[j] = 1.0;
  }
  bsn_op op;
  fill_op(&op, bed, ind_row, n, ind_col, m, center.data(), scale.data());
  op.slices = 7;
  hipStream_t st = bed->stream;
  DevBuf<double> d_V, d_XV, d_r, d_small, d_res;
  DevBuf<int32_t> d_steps;
  copy_h2d(bed, d_V.ensure((size_t)m * nv), V.data(), (size_t)m * nv * 8);
  std::vector<double> small((size_t)L + (size_t)L * K);
  std::memcpy(small.data(), correction, (size_t)L * 8);
  std::memcpy(small.data() + L, Xproj, (size_t)L * K * 8);
  copy_h2d(bed, d_small.ensure(small.size()), small.data(), small.size() * 8);
  d_XV.ensure((size_t)n * nv);
  d_r.ensure((size_t)n);
  double *res = d_res.ensure((size_t)(2 * K + 1) * n);
  d_steps.ensure((size_t)n);
  MomentBufs mb;
  mb.alloc((int)L, (int)K, 1);

  EventMarks<4> ev;
  ev.mark(0, st);
  op_prod(&op, d_V.p, m, (int)nv, d_XV.p, n);
  op_row_sums_sq(&op, d_r.p);
  ev.mark(1, st);
  // the moments of the tables, with c as the one frequency column: X0'X0, 1'X0, and the offsets c'P, c'X0, sum c, sum c^2
  moments_device(d_V.p, m, d_V.p + m * L, m, d_V.p + m * (L + K), m, m, (int)L, (int)K, 1, mb.o, mb.partial, st);
  ev.mark(2, st);
  // from d = g / 2 - c (row i of XV: d'P, d'X0, d'c, d'1):  f'V = d'V + c'V, sum f = d'1 + sum c, sum f^2 = |d|^2 + 2 d'c + sum c^2
  double off[2];
  BSN_HIP(hipStreamSynchronize(st));
  BSN_HIP(hipMemcpy(off, mb.o.csF, 8, hipMemcpyDeviceToHost));
  BSN_HIP(hipMemcpy(off + 1, mb.o.sqF, 8, hipMemcpyDeviceToHost));
  QpArgs a{};
  a.K = (int)K, a.L = (int)L, a.sum_to_one = sum_to_one, a.B = n, a.M = (double)m;
  a.D = d_DJ.p, a.J0 = d_DJ.p + K * K, a.X = d_small.p + L, a.corr = d_small.p, a.G0 = mb.o.G0, a.c0 = mb.o.csX0;
  a.l = d_XV.p, a.l_ldj = n, a.l_ldb = 1, a.l_off = mb.o.PtF;
  a.xf = d_XV.p + n * L, a.xf_ldk = n, a.xf_ldb = 1, a.xf_off = mb.o.X0tF;
  a.fs = d_XV.p + n * (L + K + 1), a.fs_off = off[0];
  a.fq = d_r.p, a.dc = d_XV.p + n * (L + K), a.fq_off = off[1];
  a.w = res, a.cor_each = res + K * n, a.cor_pred = res + 2 * K * n, a.steps = d_steps.p;
  qp_launch(a, st);
  ev.mark(3, st);
  copy_d2h(bed, w, a.w, (size_t)K * n * 8);
  copy_d2h(bed, cor_each, a.cor_each, (size_t)K * n * 8);
  copy_d2h(bed, cor_pred, a.cor_pred, (size_t)n * 8);
  copy_d2h(bed, steps, d_steps.p, (size_t)n * 4);
  BSN_HIP(hipStreamSynchronize(st));
  g_last_ms[0] = ev.ms(0, 1);
  g_last_ms[1] = ev.ms(1, 2);
  g_last_ms[2] = ev.ms(2, 3);
}

}  // namespace
}  // namespace bsn

extern "C" {

int bsn_qp_max_k(void) { return bsn::qp::kMaxK; }

int bsn_qp_simplex(const double *D, int64_t K, const double *dvec, int64_t B, int32_t sum_to_one, double *w_out, int32_t *steps_out,
                   int64_t *n_failed) {
  return bsn::guarded([&] { bsn::qp_host(D, K, dvec, B, sum_to_one, w_out, steps_out, n_failed); });
}

int bsn_ancestry_moments(const double *P, int64_t ldp, const double *X0, int64_t ldx, const double *F, int64_t ldf, int64_t M, int64_t L,
                         int64_t K, int64_t B, int32_t on_device, double *PtX0, double *PtF, double *G0, double *X0tF, double *csX0,
                         double *csF, double *sqF) {
  return bsn::guarded([&] { bsn::moments_entry(P, ldp, X0, ldx, F, ldf, M, L, K, B, on_device, PtX0, PtF, G0, X0tF, csX0, csF, sqF); });
}

int bsn_ancestry_summary(const double *F, int64_t ldf, int64_t B, const double *X0, int64_t ldx, const double *P, int64_t ldp,
                         const double *correction, int64_t M, int64_t L, int64_t K, const double *Dmat, int32_t sum_to_one,
                         int32_t on_device, double *w, double *cor_each, double *cor_pred, int32_t *steps) {
  return bsn::guarded([&] {
    bsn::summary_entry(F, ldf, B, X0, ldx, P, ldp, correction, M, L, K, Dmat, sum_to_one, on_device, w, cor_each, cor_pred, steps);
  });
}

int bsn_bed_ancestry(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const double *X0,
                     const double *P, const double *correction, int64_t L, int64_t K, const double *Dmat, const double *Xproj,
                     int32_t sum_to_one, double *w, double *cor_each, double *cor_pred, int32_t *steps) {
  return bsn::guarded([&] {
    bsn::bed_ancestry(bed, ind_row, n, ind_col, m, X0, P, correction, L, K, Dmat, Xproj, sum_to_one, w, cor_each, cor_pred, steps);
  });
}

int bsn_ancestry_last_ms(double *ms_out) {
  return bsn::guarded([&] {
    for (int k = 0; k < 3; k++) ms_out[k] = bsn::g_last_ms[k];
  });
}

}  // extern "C"
