// project.hip — the OADP projection on the device: bsn_pca_oadp_proj (host buffers in, host buffers out) and
// bsn_bed_project_pca (the simple projection X V, the squared row norms and the OADP projection of a resident image in one
// call, the three results coming back together).
//
// Replaces bigutilsr::pca_OADP_proj2 behind OADP_proj of R/bed-projectPCA.R:62-67 of the reference: n independent dense
// problems of order K + 1, each a pair of one-sided Jacobi decompositions.  The per-sample statement lives in
// oadp_step.hpp, shared with the CPU statement.  DESIGN.md 3.5l.
//
// Lane mapping.  A group of W lanes of one wave works on one sample, W the smallest of 8, 16, 32, 64 that is >= K + 1, so
// that lane i owns row i of the sample's two matrices and a wave holds 64 / W samples.  The matrices live in LDS
// (oadp::work_doubles(K) doubles per sample); a workgroup is ONE wave, so nothing in the kernel waits for another wave
// and no workgroup barrier is needed: the group's lanes run in lockstep, its dot products are butterflies of __shfl_xor
// inside the group, and where a lane reads what another lane of its group wrote a wave-scope fence keeps the compiler
// from moving the accesses (the LDS serves one wave's accesses in order).
#include <algorithm>

#include "bsn_internal.hpp"
#include "lane_group.hpp"
#include "oadp_step.hpp"

namespace bsn {
namespace {

// device milliseconds of the last call of this process (bsn_project_last_ms): the product and row-norm passes, the OADP launch
double g_last_ms[2] = {0.0, 0.0};

constexpr int kWave = kLaneGroupWave;   // LaneGroup: lane_group.hpp

// XV, out: n x K column-major; one sample per group of W lanes, 64 / W samples per workgroup of one wave
template <int W>
__global__ __launch_bounds__(kWave) void k_oadp(const double *__restrict__ XV, const double *__restrict__ xnorm,
                                                const double *__restrict__ sval, int64_t n, int K, double *__restrict__ out) {
  extern __shared__ double oadp_lds[];
  const int grp = (int)threadIdx.x / W;
  const int64_t i = (int64_t)blockIdx.x * (kWave / W) + grp;
  if (i >= n) return;   // the whole group leaves: nothing below waits for it
  const LaneGroup<W> g{(int)threadIdx.x % W};
  oadp::project_one(g, K, sval, XV + i, n, xnorm[i], oadp_lds + (size_t)grp * oadp::work_doubles(K), out + i, n);
}

int group_width(int K) { return K + 1 <= 8 ? 8 : K + 1 <= 16 ? 16 : K + 1 <= 32 ? 32 : 64; }

// queues the launch on `st`; d_sval has passed oadp::check_args on the host
void oadp_launch(const double *d_XV, const double *d_xnorm, const double *d_sval, int64_t n, int K, double *d_out, hipStream_t st) {
  const int W = group_width(K);
  const int per_wg = kWave / W;
  const int64_t blocks = (n + per_wg - 1) / per_wg;
  if (blocks > 0x7fffffffLL) fail("pca_OADP_proj: too many samples for one launch.");
  const size_t lds = (size_t)per_wg * oadp::work_doubles(K) * 8;
  static_assert((size_t)oadp::work_doubles(oadp::kMaxK) * 8 <= 65536, "a sample's work space exceeds the default LDS limit");
  const dim3 grid((unsigned)blocks), block(kWave);
  switch (W) {
    case 8: hipLaunchKernelGGL(k_oadp<8>, grid, block, lds, st, d_XV, d_xnorm, d_sval, n, K, d_out); break;
    case 16: hipLaunchKernelGGL(k_oadp<16>, grid, block, lds, st, d_XV, d_xnorm, d_sval, n, K, d_out); break;
    case 32: hipLaunchKernelGGL(k_oadp<32>, grid, block, lds, st, d_XV, d_xnorm, d_sval, n, K, d_out); break;
    default: hipLaunchKernelGGL(k_oadp<64>, grid, block, lds, st, d_XV, d_xnorm, d_sval, n, K, d_out); break;
  }
  BSN_HIP(hipGetLastError());
}

void check_oadp_args(int64_t K, const double *sval) {
  if (const char *why = oadp::check_args(K, sval)) fail("%s", why);
}

void oadp_host(const double *XV, const double *X_norm, const double *sval, int64_t n, int64_t K, double *out) {
  require_gpu();
  check_oadp_args(K, sval);
  if (n < 0) fail("pca_OADP_proj: negative number of samples");
  g_last_ms[0] = g_last_ms[1] = 0.0;
  if (n == 0) return;
  if (!XV || !X_norm || !out) fail("pca_OADP_proj: no buffer");
  DevBuf<double> d_XV, d_r, d_s, d_out;
  BSN_HIP(hipMemcpy(d_XV.ensure((size_t)n * K), XV, (size_t)n * K * 8, hipMemcpyHostToDevice));
  BSN_HIP(hipMemcpy(d_r.ensure((size_t)n), X_norm, (size_t)n * 8, hipMemcpyHostToDevice));
  BSN_HIP(hipMemcpy(d_s.ensure((size_t)K), sval, (size_t)K * 8, hipMemcpyHostToDevice));
  d_out.ensure((size_t)n * K);
  EventMarks<2> ev;
  ev.mark(0, nullptr);
  oadp_launch(d_XV.p, d_r.p, d_s.p, n, (int)K, d_out.p, nullptr);
  ev.mark(1, nullptr);
  BSN_HIP(hipStreamSynchronize(nullptr));
  BSN_HIP(hipMemcpy(out, d_out.p, (size_t)n * K * 8, hipMemcpyDeviceToHost));
  g_last_ms[1] = ev.ms(0, 1);
}

// what bsn_bed_prod_and_rowsumssq does, followed by the OADP launch on the device buffers
void bed_project_pca(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const double *center,
                     const double *scale, const double *V, int64_t K, const double *sval, double *XV, double *rowSumsSq,
                     double *OADP) {
  if (K <= 0) fail("'V' must have at least one column.");
  check_oadp_args(K, sval);
  if (!XV || !rowSumsSq || !OADP) fail("bed_projectPCA: no result buffer");
  bsn_op op;
  fill_op(&op, bed, ind_row, n, ind_col, m, center, scale);
  op.slices = 7;
  hipStream_t st = bed->stream;
  DevBuf<double> d_V, d_XV, d_r, d_s, d_out;
  copy_h2d(bed, d_V.ensure((size_t)m * K), V, (size_t)m * K * 8);
  copy_h2d(bed, d_s.ensure((size_t)K), sval, (size_t)K * 8);
  d_XV.ensure((size_t)n * K);
  d_r.ensure((size_t)n);
  d_out.ensure((size_t)n * K);
  EventMarks<3> ev;
  ev.mark(0, st);
  op_prod(&op, d_V.p, m, (int)K, d_XV.p, n);
  op_row_sums_sq(&op, d_r.p);
  ev.mark(1, st);
  oadp_launch(d_XV.p, d_r.p, d_s.p, n, (int)K, d_out.p, st);
  ev.mark(2, st);
  copy_d2h(bed, XV, d_XV.p, (size_t)n * K * 8);
  copy_d2h(bed, rowSumsSq, d_r.p, (size_t)n * 8);
  copy_d2h(bed, OADP, d_out.p, (size_t)n * K * 8);
  BSN_HIP(hipStreamSynchronize(st));
  g_last_ms[0] = ev.ms(0, 1);
  g_last_ms[1] = ev.ms(1, 2);
}

}  // namespace
}  // namespace bsn

extern "C" {

int bsn_pca_oadp_proj(const double *XV, const double *X_norm, const double *sval, int64_t n, int64_t K, double *out) {
  return bsn::guarded([&] { bsn::oadp_host(XV, X_norm, sval, n, K, out); });
}

int bsn_bed_project_pca(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const double *center,
                        const double *scale, const double *V, int64_t K, const double *sval, double *XV, double *rowSumsSq,
                        double *OADP) {
  return bsn::guarded(
      [&] { bsn::bed_project_pca(bed, ind_row, n, ind_col, m, center, scale, V, K, sval, XV, rowSumsSq, OADP); });
}

int bsn_project_last_ms(double *ms_out) {
  return bsn::guarded([&] {
    for (int k = 0; k < 2; k++) ms_out[k] = bsn::g_last_ms[k];
  });
}

}  // extern "C"
