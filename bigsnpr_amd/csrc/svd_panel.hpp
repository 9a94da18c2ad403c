// svd_panel.hpp — the launches of the panel kernels of the block-Lanczos solve (svd_panel.hip): the tall-skinny fp64
// algebra between the streaming passes.  One free function per launch: grid, block, template choice and LDS size live
// there and nowhere else, so that the backend (svd.hip) and the kernel-level test entries (bsn_panel_*) run the same launches.
#pragma once
#include "bsn_internal.hpp"
#include "orth_small.hpp"

namespace bsn {

constexpr int kMaxB = kOrthMaxB;   // vectors per pass = columns of a panel (orth_small.hpp): sizes the kernels' register arrays
constexpr int64_t kGemmRows = 1024;   // rows per workgroup of k_gemm_tn (4 waves x 256)
// doubles of `partial` that panel_gemm_tn writes for operands of `rows` rows and p columns of A
inline size_t panel_partial_count(int64_t rows, int p) {
  return (size_t)((rows + kGemmRows - 1) / kGemmRows) * (size_t)((p + 15) / 16) * 2 * 256;
}

// rows [row0, row0 + n) of the n_total x b start block into W (leading dimension ld); rows past n_total are zero
void panel_random(hipStream_t st, double *W, int64_t ld, int64_t n, int b, uint32_t seed, int64_t row0, int64_t n_total);
// M[:r, :r] (leading dimension ld) = src (r x r)
void panel_put_block(hipStream_t st, double *M, int ld, int r, const double *src);
// dC (p x cb, leading dimension ldc) = A[:, :p]' B[:, :cb] for operands with `rows` rows; cb <= 32
void panel_gemm_tn(hipStream_t st, const double *A, int64_t lda, int p, const double *B, int64_t ldb, int cb, int64_t rows,
                   double *dC, int ldc, double *partial);
void panel_gemm_nn(hipStream_t st, const double *Q, int64_t ldq, int p, const double *S, int nc, const double *In, int64_t ldi,
                   double alpha, double beta, double *Out, int64_t ldo, int64_t n);
void panel_right_mult(hipStream_t st, double *W, int64_t ld, int64_t n, int cb, int r, const double *M);
void panel_update(hipStream_t st, const double *Q, int64_t ldq, int p, const double *C, const double *Ri, int cb, double *W,
                  int64_t ldw, int64_t n, unsigned long long *mx);
void panel_orth2(hipStream_t st, const OrthSmall &a, unsigned long long *mx_clear);
// wide: 256 workgroups per column (a whole panel on one GPU), else 64 (a rank's sample block)
void panel_col_absmax(hipStream_t st, const double *X, int64_t ld, int64_t n, int cb, unsigned long long *mx, bool wide);
void panel_round_cols(hipStream_t st, double *X, int64_t ld, int64_t n, int cb, const unsigned long long *mx, int slices);
void panel_block(hipStream_t st, const double *full, int64_t n, int cb, int64_t nr, int world, double *blk);
void panel_unblock(hipStream_t st, const double *blk, int64_t n, int cb, int64_t nr, double *full);
void panel_place_rows(hipStream_t st, const double *src, int64_t rows, int cb, int64_t r0, int64_t nr, double *W);
void panel_take_rows(hipStream_t st, const double *full, int64_t n, int cb, int64_t nr, int64_t row0, double *W);
void panel_max_over_ranks(hipStream_t st, const unsigned long long *all, int world, int cb, unsigned long long *mx);
// int16 up to 16 bits (slices <= 2), int32 up to 32: q is the rank's [column][row] block of integers
void panel_pack_int(hipStream_t st, double *W, int64_t nr, int cb, const unsigned long long *mx, int slices, void *q);
void panel_unpack_int(hipStream_t st, const void *q_all, int64_t n, int cb, int64_t nr, const unsigned long long *mx, int slices,
                      double *full);

}  // namespace bsn
