/*
 * bigsnpr_hip.h — C ABI of libbigsnpr_hip.so: the MI355X (gfx950) implementation of
 * bigsnpr's genotype-matrix hot path.
 *
 * This is the drop-in boundary.  Every entry point replaces one `.Call` target of
 * the reference package (bigsnpr 1.12.21, registration table
 * src/RcppExports.cpp:597-640) or one operator that the reference hands to
 * bigstatsr::big_randomSVD (R/autoSVD.R:216-218).  The reference-side binding (an R
 * `.Call` shim) is shown in INTEGRATION.md and bindings/R/.
 *
 * Conventions
 *  - plain C types only; no R, Rcpp, torch or HIP types in any signature;
 *  - all functions return 0 on success, non-zero on error; bsn_last_error() then
 *    returns a thread-local message whose text matches the reference's
 *    Rcpp::stop() strings where the reference has one;
 *  - indices are 0-based int64 (the R shim subtracts 1 exactly where the reference
 *    does, src/bed-acc.h:64-65); arbitrary order, duplicates allowed;
 *  - `*_host` style pointers are borrowed host buffers (never freed, never kept);
 *    `d_*` pointers are device (HBM) pointers on the handle's device;
 *  - a handle owns the device image of one genotype matrix; it is created on the
 *    current device (bsn_set_device) and all work is issued on its own HIP stream.
 *  - There is NO CPU fallback: without a gfx950 device every compute call fails.
 */
#ifndef BIGSNPR_HIP_H
#define BIGSNPR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bsn_bed bsn_bed; /* packed 2-bit genotype matrix resident in HBM */
typedef struct bsn_op bsn_op;   /* scaled sub-view  A~ = ((G - center)/scale)[ind_row, ind_col] */

/* ---- runtime ------------------------------------------------------------- */
const char *bsn_last_error(void);
int bsn_version(void);
int bsn_device_count(int *count);
int bsn_set_device(int device);
/* verifies the gfx950 instruction-level assumptions the kernels rely on
 * (v_perm_b32 byte order, i8 MFMA operand/accumulator layout) on the device */
int bsn_selftest(void);

/* ---- genotype image (replaces `class bed` + bedXPtr) ----------------------
 * src/bed-acc.h:18-48, src/bed-acc-xptr.cpp:14-53 (_bigsnpr_bedXPtr, 3 args).
 * Error strings: "Error when mapping file:\n  %s.\n", "File is not a binary PED
 * file.", "Variant-major is the only mode supported.", "n or p does not match the
 * dimensions of the file." */
int bsn_bed_open(const char *path, int64_t n, int64_t m, bsn_bed **out);
/* 1 if the handle is OUT OF CORE (round 4): the file's 2-bit image did not fit the free device memory (or the budget
 * BSN_IMAGE_BUDGET, bytes) when bsn_bed_open was called, so the file stays mapped and bsn_bed_prodvec, bsn_bed_cprodvec,
 * bsn_bed_col_counts and bsn_bed_colstats walk it in slabs of variants (PCIe-bound instead of HBM-bound; same kernels,
 * same results).  The reference maps a file of any size (src/bed-acc.h:46); every other entry point refuses such a
 * handle with the reason. */
int bsn_bed_is_streamed(const bsn_bed *bed);
/* same, from a payload already in host memory (n_byte = bytes per variant, >= ceil(n/4)) */
int bsn_bed_from_host(const uint8_t *payload, int64_t n, int64_t m, int64_t n_byte, bsn_bed **out);
/* FBM.code256 (bigstatsr, one byte per genotype, column-major, n_total rows) with the
 * CODE_012 coding (R/bigSNP-class.R:7: 0,1,2, everything else NA) repacked to 2 bits
 * on the device; the FBM twin of bedXPtr for snp_* functions (src/colstats.cpp:13-14). */
int bsn_bed_from_fbm(const uint8_t *bytes, int64_t n, int64_t m, int64_t ld, bsn_bed **out);
/* The same for any FBM.code256: `code256` is the object's 256-entry decode table (R/bigSNP-class.R:7-13).
 * Tables that decode to genotype calls only (0 / 1 / 2 / NA: CODE_012, CODE_IMPUTE_PRED) give the 2-bit
 * image and every entry point of this header.  Tables whose values lie on a regular grid of at most 255
 * steps (CODE_DOSAGE: calls, imputed calls and dosages 0.00 .. 2.00 by 0.01) give a BYTE image — one int8
 * grid index per genotype, exact integer sums, the affine map back to values applied in fp64 — which
 * serves bsn_snp_colstats, bsn_bed_prodvec / bsn_bed_cprodvec (big_prodVec / big_cprodVec and so snp_PRS),
 * bsn_op_*, bsn_bed_randomsvd with explicit centre / scale and, for data without missing values,
 * bsn_cormat / bsn_ld_scores / bsn_clumping_chr(_cached) in the FBM mode; the other entry points fail on it
 * with a message.  Any other table is refused. */
int bsn_fbm_open(const uint8_t *bytes, int64_t n, int64_t m, int64_t ld, const double *code256, bsn_bed **out);
int bsn_bed_bits(const bsn_bed *bed); /* 2 or 8 */
/* total number of missing genotypes of the image if a full count has seen every variant (FBM handles
 * know it from their creation), -1 otherwise */
int64_t bsn_bed_na_known(const bsn_bed *bed);
/* synthetic matrix generated directly in HBM (DESIGN.md "Synthetic inputs");
 * byte-identical to oracle/bsn_oracle.c:orc_fake_bed */
int bsn_bed_synthetic(int64_t n, int64_t m, uint32_t seed, uint32_t npop, uint32_t na16,
                      int64_t j_begin, bsn_bed **out);
int bsn_bed_close(bsn_bed *bed);
int64_t bsn_bed_nrow(const bsn_bed *bed);
int64_t bsn_bed_ncol(const bsn_bed *bed);
int64_t bsn_bed_bytes(const bsn_bed *bed); /* HBM bytes held by the image */
/* copies the image back in .bed payload layout (ceil(n/4) bytes per variant) */
int bsn_bed_download(bsn_bed *bed, uint8_t *payload_out);

/* ---- .Call replacements (host buffers in, host buffers out) --------------- */
/* _bigsnpr_bed_pMatVec4 (7 args) src/bed-prod-vec.cpp:15-54 — R: bed_prodVec.
 * y[n] = A~ x[m].  "Incompatibility between dimensions" is raised by the caller
 * layer (lengths are explicit here). `ncores` of the reference is dropped. */
int bsn_bed_prodvec(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                    int64_t m, const double *center, const double *scale, const double *x,
                    double *y);
/* _bigsnpr_bed_cpMatVec4 (7 args) src/bed-prod-vec.cpp:59-97 — R: bed_cprodVec. z[m] = A~' x[n] */
int bsn_bed_cprodvec(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                     int64_t m, const double *center, const double *scale, const double *x,
                     double *z);

/* bed_prodVec on a column-sharded matrix ("each GPU produces a partial n-vector, one all-reduce"):
 * every rank passes its own shard (handle, ind_col, center / scale and the matching slice of x) and the
 * communicator of bsn_comm_init; y[n] receives the sum over the ranks — the product with the whole matrix — on
 * every rank.  The partial vectors are added on the device over RCCL (fp64, 3.2 MB at 400 000 samples) before
 * the one download.  comm == NULL: plain bsn_bed_prodvec.  The crossproduct needs no counterpart: z = A~' x is
 * sharded like the columns, bsn_bed_cprodvec on every rank already returns that rank's slice. */
struct bsn_comm;
int bsn_bed_prodvec_sharded(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                            int64_t m, const double *center, const double *scale, const double *x,
                            struct bsn_comm *comm, double *y);
/* _bigsnpr_bed_col_counts_cpp (4 args) src/bed-fun.cpp:51-69: res is 4 x m column-major
 * (rows: counts of 0, 1, 2, NA) */
int bsn_bed_col_counts(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                       int64_t m, int32_t *res);
/* _bigsnpr_bed_row_counts_cpp (4 args) src/bed-fun.cpp:72-99 (bed_counts(byrow = TRUE),
 * R/binom-scaling.R:166-178): per SAMPLE counts of 0, 1, 2, NA over the selected variants,
 * res[4 x n] column-major. */
int bsn_bed_row_counts(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m,
                       int32_t *res);
/* _bigsnpr_bed_colstats (4 args) src/bed-fun.cpp:9-46; *n_bad = number of variants with
 * more than 50 % missing values (the reference warns "%d variants have >50%% missing values.") */
int bsn_bed_colstats(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                     int64_t m, double *sumX, double *denoX, int32_t *nb_nona_col, int32_t *n_bad);
/* _bigsnpr_snp_colstats (4 args) src/colstats.cpp:8-35 (no NA handling: NA counts as 3
 * exactly as code256[3] would if it were 3; callers assert no NA, R/utils-assert.R:31) */
int bsn_snp_colstats(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                     int64_t m, double *sumX, double *denoX);
/* _bigsnpr_read_bed (3 args) / _bigsnpr_read_bed_scaled (5 args) src/bed-mat-acc.cpp:8-49:
 * dense n x m column-major; read_bed codes NA as na_val */
int bsn_bed_read(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                 int64_t m, int32_t na_val, int32_t *out);
int bsn_bed_read_scaled(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                        int64_t m, const double *center, const double *scale, double *out);

/* The genotype-touching part of _bigsnpr_multLinReg (5 args, src/multLinReg.cpp:8-86; SURVEY.md
 * §8f-2): for every variant j and column k of X (n x K, e.g. PC scores)
 *   P[j, k] = sum_i g_ij X[i, k] over non-missing genotypes,  Q[j, k] = sum_{i: g_ij missing} X[i, k]
 * (m x K column-major).  With the genotype counts these give xySum, ySum, yySum of the reference;
 * the K t-scores per variant are then a few flops on the host (bigsnpr_amd/pcadapt.py). */
int bsn_bed_cprod_planes(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                         int64_t m, const double *X, int64_t K, double *P, double *Q);

/* _bigsnpr_multLinReg (5 args) src/multLinReg.cpp:8-86, whole: res[m x K] column-major, the t-score of
 * each variant regressed on each column of U (n x K) over its non-missing genotypes; NaN where the
 * reference returns NA_REAL (zero denominator or fewer than two non-missing values). */
int bsn_mult_lin_reg(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m,
                     const double *U, int64_t K, double *res);

/* bigstatsr::big_univLinReg: per variant x of the selection, the least-squares coefficient of x in y ~ x + 1 + covar and
 * its standard error.  U (n x K column-major, K <= 31) is an orthonormal basis of the columns [1, covar] over the selected
 * rows (the host mirror takes it from their thin SVD); with y~ = y - U U' y:
 *   estim = x' y~ / den, den = x' x - |U' x|^2, std_err = sqrt((y~' y~ - estim x' y~) / (den (n - K - 1))).
 * A variant with a missing value among the rows, without variance over them, or with den <= 1e-14 x' x gives NaN in
 * both.  2-bit images and byte images on a grid (CODE_DOSAGE). */
int bsn_univ_linreg(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const double *y,
                    const double *U, int64_t K, double *estim, double *std_err);
/* bigstatsr::big_univLogReg: per variant x, the maximum-likelihood fit of y01 ~ x + 1 + covar (covar: n x q
 * column-major, q <= 30, may be NULL when q = 0) by iteratively reweighted least squares from the covariates-only fit,
 * which is computed inside.  Converged when max_k 2 |b_new - b_old| / (|b_new| + |b_old|) <= tol.  estim = the
 * coefficient of x, std_err = sqrt of the [0, 0] entry of the inverse of the last solve's weighted Gram matrix, niter =
 * the number of solves; niter = -1 with the last iterate when `maxiter` solves did not converge; NaN and niter = 0
 * for a variant with a missing value among the rows, without variance, or whose system is singular (a Cholesky pivot
 * at or below 1e-14 times its diagonal entry).  2-bit images and byte images on a grid. */
int bsn_univ_logreg(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const double *y01,
                    const double *covar, int64_t q, double tol, int32_t maxiter, double *estim, double *std_err,
                    int32_t *niter);

/* bigstatsr::big_spLinReg / big_spLogReg: elastic-net paths on individual-level data with cross-model selection and
 * averaging; the statement is DESIGN.md 3.5i (bigsnpr_amd/csrc/plr_step.hpp).  One chain per (alpha a, fold k),
 * c = a K + k, all chains resident on the device for the whole call.  Rows are the n rows of the selection; row i is a
 * validation row of chain (a, k) when fold[i] == k.  Columns are the m selected ones followed by the q covariates
 * (covar: n x q column-major, may be NULL when q = 0); pf [m + q] are the penalty factors (0: unpenalised).
 * Outputs, per chain c: intercept [C] and beta [(m + q) x C] of the chain's best model on the original scale;
 * lambda / loss / loss_val / iter / nb_active [nlambda x C] (entry 0 is the unpenalised start; NaN / 0 past n_done);
 * n_done [C] lambdas closed, best [C] the index of the best one, status [C]: 1 "No more improvement", 2 "Too many
 * variables", 3 "Model saturated", 4 "Complete path".  A missing value among the selection is refused.
 * bsn_bed_sp_reg: a resident 2-bit image or a byte image on a grid.  bsn_dense_sp_reg: a dense host matrix, column-major
 * with leading dimension ld, type 4 (float) or 7 (double) as in bsn_snp_grid_prs. */
typedef struct bsn_plr_options {
  int32_t family;          /* 0 linear, 1 logistic (y in {0, 1}) */
  int32_t nlambda;         /* length of the lambda grid, >= 2 */
  int32_t nlam_min;        /* no early stop before this many lambdas */
  int32_t n_abort;         /* lambdas without a better validation loss before "No more improvement" */
  int32_t dfmax;           /* non-zero coefficients at which a chain stops with "Too many variables" */
  int32_t max_iter;        /* coordinate passes per lambda */
  double eps;              /* convergence threshold relative to the null loss */
  double lambda_min_ratio; /* last lambda / first lambda */
} bsn_plr_options;
int bsn_bed_sp_reg(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const double *y,
                   const double *covar, int64_t q, const double *pf, const int32_t *fold, int32_t K, const double *alphas,
                   int32_t n_alpha, const bsn_plr_options *opt, double *intercept, double *beta, double *lambda,
                   double *loss, double *loss_val, int32_t *iter, int32_t *nb_active, int32_t *n_done, int32_t *best,
                   int32_t *status);
int bsn_dense_sp_reg(const void *X, int type, int64_t ld, int64_t n, int64_t m, const double *y, const double *covar,
                     int64_t q, const double *pf, const int32_t *fold, int32_t K, const double *alphas, int32_t n_alpha,
                     const bsn_plr_options *opt, double *intercept, double *beta, double *lambda, double *loss,
                     double *loss_val, int32_t *iter, int32_t *nb_active, int32_t *n_done, int32_t *best, int32_t *status);
/* the last bsn_*_sp_reg call of this process, device time from events: out[0] ms in sweeps, [1] ms in scans (scan, flag,
 * commit), [2] turns of the host loop, [3] coordinate updates (passes x active columns over all chains), [4] ms before the
 * first turn (statistics, start fit, lambda_max), [5] their sum.  One record per process, written without a lock (like
 * bsn_impute_last_ms): not meaningful when two host threads run bsn_*_sp_reg at the same time. */
int bsn_plr_last_stats(double *out /* 6 */);

/* _bigsnpr_impute (3 args) src/impute-simple.cpp:10-73 + R/impute.R:189-203 — R: snp_fastImputeSimple.
 * `src` is any resident 2-bit handle and is not modified; *out receives a NEW handle (the reference rewrites the FBM's
 * file in place and returns it under another decode table).  method: 0 zero, 1 mode, 2 mean0, 3 mean2, 4 random — the
 * reference's numbers plus 0.  With c1, c2 the numbers of calls 1 and 2, c the number of non-missing calls over all
 * samples and c0 = c - c1 - c2, every missing position of a variant receives
 *   zero    the call 0                                                        (FBM byte stays 3)
 *   mode    the most frequent call, ties to the smaller (lines 52-56)         (FBM byte 4 + v)
 *   mean0   nearbyint((c1 + 2.0 c2) / c), ties to even                        (FBM byte 4 + v)
 *   mean2   r / 100, r = nearbyint(100 * ((c1 + 2.0 c2) / c)) in fp64          (FBM byte 7 + r)
 *   random  (u0 < af) + (u1 < af), af = (0.5 c1 + c2) / c, u0 / u1 from one    (FBM byte 4 + v)
 *           Philox4x32-10 call keyed by `seed` with the counter (sample, variant): not R's generator
 * The result is a 2-bit image, for mean2 the int8 grid image of CODE_DOSAGE (v_off = 1, v_step = 0.01), exactly what
 * bsn_fbm_open makes of the FBM bytes under CODE_IMPUTE_PRED / CODE_DOSAGE / c(0, 1, 2, 0, NA ...).  A variant without
 * any call (c == 0) becomes 0 under zero and mode and STAYS MISSING under mean0, mean2 and random (the reference casts
 * a NaN to unsigned char there); *n_all_missing counts such variants for every method.  fbm_bytes_out (n x m
 * column-major, may be NULL) receives the content the reference's file would have; out may be NULL when only those
 * bytes are wanted.  Refused by name: a byte image, an out-of-core handle, a result that does not fit the free device
 * memory. */
int bsn_impute_simple(bsn_bed *src, int method, uint64_t seed, bsn_bed **out, uint8_t *fbm_bytes_out /* or NULL */,
                      int64_t *n_all_missing /* or NULL */);
/* device milliseconds (HIP events, host copies excluded) of the last bsn_impute_simple of this process: ms_out[0] the
 * counts (a counting pass, or a copy of the handle's resident counts) and the per-variant rule, [1] the rewrite of the
 * image, [2] the kernels that write the FBM bytes (0 when none were asked for) */
int bsn_impute_last_ms(double *ms_out);

/* R/impute.R:29-160 — R: snp_fastImpute, as one independent boosted-tree model per variant (the statement
 * is bigsnpr_amd/csrc/fastimpute_step.hpp).  `src` is any resident 2-bit handle and is not modified; *out receives a NEW
 * 2-bit handle (CODE_IMPUTE_PRED).  Variant j with a missing and an observed call is a target; its predictors are the
 * variants pred_idx[pred_off[j] .. pred_off[j + 1]) (ascending, never j, possibly none), read from `src` as the codes
 * 0, 1, 2, missing.  An observed sample trains with probability p_train (one Philox4x32-10 call keyed by `seed` with the
 * counter (sample, variant)) and validates otherwise; when nobody trains, all observed samples do.  Ten rounds of one
 * depth-4 tree on the logistic loss of call / 2 (eta 0.3, lambda 1, gamma 0, min_child_weight 1; exact greedy splits
 * over thresholds 0.5 / 1.5 / 2.5 with a learnt direction for missing codes; gradients quantised to 2^-30 and summed as
 * int64), then call = nearbyint(2 p) at every missing position.  infos (2 x m row-major, may be NULL): [0][j] the share
 * of missing calls, [1][j] the share of validation samples whose call differs from the observed one (NaN for a variant
 * that is no target or has no validation sample).  A variant without any observed call stays missing and is counted in
 * *n_all_missing.  fbm_bytes_out (n x m column-major, may be NULL): the content the reference's file would have
 * (4 + call at an imputed position).  Refused by name: a byte image, an out-of-core handle, p_train outside (0, 1], a
 * predictor outside [0, m) or equal to its target, a result image or scratch that does not fit the free device memory. */
int bsn_fast_impute(bsn_bed *src, const int64_t *pred_off /* [m+1] */, const int32_t *pred_idx, double p_train, uint64_t seed,
                    bsn_bed **out, uint8_t *fbm_bytes_out /* or NULL */, double *infos /* 2 x m */, int64_t *n_all_missing);
/* device milliseconds (HIP events, host copies excluded) of the last bsn_fast_impute of this process: ms_out[0] the
 * boosting kernel, [1] the copy of the image it rewrites, [2] the kernels that write the FBM bytes (0 when none were
 * asked for) */
int bsn_fast_impute_last_ms(double *ms_out);

/* ---- snp_readBGEN / snp_prodBGEN: inflate and decode BGEN on the device ----------------------------------
 * BGEN v1.2 files as the UK Biobank ships them (R/read-bgen.R, src/read-bgen.cpp, src/prod-bgen.cpp): layout 2, zlib,
 * two alleles, unphased, 8 bits per probability.  The probabilities of a variant are one zlib stream of 10 + 3 N bytes;
 * blocks of variants are uploaded compressed, inflated one wave per stream, and decoded.  The library links no zlib:
 * the statement of a stream is bigsnpr_amd/csrc/inflate_step.hpp.
 *
 * bsn_inflate: K independent zlib streams, stream k = in[in_off[k] .. in_off[k + 1]) into out[out_off[k] .. out_off[k + 1]),
 * whose length is both the room and the expected length (host buffers; the test seam).  status[k]:
 *   0 ok   1 bad zlib header   2 input exhausted   3 output would exceed its room   4 invalid block type, stored length
 *   or code   5 distance before the start of the output   6 Adler-32 mismatch   7 stream ended short of its length
 * A stream with a non-zero status leaves its part of `out` undefined; the call itself succeeds.
 *
 * bsn_bgen_read: the variants whose records start at offsets[0 .. K) of `path` (N samples; the rows ind_row[0 .. n), file
 * samples from 0, any order, repeats allowed) become columns col0 .. col0 + K - 1 of an n x m_total int8 grid image of
 * CODE_DOSAGE (v_off = 1, v_step = 0.01), exactly what bsn_fbm_open makes of the same FBM bytes.  *inout NULL: the image
 * is created (and freed again if the call fails); else it is filled.  dosage != 0: the FBM byte of a sample is
 * decode[2 p0 + p1] (511 bytes, the reference's 207 - round(0:510 * 100 / 255)); dosage == 0: the call 0 / 1 / 2 (FBM
 * byte 4 / 5 / 6) drawn with first = 255 u - p0, u from one Philox4x32-10 call keyed by `seed` with the counter
 * (position in ind_row, global column): not R's generator.  A ploidy byte >= 0x80 is a missing sample (FBM byte 3).
 * info_out / freq_out (K each, may be NULL): 1 - num 2 nona / (af (coef - af)) and 1 - af / coef from exact integer sums,
 * in the reference's operation order; NaN for a variant without a non-missing sample.  fbm_bytes_out: n x K column-major.
 * Errors keep the reference's words: "'%s' is not a BGEN file.", "... is not compressed with zlib.", "... is not using
 * Layout 2.", "Positions should be positive.", "Only 2 alleles allowed.", "Probabilities should be stored using 8 bits.",
 * "Problem when uncompressing." followed by the variant's index and the stream's status.  Refused by name: a byte of
 * `decode` above 207, a result image that does not fit the free device memory.
 *
 * bsn_bgen_prod: XY (n x ncol column-major, added to) += X Y with X the n x K matrix of the same variants, never stored:
 * x = decode[2 p0 + p1] (511 doubles, the reference's 510:0 / 255) or the drawn call, NaN for a missing sample (which
 * turns that sample's row into NaN); Y is K x ncol with leading dimension ldy.  fp64 throughout.
 *
 * bsn_bgen_last_ms: device milliseconds (HIP events) of the last of these calls of this process: [0] the inflate
 * kernel, [1] the conversion to image rows, [2] the product; a phase that did not run reports exactly 0. */
int bsn_inflate(const uint8_t *in, const int64_t *in_off /* K+1 */, int64_t K, uint8_t *out, const int64_t *out_off /* K+1 */,
                int32_t *status /* K */);
int bsn_bgen_read(const char *path, const int64_t *offsets, int64_t K, int64_t N, const int64_t *ind_row, int64_t n,
                  const uint8_t *decode /* 511 FBM bytes */, int dosage, uint64_t seed, int64_t col0, int64_t m_total,
                  int64_t block_variants /* 0: chosen from free memory */, bsn_bed **inout, uint8_t *fbm_bytes_out /* or NULL */,
                  double *info_out /* K */, double *freq_out /* K */);
int bsn_bgen_prod(const char *path, const int64_t *offsets, int64_t K, int64_t N, const int64_t *ind_row, int64_t n,
                  const double *decode /* 511 */, int dosage, uint64_t seed, int64_t col0, const double *Y, int64_t ldy,
                  int64_t ncol, int64_t block_variants, double *XY /* n x ncol, added to */);
int bsn_bgen_last_ms(double *ms_out /* 3: inflate, convert, product */);

/* ---- per-group genotype counts, snp_fst, snp_MAX3 ------------------------------------------------------
 * Counts of the four codes of every selected variant, split by a label on the selected rows, in ONE pass over the image
 * (the reference, and bsn_bed_col_counts, need one pass per group): res[4 * (G * j + g) + c] is the number of rows i with
 * group[i] == g whose code at variant ind_col[j] is c — c = 0, 1, 2, 3 (NA), the row order of bsn_bed_col_counts.
 * group[i] is 0 .. G - 1, or -1 for a row in no group; rows count as often as ind_row lists them, and a file row may be
 * listed under several groups.  The multiplicity panel (file rows x groups) is built on the device with integer atomics
 * and fills the digit columns of the streaming crossproduct kernel: 16 groups per column block while no multiplicity
 * exceeds 127, 4 otherwise; two column blocks per launch where that saves one.  Resident and out-of-core handles (slabs,
 * like bsn_bed_col_counts); the streaming-layout copy is read when the handle has one.  Refused with a message: G < 1, a
 * label outside -1 .. G - 1, a group of more than INT32_MAX rows, a byte (dosage) image.  The counts that
 * bsn_bed_col_counts keeps on the handle are neither read nor changed. */
int bsn_bed_group_counts(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int32_t *group /* [n] */, int32_t G,
                         const int64_t *ind_col, int64_t m, int32_t *res /* 4 x G x m */);
/* R: snp_fst (R/Fst.R:47-85), Weir & Cockerham's Fst from per-population allele frequencies.  af, N: r x m, population
 * p's vector (the `af` and `N` of bed_MAF) at p * m.  fst (m, may be NULL): a / (a + b + c) per variant, NaN where the
 * variant is not kept (p_bar outside (min_maf, 1 - min_maf), or NaN).  overall (3, may be NULL): sum a / sum (a + b + c)
 * over the kept variants, then the two sums; they are taken in a fixed order (blocks of 256 variants by a binary tree,
 * block sums in index order), so the result does not depend on the launch.  Errors, the reference's: "You should
 * provide frequencies for at least 2 populations.", "Parameter 'min_maf' should be in range [0, 0.45]." */
int bsn_fst(const double *af, const double *N, int64_t r, int64_t m, double min_maf, double *fst /* or NULL */,
            double *overall /* or NULL */);
/* the same from the genotypes: bsn_bed_group_counts, allele frequencies as bed_MAF forms them and the statistic, all on the
 * device; only fst / overall come back.  Bit-identical to bsn_fst on the frequencies of the same groups. */
int bsn_bed_fst(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int32_t *group /* [n] */, int32_t G,
                const int64_t *ind_col, int64_t m, double min_maf, double *fst /* or NULL */, double *overall /* or NULL */);
/* R: snp_MAX3 (R/MAX3.R:3-28,81-107).  y01[i]: 0 = control, 1 = case (anything else is an error).  score[j] = max over
 * x in val[0 .. L - 1] of Z_CATT(x)^2 with genotype scores (0, x, 1), from the counts of 0 / 1 / 2 among cases and
 * controls (missing genotypes are left out); a NaN statistic counts as 0.  val = (0, 0.5, 1): MAX3; (0.5): the Armitage
 * trend test. */
int bsn_snp_max3(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int32_t *y01 /* [n] */, const int64_t *ind_col,
                 int64_t m, const double *val, int32_t L, double *score /* [m] */);
/* device milliseconds (HIP events) of the last of the four calls above in this process: ms_out[0] the multiplicity and
 * digit panels, [1] the streaming launches, [2] the finalising kernels, [3] the statistic (0 for bsn_bed_group_counts).
 * One record per process, written without a lock, like bsn_impute_last_ms. */
int bsn_popstat_last_ms(double *ms_out /* 4 */);

/* ---- exact Hardy-Weinberg test and the QC filters (bed_hwe / bed_plinkQC; what snp_plinkQC asks of PLINK,
 * R/external-software.R:247-290) ----
 * The exact test of Wigginton, Cutler & Abecasis (2005) per variant, as csrc/hwe_step.hpp states it:
 * p_out[j] from counts[3 j .. 3 j + 2] = the homozygotes of one allele, the heterozygotes, the homozygotes of the other.
 * midp != 0: the mid-p variant.  No genotype: NaN; monomorphic: 1; a p-value below about 1e-300 may come back as 0.
 * Refused by name: a negative count, a variant with more than INT32_MAX genotypes, m < 1. */
int bsn_hwe(const int32_t *counts /* 3 x m: hom1, het, hom2 */, int64_t m, int midp, double *p_out /* [m] */);
/* the same with the kernel form chosen by the caller: lanes = 1 (one lane walks down and up), 2 (two adjacent lanes, one
 * walk each) or 0 (what bsn_hwe takes).  Every form returns the same bits.  ms_out (may be NULL): device ms of the kernel.
 * For tests and tools/probe_qc.py. */
int bsn_hwe_lanes(const int32_t *counts, int64_t m, int midp, int lanes, double *p_out, double *ms_out);
/* the test over the selected samples of a genotype handle: one counting pass (as bsn_bed_group_counts with one group;
 * out-of-core handles are served slab by slab), the counts stay on the device for the test.  counts_out (may be NULL):
 * the counts of 0, 1, 2 and missing, 4 x m.  Refused by name: a byte (dosage) image, more than INT32_MAX samples. */
int bsn_bed_hwe(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, int midp,
                double *p_out /* [m] */, int32_t *counts_out /* 4 x m or NULL */);
/* plink --mind --geno --maf --hwe in one call; nothing but the results leaves the device.  cls[i]: 0 = founder and counted
 * for the test, 1 = founder, not counted for the test, 2 = not a founder (counted for the missing rates only).
 *  1. sample i is removed when NA_i > mind * m over the selected variants; S1 is the rest;
 *  2. over S1, independently of each other, variant j is removed when NA_j > geno * |S1|, when the exact test over class 0
 *     gives p < hwe (skipped when hwe <= 0), or when its minor allele frequency over classes 0 and 1 is not >= maf (no call
 *     among them: NaN, removed whenever maf > 0).
 * keep_row [n], keep_col [m]: 1 = kept.  row_miss (n, may be NULL): NA_i / m.  col_stats (3 x m at 3 j, may be NULL): the
 * missing rate over S1, the minor allele frequency, p (computed for col_stats also when hwe <= 0).
 * Refused by name: a byte (dosage) image, an out-of-core handle, a threshold outside [0, 1], a class outside 0 .. 2, more
 * than INT32_MAX samples, every sample removed, no sample of class 0 while hwe > 0, none of class 0 or 1 while maf > 0. */
int bsn_bed_qc(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const int32_t *cls /* [n] */,
               double maf, double geno, double mind, double hwe, int midp, uint8_t *keep_row /* [n] */,
               uint8_t *keep_col /* [m] */, double *row_miss /* [n] or NULL */, double *col_stats /* 3 x m or NULL */);
/* device milliseconds (HIP events) of the last bsn_bed_hwe / bsn_bed_qc of this process: [0] the per-sample counts, [1] the
 * per-class counting pass, [2] the test kernel, [3] the masks.  One record per process, written without a lock. */
int bsn_qc_last_ms(double *ms_out /* 4 */);

/* ---- KING-robust kinship table (bed_king / bed_kingQC; what snp_plinkKINGQC asks of PLINK 2, R/external-software.R:520-590) ----
 * For every pair of positions i < j of ind_row, over the selected variants where both samples are called: NSNP, HETHET
 * (both heterozygous), IBS0 (opposite homozygotes), HET1HOM2 (i heterozygous, j homozygous), HET2HOM1 (the reverse) and
 *   KINSHIP = 0.5 - (double)(4 IBS0 + HET1HOM2 + HET2HOM1) / (4.0 * (double)(HETHET + min(HET1HOM2, HET2HOM1)))
 * (Manichaikul et al. 2010, between-family; one division and one subtraction in IEEE double: NaN for 0 / 0, -inf for a
 * zero denominator otherwise).  The counts are exact: seven int32 plane products over the sample-major copy of the image
 * on the int8 matrix pipe, two when every selected variant is known to hold no missing call (bsn_bed_na_known's record;
 * BSN_KING_GENERAL=1 forces the seven).  ind_row may be any list, repeats included; ind_col other than all variants in
 * file order is served from a gathered copy of the selection.
 * Two-phase like bsn_cormat: this call computes on the device and returns the number of rows; filter = 0 keeps every
 * pair (non-finite kinships included), otherwise the pairs with KINSHIP >= thr.  Rows ascend in (i, j); two calls return
 * the same bytes.  Refused by name: a byte (dosage) image, an out-of-core handle, no room for the sample-major operand
 * or for the table, n < 2, m < 1, m >= 2^29. */
typedef struct bsn_king bsn_king;
int bsn_bed_king(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, double thr, int filter,
                 int64_t *count, bsn_king **out);
/* i1, i2 [count] (positions in ind_row, 0-based), counts [5 x count] (row k at 5 k: NSNP, HETHET, IBS0, HET1HOM2,
 * HET2HOM1), kinship [count].  The bsn_bed of the call must still be open. */
int bsn_king_fetch(bsn_king *king, int32_t *i1, int32_t *i2, int32_t *counts, double *kinship);
int bsn_king_free(bsn_king *king);
/* device milliseconds (HIP events) of the last bsn_bed_king of this process: [0] the operand (gathered selection,
 * sample-major copy), [1] the per-sample totals of the two-product path (0 on the general path), [2] the pair kernel,
 * [3] the compaction.  One record per process, written without a lock. */
int bsn_king_last_ms(double *ms_out /* 4 */);

/* ---- method-of-moments IBD table (bed_ibd / bed_ibdQC; what snp_plinkIBDQC asks of PLINK 1.9's --genome) ----
 * For every pair of positions i < j of ind_row, over the selected variants where both samples are called: IBS0 (opposite
 * homozygotes), IBS1 (one heterozygous, the other homozygous), IBS2 (the rest), and the estimate of csrc/ibd_step.hpp
 * (DESIGN.md 3.5p): Z0, Z1, Z2 (PLINK's default, "bounded"), PI_HAT = Z1 / 2 + Z2 and DST = (IBS2 + IBS1 / 2) / S.  The
 * moments E00, E01, E02, E11, E12 are means over the variants with more than 3 called alleles and both alleles seen among
 * the frequency samples: the positions of ind_row where freq_mask is non-zero (NULL: all), summed in the fixed order of
 * the header.  A pair without a shared call is NaN in every double.  filter = 0: every pair; otherwise the pairs with
 * PI_HAT >= min_pi_hat (NaN passes nothing).  Rows ascend in (i, j); two calls return the same bytes.  The pair statistics
 * are those of bsn_bed_king (same kernel, operand and batches; BSN_KING_GENERAL keeps its meaning).
 * Refused by name: a byte (dosage) image, an out-of-core handle, n < 2, m < 1, m >= 2^29, no room for the sample-major
 * operand or for the table, min_pi_hat outside [0, 1], a frequency mask without a sample, no variant used for the moments. */
typedef struct bsn_ibd bsn_ibd;
int bsn_bed_ibd(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m,
                const uint8_t *freq_mask /* [n] or NULL */, double min_pi_hat, int filter, int64_t *count, bsn_ibd **out);
/* i1, i2 [count] (positions in ind_row, 0-based), ibs [3 x count] (row k at 3 k: IBS0, IBS1, IBS2), est [5 x count] (row k
 * at 5 k: Z0, Z1, Z2, PI_HAT, DST), E [5] and n_used (either may be NULL; filled for an empty table too).  The bsn_bed
 * of the call must still be open. */
int bsn_ibd_fetch(bsn_ibd *ibd, int32_t *i1, int32_t *i2, int32_t *ibs, double *est, double *E, int64_t *n_used);
int bsn_ibd_free(bsn_ibd *ibd);
/* device milliseconds (HIP events) of the last bsn_bed_ibd of this process: [0] .. [3] as bsn_king_last_ms, [4] the counting
 * pass of the frequency samples, [5] the moment kernels.  One record per process, written without a lock. */
int bsn_ibd_last_ms(double *ms_out /* 6 */);

/* _bigsnpr_prod_and_rowSumsSq (6 args) src/bed-fun.cpp:103-133 (the kernel of
 * bed_projectSelfPCA, R/bed-projectPCA.R:45-59): XV[n x K] = A~ V[m x K] and
 * rowSumsSq[i] = sum_j A~[i, j]^2, column-major host buffers. */
int bsn_bed_prod_and_rowsumssq(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                               int64_t m, const double *center, const double *scale, const double *V,
                               int64_t K, double *XV, double *rowSumsSq);

/* _bigsnpr_prod_and_rowSumsSq2 (6 args) src/project-utils.cpp:12-43: the same on an FBM.code256 handle;
 * rows that hold a missing code come back NaN (the FBM accessor yields NA_real there). */
int bsn_snp_prod_and_rowsumssq2(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                                int64_t m, const double *center, const double *scale, const double *V,
                                int64_t K, double *XV, double *rowSumsSq);

/* OADP_proj of R/bed-projectPCA.R:62-67 (bigutilsr::pca_OADP_proj2, external to the reference tree): the Online
 * Augmentation - Decomposition - Procrustes projection of n new samples from their simple projections XV[n x K], their
 * squared norms X_norm[n] and the K singular values sval of the reference PCA; out[n x K].  Column-major host buffers.
 * One group of lanes per sample, two one-sided Jacobi decompositions of order K + 1 and K in LDS (csrc/oadp_step.hpp).
 * 1 <= K <= 60; sval must be finite and positive (checked before any launch).  A row that holds a NaN or an infinity in
 * XV or X_norm comes back NaN. */
int bsn_pca_oadp_proj(const double *XV, const double *X_norm, const double *sval, int64_t n, int64_t K, double *out);

/* bed_projectPCA / bed_projectSelfPCA (R/bed-projectPCA.R:147-171, 214-226) in one call on a resident image: what
 * bsn_bed_prod_and_rowsumssq does, followed by the OADP kernel on the device buffers; XV[n x K], rowSumsSq[n] and
 * OADP[n x K] come back together.  A negative entry of scale is accepted: it is a variant whose alleles are reversed in
 * the target (centre' = (centre - 1) beta + 1, scale' = scale beta with beta = -1). */
int bsn_bed_project_pca(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m,
                        const double *center, const double *scale, const double *V, int64_t K, const double *sval,
                        double *XV, double *rowSumsSq, double *OADP);
/* device milliseconds (HIP events) of the last of the two calls above in this process: ms_out[0] the product and row-norm
 * passes (0 for bsn_pca_oadp_proj), [1] the OADP launch.  One record per process, written without a lock. */
int bsn_project_last_ms(double *ms_out /* 2 */);

/* ---- ancestry proportions from allele frequencies (ancestry.hip) ---------------------------------------------------------
 * snp_ancestry_summary (R/ancestry-summary.R:31-74; Privé 2022) for many frequency vectors at once, and for every sample of
 * a genotype image (frequency = genotype / 2).  quadprog::solve.QP and Matrix::nearPD, which the reference calls, are
 * external to its tree: parity with their numbers is not pinned; the rule is stated in csrc/qp_step.hpp and
 * pinned against a CPU statement compiled from that header.
 * The primitive: B problems   minimise 1/2 w'D w - d'w   s.t.  w >= 0,  sum w = 1 (sum_to_one) or sum w <= 1,   that share
 * D (K x K, column-major, symmetric positive definite), by the dual active-set method of Goldfarb & Idnani, one group of
 * lanes per problem.  dvec: K x B column-major; w_out: B x K column-major; steps_out [B]: active-set steps, -1: a NaN or an
 * infinity in d (a NaN row), -2: the step cap was reached (a NaN row; counted in n_failed).  Host buffers.  Refused with
 * a message before any launch: K < 1, K > 60 (bsn_qp_max_k), a D whose Cholesky factorisation fails. */
int bsn_qp_max_k(void);
int bsn_qp_simplex(const double *D, int64_t K, const double *dvec, int64_t B, int32_t sum_to_one, double *w_out,
                   int32_t *steps_out, int64_t *n_failed);
/* The moment pass over P (M x L), X0 (M x K) and F (M x B, B may be 0: F is not read), column-major with leading
 * dimensions >= M; on_device != 0: the three are device pointers (bsn_malloc), else host.  Host results, column-major and
 * compact, each may be NULL: PtX0 = P'X0 (L x K), PtF (L x B), G0 = X0'X0 (K x K), X0tF (K x B), the column sums csX0 [K]
 * and csF [B], the column sums of squares sqF [B].  fp64; rows in slabs of 4096 whose partial sums are added in ascending
 * order (the same bits in every run); BSN_ANC_SLABS=<s> forces the number of slabs.  1 <= K <= 60, 1 <= L <= 64. */
int bsn_ancestry_moments(const double *P, int64_t ldp, const double *X0, int64_t ldx, const double *F, int64_t ldf, int64_t M,
                         int64_t L, int64_t K, int64_t B, int32_t on_device, double *PtX0, double *PtF, double *G0,
                         double *X0tF, double *csX0, double *csF, double *sqF);
/* The moment pass, then one program per column of F: X = P'X0, y = (P'f) o correction [L], dvec = X'y, D = Dmat — which the
 * caller derives from X (Matrix::nearPD of X'X in the reference).  w, cor_each (cor(X0[, k], f)): B x K column-major;
 * cor_pred (cor(X0 w, f)) and steps: B.  Matrices as for bsn_ancestry_moments; everything else host. */
int bsn_ancestry_summary(const double *F, int64_t ldf, int64_t B, const double *X0, int64_t ldx, const double *P, int64_t ldp,
                         const double *correction, int64_t M, int64_t L, int64_t K, const double *Dmat, int32_t sum_to_one,
                         int32_t on_device, double *w, double *cor_each, double *cor_pred, int32_t *steps);
/* The same for the n selected samples of a resident 2-bit image, f = g / 2 over the m selected variants: X0 (m x K), P
 * (m x L), Xproj = P'X0 (L x K), compact host matrices.  One product pass A~ [P | X0 | c | 1] with centre 2 c and scale 2,
 * c_j = mean_k X0[j, k] (a missing genotype counts as c_j: a sample's result depends on its own row alone), the row sums of
 * squares, a moment pass over the tables, then the program kernel on the device buffers.  Results n x K / n as above.
 * A byte image (dosages) or a generic FBM.code256 handle is refused with a message. */
int bsn_bed_ancestry(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const double *X0,
                     const double *P, const double *correction, int64_t L, int64_t K, const double *Dmat, const double *Xproj,
                     int32_t sum_to_one, double *w, double *cor_each, double *cor_pred, int32_t *steps);
/* device milliseconds (HIP events) of the last of the four calls above in this process: [0] the genotype pass (product and
 * row norms), [1] the moment pass, [2] the program kernel.  One record per process, written without a lock. */
int bsn_ancestry_last_ms(double *ms_out /* 3 */);

/* The genotype-touching part of snp_grid_PRS (R/SCT.R:201-262), which in the
 * reference is one snp_PRS call (R/PRS.R:36-76 -> bigstatsr::big_prodVec) per clumping set:
 * scores for C column sets x T thresholds in a single sweep, one n x C GEMM per threshold bin.
 *   ind_col[m], betas[m]  the union of the C sets and its weights
 *   bin[m]                number of (ascending-sorted) thresholds that lpS[j] exceeds, 0..T
 *   member[m x C]         column-major 0/1: column j belongs to set c
 *   out[n x (C*T)]        column c*T + t = sum over j in set c with bin[j] > t of G[, j] betas[j],
 *                         accumulated from the highest threshold down as snp_PRS does
 * slices: fixed-point width of the weight panel (0 -> 7 = 56 bits). */
int bsn_snp_grid_prs(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m,
                     const double *betas, const int32_t *bin, const uint8_t *member, int64_t C, int64_t T,
                     int slices, double *out);

/* ---- .bed <-> FBM.code256 (the data formats either side of the path) ------
 * _bigsnpr_readbina2 (5 args) src/read-plink.cpp:61-80: decoded genotypes of the sub-matrix,
 * one byte each (0, 1, 2, 3 = missing), n x m column-major — the content of the .bk file that
 * snp_readBed / snp_readBed2 create (R/read-plink.R:27-111). */
int bsn_bed_to_fbm(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m,
                   uint8_t *out);
/* _bigsnpr_readbina (3 args) src/read-plink.cpp:13-56 (snp_readBed, R/read-plink.R:54): the WHOLE matrix of the
 * handle as FBM bytes, column-major n x m, every .bed byte decoded through the caller's 4 x 256 raw table
 * (tab[4 * byte + e] = FBM byte of genotype e of that byte; getCode(), R/utils.R:21-31).  The end-of-file flag
 * the reference returns is a property of the file, not of the payload: the R shim derives it from the file size. */
int bsn_bed_readbina(bsn_bed *bed, const uint8_t *tab, uint8_t *out);
/* _bigsnpr_writebina (5 args) src/write-plink.cpp:13-52: the .bed payload (ceil(n/4) bytes per
 * variant, pad bits 0, no magic header) of the sub-matrix [ind_row, ind_col] of the image;
 * snp_writeBed (R/write-plink.R:15-44) writes magic + this + .bim/.fam. */
int bsn_bed_subset_payload(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                           int64_t m, uint8_t *payload_out);

/* ---- device-resident operator (the fun.prod / fun.cprod seam of big_randomSVD,
 *      R/autoSVD.R:216-218, kept on the device so vectors never cross PCIe) ----- */
int bsn_op_create(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                  int64_t m, const double *center, const double *scale, bsn_op **out);
int bsn_op_destroy(bsn_op *op);
/* number of 8-bit slices the fp64 panels are split into (exact int8 MFMA arithmetic on
 * a fixed-point image of the vectors; 4 = 32-bit, 7 = 56-bit).  Default 4. */
int bsn_op_set_slices(bsn_op *op, int slices);
/* Y[n x nvec] = A~ X[m x nvec];  Z[m x nvec] = A~' X[n x nvec]; column-major, leading
 * dimensions ldx / ldy in elements; all pointers are DEVICE pointers */
int bsn_op_prod(bsn_op *op, const double *d_X, int64_t ldx, int nvec, double *d_Y, int64_t ldy);
int bsn_op_cprod(bsn_op *op, const double *d_X, int64_t ldx, int nvec, double *d_Z, int64_t ldz);
int bsn_op_sync(bsn_op *op);

/* ---- partial SVD (replaces bed_randomSVD -> bigstatsr::big_randomSVD -> RSpectra::svds,
 *      R/autoSVD.R:205-219; result fields of class "big_SVD": d, u, v, niter, nops) --------
 * Block Lanczos with full re-orthogonalisation on A~ A~' driven entirely on the device; basis
 * blocks are rounded to the fixed-point grid of the streaming products, which makes the products
 * exact, and the Ritz values come from the pair (Z'Z, Q'Q): d does not depend on `slices`.
 * `center`/`scale` are what fun.scaling returned (bed_scaleBinom, R/binom-scaling.R:133-142).
 * Multi-GPU: every rank calls this on its own column shard (ind_col local to its image),
 * passes m_total and an all-reduce hook that sums a device buffer of `count` doubles over
 * ranks in place (RCCL); u (n x k) is then identical on all ranks and v (m x k) is the
 * rank's own shard.  u / v may be NULL. */
typedef void (*bsn_allreduce_fn)(void *d_buf, int64_t count, void *ctx);

/* ---- multi-GPU: one process per GPU, variants (columns) sharded over the ranks -------------
 * north_star: "SNP columns shard naturally across the 8 GPUs of one node, with the SVD's panel
 * all-reduced over RCCL/xGMI".  A communicator wraps an RCCL (ncclComm_t) communicator created
 * on the CURRENT device; RCCL is loaded on first use (dlopen), single-GPU callers never need it.
 * Rank 0 calls bsn_comm_unique_id and hands the BSN_COMM_ID_BYTES bytes to the other ranks by
 * whatever means the host program has (MPI, a socket, a file); every rank then calls
 * bsn_comm_init (collective).  With `comm` set in bsn_svd_options, bsn_bed_randomsvd runs its
 * exchange inside the library: the n x b partial panel is reduce-scattered by sample blocks,
 * each rank orthogonalises its block of rows (small b x p coefficient all-reduces), and the
 * finished basis block is all-gathered for the next crossproduct pass — all on HIP streams the
 * library owns, the reduce-scatter overlapping the local Gram kernels.  There is no reference
 * counterpart: bigsnpr parallelises over OpenMP threads of one process (src/bed-prod-vec.cpp:29). */
#define BSN_COMM_ID_BYTES 128
typedef struct bsn_comm bsn_comm;
int bsn_comm_unique_id(uint8_t *id_out /* BSN_COMM_ID_BYTES */);
int bsn_comm_init(const uint8_t *id, int rank, int world, bsn_comm **out);
int bsn_comm_rank(const bsn_comm *comm);
int bsn_comm_world(const bsn_comm *comm);
/* sum of a device buffer of doubles over the ranks, in place, blocking (tests, host-side reductions) */
int bsn_comm_allreduce(bsn_comm *comm, double *d_buf, int64_t count);
/* ncclCommAbort: ends the collectives in flight on this communicator and makes every later call fail; the handle must
 * still be given to bsn_comm_destroy.  What the watchdog of a sharded solve calls (bsn_svd_options.exchange_timeout_ms);
 * exported for hosts that run their own. */
int bsn_comm_abort(bsn_comm *comm);
int bsn_comm_destroy(bsn_comm *comm);
typedef struct bsn_svd_options {
  int32_t k;          /* number of singular triplets (R default 10) */
  double tol;         /* relative residual on eigenvalues of A~A~' (R default 1e-4) */
  int32_t block;      /* vectors per pass, 1..16 (0 -> 16 / slices, at most 8: 8 at the default tol) */
  int32_t slices;     /* int8 slices of the fp64 panels, 1..7 (0 -> from tol and block: 2 at tol 1e-4
                         with block 8, 3 with block 5; the Ritz values do not depend on it) */
  int32_t max_basis;  /* cap on the Krylov basis (0 -> automatic) */
  uint32_t seed;      /* start block seed (0 -> 1) */
  int32_t verbose;
  int64_t m_total;    /* total number of columns over all ranks (0 -> m) */
  bsn_allreduce_fn allreduce; /* host-side hook summing a device buffer over ranks (tests); NULL otherwise */
  void *allreduce_ctx;
  int32_t hook_rank, hook_world; /* rank / number of ranks behind the hook (ignored with `comm`) */
  struct bsn_comm *comm; /* RCCL communicator of bsn_comm_init: the panel exchange then runs inside the
                            library on its own stream (NULL: one GPU, or the hook above) */
  /* binom_scaling = 1: fun.scaling is bed_scaleBinom (R/binom-scaling.R:133-142) evaluated INSIDE the
   * solve: the code counts ride along the first crossproduct pass (no separate statistics pass);
   * the `center` / `scale` arguments are ignored and the values used are written to center_out /
   * scale_out (length m each, may be NULL). */
  int32_t binom_scaling;
  double *center_out, *scale_out;
  /* warm start: power iterations of the random start block on the leading 1/16 of the variants before
   * the first full pass (each costs two streaming launches over that subset, 1/8 of a pass together).
   * 0 -> 2 (default since round 5; 1 before), n > 0 -> n, -1 -> none.  Matrices with fewer than 262 144 variants
   * (over all ranks) skip it. */
  int32_t warm_start;
  int32_t warm_denominator; /* the subset is the leading 1 / warm_denominator of the variants (0 -> 16) */
  /* A Krylov basis that fills up (max_basis) before the residuals meet tol is compressed to the k + block
   * best Ritz vectors and the iteration goes on (thick restart; RSpectra::svds behind the reference restarts
   * implicitly).  0 -> at most 100 restarts, n > 0 -> n, < 0 -> none: a full basis ends the solve with return
   * code 2. */
  int32_t max_restarts;
  /* Accuracy of the singular VECTORS (round 5).  The Ritz values do not see the rounding of the panels (exact-product
   * Rayleigh-Ritz), the vectors do: at `slices` digits every vector that converges early keeps a relative residual
   * of 1.2 * 2^(-8 slices) — 1.8e-5 at 16 bits, i.e. angles of 1e-4 .. 3e-4 to the true singular vectors, where the
   * reference's fp64 Lanczos leaves its leading vectors at 1e-7.  vec_floor is the residual floor wanted instead:
   * the early block steps (while the leading half of the k pairs is still far from converged) then run on wider
   * panels — 24 bits for the default — and the late ones, whose rounding enters a converged vector with the small
   * weight of its last components, stay narrow.  0 -> 1e-7 when `slices` is 0 (automatic; 2.5e-7 until round 5), none when the caller
   * fixed `slices`; > 0 -> that floor (digits up to 56 bits); < 0 -> none: every step at `slices` (round 4). */
  double vec_floor;
  /* Sharded solve (comm != NULL), round 5.  exchange_timing = 1: every collective of the solve is bracketed by HIP
   * events on the stream it runs on; bsn_svd_info.exchange_ms reports the sums.  exchange_timeout_ms > 0: a watchdog
   * thread aborts the communicator (ncclCommAbort) when the solve has not returned after that many milliseconds — a
   * collective that never completes (the first contact of the overlapped exchange with a real transport) then ends
   * the call with an error instead of hanging the process; the communicator is dead afterwards (destroy it, make a
   * new one, choose a more conservative exchange: BSN_NO_OVERLAP=1, BSN_NO_SEGMENTS=1 — bigsnpr_amd.comm.negotiate
   * does exactly that on a miniature solve).  0: the environment variable BSN_EXCHANGE_TIMEOUT_MS, else no watchdog. */
  int32_t exchange_timing;
  int32_t exchange_timeout_ms;
} bsn_svd_options;
typedef struct bsn_svd_info {
  int32_t niter;      /* block steps */
  int32_t nops;       /* streaming passes over the genotype image (A~ or A~' applications) */
  int32_t basis;      /* Krylov basis size at exit */
  int32_t converged;
  double max_rel_resid;
  double gpu_ms;      /* HIP-event time of the whole solve on the handle's stream */
  /* per-launch HIP-event time of the two streaming kernels inside this solve */
  double cprod_ms;    /* total over n_cprod launches of k_cprod (A~' panel) */
  double prod_ms;     /* total over n_prod launches of k_prod (A~ panel) */
  int32_t n_cprod, n_prod;
  int32_t block, slices; /* vectors per pass and int8 slices actually used */
  int32_t n_bad;      /* binom_scaling: variants with > 50 % missing values (src/bed-fun.cpp:40-41) */
  int32_t fused_stats;/* 1 if the scaling statistics rode along the first crossproduct pass */
  double cprod_stats_ms; /* the k_cprod launches that also counted the codes (not in cprod_ms) */
  int32_t n_cprod_stats;
  int32_t warm_launches; /* streaming launches of the warm start, each over warm_fraction of the variants
                            (they are counted in nops and in the kernel timings too) */
  double warm_fraction;
  double warm_ms;        /* HIP-event time of those launches (not in cprod_ms / prod_ms) */
  int32_t tiled;         /* 1 if the streaming kernels read the tiled second copy of the image (bsn_bed_tile); 2 if the
                            product passes read the sample-major second copy (two-block solves, round 4) */
  int32_t segmented_passes; /* sharded solve: product passes that ran in segments of sample blocks with their reduce-scatters
                            queued behind each segment (on a second stream unless BSN_NO_OVERLAP=1); round 4 */
  int32_t compact_gathers;  /* sharded solve: basis blocks all-gathered as the 16-bit integers they are rounded to (a quarter
                            of the fp64 volume, same values; BSN_NO_COMPACT_GATHER=1: fp64); round 4 */
  /* precision schedule (vec_floor): widest panels used, block steps that ran wider than `slices`, and the
   * streaming launches with THREE column blocks (48 digit columns: 16 vectors x 24 bits), timed apart from
   * cprod_ms / prod_ms */
  int32_t slices_max, wide_steps;
  double wide_cprod_ms, wide_prod_ms;
  int32_t n_wide_cprod, n_wide_prod;
  double lead_rel_resid;    /* residual estimate of the leading half of the k pairs at exit (max_rel_resid: all k) */
  /* sharded solve: how the product passes exchanged their panel — 0 no exchange, 1 whole pass + one reduce-scatter,
   * 2 segments of sample blocks on the solve's stream, 3 segments with the reduce-scatters on a second stream — and,
   * with exchange_timing, HIP-event time (ms) and number of its collectives by class: [0] reduce-scatter of the
   * panel / of its segments, [1] all-gather of a basis block or of u, [2] small all-reduces / all-gathers, [3] what
   * the solve's stream WAITED for the exchange stream (the part of the overlapped reduce-scatters left exposed) */
  int32_t exchange_mode;
  int32_t n_exchange[4];
  double exchange_ms[4];
  /* 1 when ind_col was not a contiguous range and the solve ran on a compacted copy of the selected variants (kept on
   * the handle, re-gathered in place by the next solve over another list: the rounds of bed_autoSVD); compact_ms =
   * host wall time of making / finding that copy inside this call (0.0x ms when the same list was solved before) */
  int32_t compacted;
  double compact_ms;
  /* 1 when the handle is out of core (bsn_bed_is_streamed): both passes of every block step walked the file in slabs
   * of variants through the resident slab image — PCIe-bound (the whole file per pass), same kernels, same arithmetic */
  int32_t out_of_core;
  /* share of the K-steps (1 024 genotypes each) of the two streaming products that hold NO missing code, sampled
   * once per image ([0] crossproduct, [1] product; 0 while not measured), and na_skip: bit 0 / bit 1 = the
   * crossproduct / the product passes of this solve ended on the kernels that issue the missing-value plane only
   * for steps that have one (used from a share of 0.30: nearly complete or batch-structured data; same integers) */
  double na_free_steps[2];
  int32_t na_skip;
  /* early Rayleigh-Ritz (one GPU, resident image, page-locked u / v; BSN_NO_EARLY_RITZ=1: off): [0] guesses "the solve
   * ends at this step" for which u and v were formed and sent to the host beside the step's product pass, [1] 1 if
   * the u / v returned came from one (the last step's), 0 if they were formed after the last pass.  A solve that is
   * repeated on 56-bit panels reports both attempts together in [0], as niter and nops do; [1] is the repeat's. */
  int32_t early_ritz[2];
} bsn_svd_info;
/* Returns 0 on success, 1 on error, and 2 when the solve ran to the end of its basis without all
 * k residuals meeting tol (outputs are filled with the best available triplets, bsn_last_error()
 * says how far they are; RSpectra warns in that case, so should the caller). */
int bsn_bed_randomsvd(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                      int64_t m, const double *center, const double *scale,
                      const bsn_svd_options *options, double *d, double *u, double *v,
                      bsn_svd_info *info);
/* Measurement hygiene: the names (as rocprofv3 prints them, without the argument list) of the streaming kernels the
 * last bsn_bed_randomsvd on this handle launched, one "kind=name" line per kind (cprod, prod, cprod_stats, warm).
 * bench.py matches them against profiles/pmc_traffic.json before it quotes that record's HBM traffic. */
int bsn_bed_streaming_kernels(bsn_bed *bed, char *buf, int64_t len);
/* ... and the name of the streaming kernel the last bsn_op_prod of an operator launched (empty before the first). */
int bsn_op_last_kernel(bsn_op *op, char *buf, int64_t len);
/* Streaming layout.  The passes of bsn_bed_randomsvd / bsn_bed_prodvec / bsn_bed_cprodvec over a 64-aligned
 * contiguous range of variants run faster (about 8 %) on a second copy of the 2-bit image stored in tiles of
 * 64 variants x 1024 samples (16 KB): every load of a wavefront then lands in one contiguous run instead of 16 -
 * 64 rows a whole variant apart.  bsn_bed_randomsvd builds the copy by itself when the device has the room
 * (image size + 24 GB free; set BSN_NO_TILED=1 to forbid it); this call builds it ahead of time for the
 * one-shot products.  *built = 1 if the copy exists afterwards.  It costs one extra pass (read + write) once,
 * doubles the HBM held by the handle, and is freed by bsn_bed_close.  Results are bit-identical. */
int bsn_bed_tile(bsn_bed *bed, int *built);
/* Sample-major layout (round 4).  A second copy of the 2-bit image with the VARIANTS contiguous (sample i at
 * i * pitch, four variants per byte): on it the product A~ X of 9 .. 16 vectors (two MFMA column blocks) contracts
 * over the contiguous index like the crossproduct does on the variant-major image, and runs as the crossproduct's
 * kernel shape (no byte transposes, 16 accumulator registers instead of 128).  bsn_bed_randomsvd builds it by itself
 * for a solve on 16-vector blocks when the device has the room (image size + 24 GB free; BSN_NO_SMAJ=1 forbids it);
 * this call builds it ahead of time for bsn_op_prod / bsn_bed_prod* on 9 .. 16 vectors.  One extra read + write pass
 * once, doubles the HBM held by the handle, freed by bsn_bed_close / bsn_bed_release_workspace.  Results are
 * bit-identical (same exact integer sums). */
int bsn_bed_sample_major(bsn_bed *bed, int *built);

/* The device workspace of a solve (Krylov basis, panels, quantised operands: about
 * 8 (n + m) (8 k + 4 block) bytes, 4 GB at 400K x 1M, k = 20) stays on the handle for the next
 * solve (snp_autoSVD runs up to six in a row); this frees it early, together with the streaming-layout copy
 * of the image (bsn_bed_tile) and the cached work buffers of the device.  bsn_bed_close frees it too. */
int bsn_bed_release_workspace(bsn_bed *bed);

/* bed_tcrossprodSelf (R/bed-tcrossprodSelf.R:21-52): K[n x n] = A~ A~'; center / scale of length m as
 * returned by fun.scaling.  block_size is the reference's RAM block (R/bed-tcrossprodSelf.R:40-49) and is
 * ignored: the genotypes are decoded inside the fp64-MFMA kernel, nothing dense is materialised.  K is
 * column-major and exactly symmetric (the upper triangle is computed, the lower one mirrored). */
int bsn_bed_tcrossprod(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                       int64_t m, const double *center, const double *scale, int64_t block_size,
                       double *K);

/* ---- windowed LD (replaces corMat, ld_scores, clumping_chr, bed_clumping_chr) -----------
 * The handle may come from bsn_bed_open (.bed) or bsn_bed_from_fbm (FBM.code256 with NA),
 * which is the dispatch of src/corr.cpp:113-125.  `pos` has length m and must be sorted;
 * `size` is already in position units (R multiplies by 1000, R/corr.R:29).  A row list with repeated
 * samples is served from a gathered copy of the selected sub-matrix. */
typedef struct bsn_cor bsn_cor;
/* _bigsnpr_corMat (8 args) src/corr.cpp:102-126.  Two-phase: this call computes everything
 * on the device, fills p_out[m+1] (CSC column pointers exactly as R/corr.R:43-47 builds
 * them) and *nnz_out; bsn_cormat_fetch copies @i (ascending row index, diagonal last in each
 * column) and @x; thr has length n (thr[nona-1], src/corr.cpp:82). */
int bsn_cormat(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m,
               double size, const double *thr, const double *pos, int fill_diag, int32_t *p_out,
               int64_t *nnz_out, bsn_cor **out);
int bsn_cormat_fetch(bsn_cor *cor, int32_t *i_out, double *x_out);
/* *out = 1 when a stored correlation is NaN (a variant without variation among the selected samples): what
 * R/corr.R:53-54 finds with anyNA(corr@x), here noted by the kernel that writes @x instead of a pass over the
 * 12 bytes per pair on the host. */
int bsn_cormat_has_nan(const bsn_cor *cor, int *out);
int bsn_cormat_free(bsn_cor *cor);
/* measurement hook (bench.py --workload ld): figures of the last bsn_cormat / bsn_ld_scores /
 * bsn_clumping_* call of this process: out[0] = variant pairs in the band, out[1] = 64 x 64 tile
 * pairs, out[2] = total HIP-event time (ms) of the pair-statistics launches, out[3] = launches,
 * out[4] = kernel (0: six products, fused epilogue; 1: six products, K split; 2: cross product only) */
int bsn_ld_last_stats(double *out /* 5 */);
/* _bigsnpr_ld_scores (6 args) src/ld-scores.cpp:83-105 */
int bsn_ld_scores(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m,
                  double size, const double *pos, double *out);
/* _bigsnpr_clumping_chr (12 args) src/clumping.cpp:10-91 (mode 0: aux1 = sumX, aux2 = denoX)
 * and _bigsnpr_bed_clumping_chr (12 args) src/clumping-bed.cpp:11-91 (mode 1: aux1 = center,
 * aux2 = scale).  ordInd / rankInd are 0-based; keep[m] receives 0 / 1 (the reference's
 * `keep` FBM, R/clumping.R:116). */
int bsn_clumping_chr(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                     int64_t m, int mode, const double *aux1, const double *aux2,
                     const int32_t *ordInd, const int32_t *rankInd, const double *pos, double size,
                     double thr, int32_t *keep);
/* _bigsnpr_clumping_chr_cached (14 args) src/clumping-cached.cpp:11-107 as driven by the grid
 * loops of snp_grid_clumping (R/SCT.R:100-131): the same greedy clumping for
 * n_grid (size, thr) pairs over one column set.  The reference threads a sparse r2 cache through
 * the calls; here the r2 band is computed once at the largest window and every grid point sweeps
 * it.  keep[g * m + j] receives 0 / 1 for grid point g. */
int bsn_clumping_chr_cached(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col,
                            int64_t m, int mode, const double *aux1, const double *aux2,
                            const int32_t *ordInd, const int32_t *rankInd, const double *pos,
                            int64_t n_grid, const double *sizes, const double *thrs, int32_t *keep);

/* ---- robust statistics of the outlier step of snp_autoSVD / bed_autoSVD (round 5) ----------------------------------
 * R/autoSVD.R:142-148,295-301: bigutilsr::dist_ogk(obj.svd$v) — the orthogonalised Gnanadesikan-Kettenring estimator
 * (Maronna & Zamar 2002; robustbase::covOGK with scaleTau2) — needs, per round, p + p (p - 1) robust scales of vectors as
 * long as the number of variants: two medians and two weighted sums each, the bulk of the function's wall time once its
 * solves run on the GPU.  These entry points compute them for whole batches of columns of a DEVICE matrix (column-major,
 * leading dimension ld >= m; bsn_malloc / bsn_memcpy_h2d): medians by radix select, sums in a fixed order.  The loop
 * around them (p x p eigen-decompositions, hard rejection, Mahalanobis distances) is host code (bigsnpr_amd/autosvd.py,
 * an R shim would keep bigutilsr's own).  Small host vectors in and out. */
/* robustbase::scaleTau2(x, c1, c2, mu.too = TRUE, consistency = TRUE) of every column: mu_out / s_out [ncol] (either may be NULL) */
int bsn_robust_scale_tau2(const double *d_X, int64_t m, int64_t ld, int32_t ncol, double c1, double c2, double *mu_out, double *s_out);
/* the medians those scales start from, on their own: median of every column (centre NULL) or of |x - centre[c]| (the MAD
 * step), both middle order statistics averaged for an even m.  centre: host [ncol] or NULL; med_out: host [ncol] */
int bsn_robust_medians(const double *d_X, int64_t m, int64_t ld, int32_t ncol, const double *centre, double *med_out);
/* the same scale of Z_i + Z_j and Z_i - Z_j for every pair i > j of the p <= 64 columns, pairs in the order
 * (1,0), (2,0), (2,1), (3,0) ...: s_sum_out / s_diff_out [p (p - 1) / 2] */
int bsn_robust_pair_scales(const double *d_Z, int64_t m, int64_t ld, int32_t p, double c1, double c2, double *s_sum_out, double *s_diff_out);
/* medcouple of tukey_mc_up (Brys, Hubert & Struyf 2004): number of pairs (u, l), u from d_up [nu], l from the ASCENDING
 * d_lo [nl] (both positive distances to the median), with (u - l) / (u + l) <= t, -1 < t < 1 — the count the bisection
 * on t evaluates ~50 times per call */
int bsn_robust_mc_count(const double *d_up, int64_t nu, const double *d_lo, int64_t nl, double t, int64_t *count_out);
int bsn_robust_scale_cols(double *d_Z, int64_t m, int64_t ld, int32_t p, const double *div /* [p] */);      /* Z[, j] /= div[j] */
int bsn_robust_rotate(double *d_Z, int64_t m, int64_t ld, int32_t p, const double *E /* p x p, column-major */); /* Z <- Z E */
/* out[i] = sum_j ((Z[i, j] - mu[j]) / sig[j])^2, to the host */
int bsn_robust_wdist(const double *d_Z, int64_t m, int64_t ld, int32_t p, const double *mu, const double *sig, double *out);
/* (round 6) bigutilsr::dist_ogk end to end: squared robust Mahalanobis distances of the m rows of the DEVICE matrix d_U
 * (m x p, p <= 64, not modified) to the host vector dist_out [m] — the OGK rounds above (niter of them), the hard
 * rejection wdist <= median(wdist) * cut_ratio (cut_ratio = qchisq(beta, p) / qchisq(0.5, p), the caller's quantiles),
 * centre and covariance (denominator n_kept - 1) of the kept rows, distances with the pseudo-inverse of that covariance
 * (singular values <= 1e-15 x the largest dropped).  Only p x p matrices visit the host.  n_kept_out may be NULL.
 * R/autoSVD.R:142,295 (`bigutilsr::dist_ogk(obj.svd$v)`) */
int bsn_robust_dist_ogk(const double *d_U, int64_t m, int64_t ld, int32_t p, int32_t niter, double cut_ratio, double c1, double c2,
                        double *dist_out, int64_t *n_kept_out);
/* bigutilsr::rollmean of the HOST vector x [m] with the odd-length weight vector w [len] inside each of the consecutive
 * groups [group_off[g], group_off[g + 1]) (NULL / 0: one group); edge windows are renormalised by the weights they
 * contain.  R/autoSVD.R:143-144,296-297 (per chromosome) */
int bsn_robust_rollmean(const double *x, int64_t m, const double *w, int32_t len, const int64_t *group_off, int32_t ngroups, double *out);
/* ascending sort of a HOST vector of finite doubles in place (device radix sort): the order statistics of tukey_mc_up */
int bsn_robust_sort(double *x, int64_t m);
/* medcouple, the end of the bisection: the kernel values (u - l) / (u + l) in (a, b], -1 < a < b < 1, of the pairs counted
 * by bsn_robust_mc_count, to the host in no particular order; count_out receives their number and nothing is written when
 * it exceeds cap */
int bsn_robust_mc_window(const double *d_up, int64_t nu, const double *d_lo, int64_t nl, double a, double b, int64_t cap, double *out,
                         int64_t *count_out);

/* ---- exact k nearest neighbours and the outlier-sample statistics over them (knn.hip) --------------------------------
 * The outlier-sample step of the reference's PCA workflow (vignettes/bedpca.Rmd: bigutilsr::prob_dist(obj.svd$u), then
 * dist.self / sqrt(dist.nn)), and bigutilsr::knn_parallel / LOF.  bigutilsr is external to the reference tree: parity with
 * its numbers is not pinned; the rule is stated in csrc/knn_step.hpp and pinned against a CPU statement
 * compiled from that header.  All pairs in fp64: squared distance acc = fma(t, t, acc), t = q[d] - x[d], d ascending;
 * candidates ordered by (squared distance, 0-based index of the data point); the k smallest in that order.
 * DEVICE matrices, column-major with a leading dimension (bsn_malloc / bsn_memcpy_h2d), not modified; host vectors out.
 * Refused by name: p or k outside 1 .. 64, k above the number of candidates, 2^31 points or more, a non-finite coordinate,
 * no room for the workspace.  BSN_KNN_SLABS=<s> forces the number of slabs of data points (same bits for every s). */
/* d_data: n x p; d_query: nq x p, or NULL — self mode: the data is its own query (nq, ldq ignored) and the candidate with
 * the query's own index is left out, by index (other rows equal to the query stay in, at distance 0).
 * idx_out (int32, 0-based) / dist_out (the correctly rounded square root): nq x k, column-major */
int bsn_knn(const double *d_data, int64_t n, int64_t ld, const double *d_query /* NULL: self mode */, int64_t nq, int64_t ldq,
            int32_t p, int32_t k, int32_t *idx_out, double *dist_out);
/* over the self-mode table with k = kNN: m2[i] = mean of the squared distances of i's neighbours; dist_self_out [n] =
 * sqrt(m2); dist_nn_out [n] = mean of m2 over i's neighbours */
int bsn_prob_dist(const double *d_U, int64_t n, int64_t ld, int32_t p, int32_t kNN, double *dist_self_out, double *dist_nn_out);
/* local outlier factors (Breunig et al. 2000) for every kk of seq_k [nk] over the self-mode table with k = max(seq_k):
 * lof_out n x nk, column-major.  Duplicated rows give inf and NaN as IEEE has them */
int bsn_lof(const double *d_U, int64_t n, int64_t ld, int32_t p, const int32_t *seq_k, int32_t nk, double *lof_out);
/* the last of the three calls above in this process: device ms of the packing pass, the scan, the merge, what follows the
 * table (square roots, statistics); then the slab count and the queries per workgroup it ran with */
int bsn_knn_last_stats(double *out /* 6 */);

/* R/clumping.R:106, R/bed-clumping.R:48 — `ord <- order(S.chr, decreasing = TRUE)` — for every chromosome at once: S [m]
 * holds the statistics of the groups [group_off[g], group_off[g + 1]) one after the other (NULL / 0: one group); ord
 * receives, group by group, the 0-based positions INSIDE the group in decreasing order of S, ties in index order (R's
 * order is stable), rank its inverse (rank[group_off[g] + ord[group_off[g] + t]] = t): the ordInd / rankInd arguments of
 * bsn_clumping_chr.  Two stable device radix sorts (by value, then by group); a NaN is refused (the host path puts
 * them last, as R does). */
int bsn_order_decreasing(const double *S, int64_t m, const int64_t *group_off, int32_t ngroups, int32_t *ord, int32_t *rank);

/* ---- sparse LD matrix in HBM and lassosum2 over it --------------------------------------------------------------------
 * bigsparser's SFBM as R/lassosum2.R receives it (`corr`): full columns of a sparse symmetric LD matrix, held on the
 * device and reused across calls.  From a CSC with p [m2 + 1] (0-based offsets), rows i [p[m2]] strictly ascending in
 * each column, values x [p[m2]]: upper = 1 reads the upper triangle with the diagonal (the @i / @p / @x of bsn_cormat_fetch,
 * uplo = "U") and expands it to full columns on the device; upper = 0 reads full columns (a dgCMatrix).  Bad p, rows out
 * of range or unsorted rows are refused before any device work. */
typedef struct bsn_sfbm bsn_sfbm;
int bsn_sfbm_from_csc(const int64_t *p, const int32_t *i, const double *x, int64_t m2, int upper, bsn_sfbm **out);
/* columns, stored entries of the full columns and bandwidth (max |row - column| over stored entries); any may be NULL */
int bsn_sfbm_ncol(const bsn_sfbm *s, int64_t *m2_out, int64_t *nnz_out, int64_t *bandwidth_out);
int bsn_sfbm_free(bsn_sfbm *s);
/* _bigsnpr_lassosum2 (8 args) src/lassosum2.cpp:8-70, for G grid points per call instead of one.  Grid point g uses
 * lambda_j = pf[j] * lambda[g] and delta_plus_one_j = pf[j] * delta[g] + 1 (R/lassosum2.R:59-60, formed on the device);
 * ind_sub [m] (0-based columns of `corr`, any order, NULL: 0 .. m2 - 1 with m = m2).  beta_out [m * G] is column-major,
 * one column per grid point in the caller's order, NaN where the reference returns NA (gap > gap0); num_iter_out [G]
 * is the reference's k + 1; time_out [G] (may be NULL) the seconds of each grid point on the device clock.  Every
 * result equals the sequential loop bit for bit. */
int bsn_lassosum2(const bsn_sfbm *s, const double *beta_hat, int64_t m, const double *pf, const double *lambda,
                  const double *delta, int64_t G, const int64_t *ind_sub, double dfmax, int32_t maxiter, double tol,
                  double *beta_out, int32_t *num_iter_out, double *time_out);
/* LDpred2-grid's Gibbs sampler: ldpred2_gibbs_one (src/ldpred2.cpp:9-69) for G chains per call, and
 * ldpred2_gibbs_one_sampling (src/ldpred2-sampling.cpp:9-59) for one.  Chain g uses h2[g], p[g] (0 < p <= 1), sparse[g]
 * and the random numbers of stream[g] (NULL: g): U and Z of sweep k, position j come from a counter-based generator
 * keyed by `seed` at the counter (j, k + burn_in, stream[g]) and from nothing else, so a chain's result depends on
 * neither its place in the call nor the other chains.  ind_sub [m] as above, without repeats.  beta_out [m * G] is
 * column-major, avg_beta / num_iter, all NaN where the reference returns NA (gap > gap0 after a sweep); sample_out
 * [m * num_iter] holds curr_beta after each sweep past burn-in.  seconds_out (may be NULL): each chain's seconds on the
 * device clock.  Every floating-point operation is the reference's, in its order; only the generator differs from R's.
 * Arguments are checked before any device work. */
int bsn_ldpred2_gibbs(const bsn_sfbm *s, const double *beta_hat, const double *n_vec, int64_t m, const int64_t *ind_sub,
                      const double *h2, const double *p, const int32_t *sparse, const uint64_t *stream, int64_t G, int burn_in,
                      int num_iter, uint64_t seed, double *beta_out, double *seconds_out);
int bsn_ldpred2_gibbs_sampling(const bsn_sfbm *s, const double *beta_hat, const double *n_vec, int64_t m, const int64_t *ind_sub,
                               double h2, double p, int32_t sparse, uint64_t stream, int burn_in, int num_iter, uint64_t seed,
                               double *sample_out, double *seconds_out);
/* LDpred2-auto: ldpred2_gibbs_auto (src/ldpred2-auto.cpp:57-202) for G chains per call, chain g from p_init[g] and the
 * random numbers of stream[g] (NULL: g).  log_var [m] is 2 log(sd) (read with use_mle only); alpha_lo / alpha_hi bound
 * alpha + 1, as the reference passes them; mean_ld is the mean LD score over ind_sub.  The coordinate draws are those of
 * bsn_ldpred2_gibbs at the counter (j, k, stream[g]), k counting from the first burn-in sweep; the draws of a sweep's
 * epilogue (the two gammas of rbeta, the bootstrap of the causal set) carry a purpose tag in the two top bits of the
 * sweep word, hence burn_in + num_iter < 2^30.  The bounded MLE of (alpha + 1, sigma2) is the exact minimiser over the
 * reference's box, found by bisection on the profile's derivative with sums of one fixed order, in the place of the
 * reference's L-BFGS-B run.  Outputs are column-major per chain: beta_est, postp_est, corr_est [m * G] (averages over
 * num_iter, all NaN where the reference returns NA); sample_beta [m * n_report * G] with n_report = num_iter / report_step
 * (may be NULL when that is 0), the causal entries of curr_beta after sweep burn_in + c * report_step - 1; path_p,
 * path_h2, path_alpha [(burn_in + num_iter) * G], NaN from the sweep on at which a chain diverged (path_alpha all NaN
 * without use_mle).  seconds_out (may be NULL): each chain's seconds on the device clock.  Every result equals the
 * sequential loop over the same arithmetic bit for bit.  Arguments are checked before any device work. */
int bsn_ldpred2_auto(const bsn_sfbm *s, const double *beta_hat, const double *n_vec, const double *log_var, int64_t m,
                     const int64_t *ind_sub, const double *p_init, const uint64_t *stream, int64_t G, double h2_init,
                     int burn_in, int num_iter, int report_step, int no_jump_sign, double shrink_corr, int use_mle,
                     double p_lo, double p_hi, double alpha_lo, double alpha_hi, double mean_ld, uint64_t seed,
                     double *beta_est, double *postp_est, double *corr_est, double *sample_beta,
                     double *path_p, double *path_h2, double *path_alpha, double *seconds_out);

/* ---- products with the resident matrix: bigsparser's sp_prodVec and sp_solve_sym, ld_scores_sfbm ------------------------
 * ind_sub [m] (0-based columns of `corr`, any order; NULL: all of them, m = m2) means "as if run on corr[ind_sub, ind_sub]".
 * Every sum has a fixed order that depends on the shapes only: two calls on the same inputs return the same bits.
 *
 * bsn_sfbm_prodvec: y_out [m] = corr[ind_sub, ind_sub] . x [m] (sp_prodVec; sp_cprodVec is the same call, the matrix is
 * symmetric).  A repeated index is refused before any device work. */
int bsn_sfbm_prodvec(bsn_sfbm *s, const double *x, const int64_t *ind_sub, int64_t m, double *y_out);
/* src/ld-scores-sfbm.cpp:10-69: out [j] = sum of x^2 over the stored entries of column ind_sub[j] whose row is in ind_sub
 * (a mask: repeated indices are allowed and give repeated values). */
int bsn_sfbm_ld_scores(bsn_sfbm *s, const int64_t *ind_sub, int64_t m, double *out);
/* Solves (corr[ind_sub, ind_sub] + diag(add_to_diag)) x = b by MINRES (Paige & Saunders), the iteration on the device.
 * Stops when the recurrence's residual norm is <= tol * ||b||, then forms the TRUE residual ||b - (A + D) x|| / ||b|| with
 * one more product (relres_out) and goes on, from that residual, while it exceeds tol.  After maxiter iterations without
 * that the call returns an error whose message names the iterations and the residual reached; x_out [m], iters_out and
 * relres_out (either may be NULL) are filled in that case too.  A repeated index is refused before any device work. */
int bsn_sfbm_solve_sym(bsn_sfbm *s, const double *b, const double *add_to_diag, const int64_t *ind_sub, int64_t m, double tol,
                       int32_t maxiter, double *x_out, int32_t *iters_out, double *relres_out);
/* device milliseconds (HIP events, host copies excluded) of the last of the three calls above on this handle */
int bsn_sfbm_last_ms(const bsn_sfbm *s, double *ms_out);

/* ---- snp_ldsplit (R/split-LD.R, src/split-LD.cpp): optimal LD block splitting over the resident matrix -------------------
 * Works on the lower triangle of `corr`, whose every column must store a non-zero diagonal.  thr_r2: squared correlations
 * below it are ignored; max_r2: no pair above it may be split; block sizes min_size .. max_size; K = 1 .. max_K blocks;
 * max_cost (may be +Inf) as get_C takes it, the caller clamps; pos_scaled [m] ascending (NULL: all 0).
 * Outputs, any may be NULL: C_out [m * max_K] column-major, the reference's C (+Inf where no split exists);
 * best_ind_out [m * max_K], the reference's best_ind: the 0-based first row of the next block, -1 for NA;
 * cost_out [max_K] = C(0, K - 1); n_block_ok_out [max_K]: 1 where K blocks were reconstructed (cost <= max_cost and a
 * path exists); cost2_out [max_K] the sum of squared block sizes (+Inf where not reconstructed); perc_kept_out [max_K]
 * get_perc (-1 where not reconstructed); all_last_out [max_K * max_K], K entries from (K - 1) * max_K on: best_ind along
 * the path, the rest -1; levels_run_out: the levels computed before the reference's early stop; seconds_out [3]: device
 * seconds of E (with the suffix sums), of the levels and of the epilogue.  Every result equals the reference's sequential
 * loops bit for bit.  min_size < 1, max_size < min_size, max_size > m, max_K < 1, a pos_scaled that is not ascending and
 * a column without a non-zero diagonal are refused by name, and the tables must fit the free device memory. */
int bsn_sfbm_ldsplit(const bsn_sfbm *s, double thr_r2, double max_r2, int32_t min_size, int32_t max_size, int32_t max_K,
                     double max_cost, const double *pos_scaled, double *C_out, int32_t *best_ind_out, double *cost_out,
                     double *cost2_out, double *perc_kept_out, int32_t *n_block_ok_out, int32_t *all_last_out,
                     int32_t *levels_run_out, double *seconds_out);

/* ---- scoring a grid of models: big_prodMat, AUC, AUCBoot, pcor (bigsnpr_amd/csrc/auc.hip, the rule in auc_step.hpp) ---------
 * Score matrices are column-major, fp64 (is_f32 = 0) or fp32 (is_f32 != 0), in host memory (on_device = 0) or in device memory
 * of the caller (bsn_malloc, or the d_XV of bsn_bed_prodmat); `ld` is the leading dimension in elements.  Null stream,
 * synchronised before returning.  BSN_AUC_BATCH=<n> allows at most n columns per sort batch and n replicates per bootstrap
 * launch; every n gives the same bits. */
/* bigstatsr::big_prodMat on a genotype image: XV (n x K) = A~[ind_row, ind_col] A, through the product pass of
 * bsn_bed_prod_and_rowsumssq.  center / scale: both NULL or both m values.  XV (host) and d_XV (device, n x K, leading dimension
 * n) may each be NULL, not both.  A column of A that holds a NaN comes back as a column of NaN. */
int bsn_bed_prodmat(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, const double *center,
                    const double *scale, const double *A, int64_t K, double *XV, double *d_XV);
/* AUC of K score columns against one 0 / 1 target (n values, one per selected row): twoU = 2 #{case > control} + #{case = control}
 * in exact integers, auc_out[j] = twoU / (2 n1 n0).  `pred` has n_src rows and K * n_sum columns; result column j is the fp64 sum,
 * ascending, of the columns j, j + K, ..., j + (n_sum - 1) K (n_sum = 1: the column itself; n_sum = chromosomes: snp_grid_AUC).
 * ind_row: NULL (n = n_src) or n row indices.  Refused by name: a NaN (the message names the first such column), a target value
 * other than 0 / 1, one class only, 2^31 rows or more, no room for one column's workspace. */
int bsn_auc(const void *pred, int32_t is_f32, int32_t on_device, int64_t ld, int64_t n_src, int64_t K, int64_t n_sum,
            const int64_t *ind_row, int64_t n, const uint8_t *target, double *auc_out);
/* nboot bootstrap replicates of the AUC of each of K columns (replicates_out: nboot x K, column-major).  Replicate b draws n rows
 * by the rule of auc_step.hpp from (b, seed) alone: every column sees the same resamples.  A replicate without a case or without
 * a control is NaN. */
int bsn_auc_boot(const void *pred, int32_t is_f32, int32_t on_device, int64_t ld, int64_t n, int64_t K, const uint8_t *target,
                 int64_t nboot, uint64_t seed, double *replicates_out);
/* FOR TESTS: the n rows that replicate b draws, generated on the device */
int bsn_auc_boot_draws(int64_t n, int64_t b, uint64_t seed, int32_t *rows_out);
/* pcor's device part: for every column x of the score matrix, with Q (n x p, p <= 31, host, orthonormal columns) and r_y (n, host),
 * e = x - Q Q'x, ee_out = e'e, ery_out = e'r_y.  Two passes over fixed row slabs, no atomics: the same bits in every run. */
int bsn_pcor_moments(const void *x, int32_t is_f32, int32_t on_device, int64_t ld, int64_t n, int64_t K, const double *Q, int64_t p,
                     const double *ry, double *ee_out, double *ery_out);
/* device milliseconds of the last call above in this process: key pass, sort, group + evaluation kernels, bootstrap kernel, pcor */
int bsn_auc_last_ms(double *ms_out);

/* ---- the panel kernels of bsn_bed_randomsvd one at a time: FOR TESTS, not part of the drop-in surface ----------------------
 * The tall-skinny fp64 algebra between the streaming passes of a solve (bigsnpr_amd/csrc/svd.hip), through the launch
 * functions the solve itself uses, on DEVICE matrices of the caller (column-major; bsn_malloc / bsn_memcpy_h2d /
 * bsn_memcpy_d2h).  Null stream, synchronised before returning.  Every entry checks its arguments before the first launch and
 * refuses by name: null pointers, 1 <= cb <= 32 for bsn_panel_gemm_tn and cb, r, nc <= 16 elsewhere, cb * r <= 256, leading
 * dimensions below the row count.  No stability is promised for these names. */
/* C (p x cb, leading dimension ldc) = A[:, :p]' B[:, :cb] over `rows` rows: k_gemm_tn<1|2> + k_gemm_tn_reduce */
int bsn_panel_gemm_tn(const double *d_A, int64_t lda, int32_t p, const double *d_B, int64_t ldb, int32_t cb, int64_t rows,
                      double *d_C, int32_t ldc);
/* Out[:, :nc] = alpha In[:, :nc] + beta Q[:, :p] S (p x nc, leading dimension p); In may be NULL when alpha == 0 and may be Out */
int bsn_panel_gemm_nn(const double *d_Q, int64_t ldq, int32_t p, const double *d_S, int32_t nc, const double *d_In, int64_t ldi,
                      double alpha, double beta, double *d_Out, int64_t ldo, int64_t n);
/* in place W[:, :r] = W[:, :cb] M (cb x r, leading dimension cb) */
int bsn_panel_right_mult(double *d_W, int64_t ld, int64_t n, int32_t cb, int32_t r, const double *d_M);
/* in place W <- (W - Q[:, :p] C) Ri: k_update<8|16>.  C p x cb (leading dimension p), Ri cb x cb; d_mx: 16 x uint64 or NULL, the
 * bit patterns of the column maxima of |W| are folded into its first cb entries by atomic max */
int bsn_panel_update(const double *d_Q, int64_t ldq, int32_t p, const double *d_C, const double *d_Ri, int32_t cb, double *d_W,
                     int64_t ldw, int64_t n, uint64_t *d_mx);
/* rounding of the columns of X to the 8 * slices bit grid of the streaming products.  have_mx = 0: d_mx [16] is cleared and filled
 * by k_col_absmax first, with 256 (wide_grid != 0) or 64 workgroups per column; have_mx != 0: d_mx is taken as it is */
int bsn_panel_round_cols(double *d_X, int64_t ld, int64_t rows, int32_t cb, int32_t slices, int32_t have_mx, uint64_t *d_mx,
                         int32_t wide_grid);
/* the device queue of the fused block step on d_QW (nr x (p + cb), the panel W behind the basis Q, leading dimension nr): both
 * passes of gemm_tn -> k_orth2 -> k_update, with p > 0 the [Q W]'[Qb W] product of pass 0 (Qb = columns p0 = p - cb .. p - 1),
 * no host round trip in between.  W is replaced in place; flag_out [1] and Rout_out [cb * cb] go to the host.  Returns -1 (and does
 * nothing) where the solve takes the step-by-step path: cb > 16 or p + cb > 384. */
int bsn_panel_fused_orth(double *d_QW, int64_t nr, int32_t p, int32_t p0, int32_t cb, int32_t iters, double *flag_out,
                         double *Rout_out);
/* what the sharded solve's rounding of a finished block does, on one device and without a communicator: `world` sample blocks of
 * nr = ceil(n / world) rounded up to a multiple of 4 rows, k_take_rows + k_col_absmax per block, k_max_over_ranks,
 * k_pack_int<int16 (slices <= 2) | int32> per block, k_unpack_int into d_out (n x cb, leading dimension n).  d_full: n x cb, ld n */
int bsn_panel_compact_gather(const double *d_full, int64_t n, int32_t cb, int32_t world, int32_t slices, double *d_out);
/* k_block of d_full (n x cb, ld n) into the same sample blocks, k_unblock into d_out (n x cb) and k_place_rows of every block into
 * d_placed (world * nr rows, leading dimension world * nr) */
int bsn_panel_block_roundtrip(const double *d_full, int64_t n, int32_t cb, int32_t world, double *d_out, double *d_placed);

/* ---- device memory + timing helpers for hosts without a HIP binding -------- */
int bsn_malloc(void **d_ptr, int64_t bytes);
int bsn_free(void *d_ptr);
/* Page-locked host memory.  Every entry point accepts ordinary (pageable) caller memory and stages it
 * through pinned buffers of its own; a result buffer obtained here is written by the DMA engines directly
 * (bsn_bed_randomsvd: u and v, 224 MB at 400K x 1M, k = 20 — no staging copy, no first-touch page faults).
 * The reference returns freshly allocated R vectors (R/autoSVD.R:216-218); an R shim has to copy into
 * those, a host that controls its allocations (the Python mirror) does not. */
int bsn_host_alloc(void **h_ptr, int64_t bytes);
int bsn_host_free(void *h_ptr);
int bsn_memcpy_h2d(void *d_dst, const void *src, int64_t bytes);
int bsn_memcpy_d2h(void *dst, const void *d_src, int64_t bytes);
int bsn_device_sync(void);
/* HIP events on the handle's stream (bench.py roofline timing) */
int bsn_timer_start(bsn_bed *bed);
int bsn_timer_stop(bsn_bed *bed, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* BIGSNPR_HIP_H */
