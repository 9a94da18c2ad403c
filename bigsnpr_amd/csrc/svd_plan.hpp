// svd_plan.hpp — what a bsn_bed_randomsvd call solves with (svd.hip): vectors per pass, digit slices, precision schedule,
// start grid, warm start and which second copy of the image serves it, decided once per call from plain facts.
// No HIP in here: tests/native pins the table on the CPU (tests/test_svd_plan_cpu.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "orth_small.hpp"   // kOrthMaxB: the columns of a panel, i.e. the most vectors a pass takes
#include "svd_driver.hpp"

namespace bsn {

// bsn_svd_options::warm_denominator (0 -> 16)
inline int warm_den_of(int asked) { return asked >= 2 ? asked : 16; }

struct SolveFacts {
  // bsn_svd_options, as the caller gave them (0 = automatic)
  int k = 10;
  double tol = 0.0;
  int slices = 0, block = 0;
  double vec_floor = 0.0;
  int warm_start = 0, warm_denominator = 0, max_basis = 0, max_restarts = 0;
  uint32_t seed = 0;
  int verbose = 0;
  // the operator: variants of this rank, variants over all ranks (never 0), samples, and where its variants lie in the image
  int64_t m = 0, m_total = 0, n = 0;
  bool cols_contig = false;
  int64_t col0 = 0;
  bool fused = false;               // the scaling is bed_scaleBinom evaluated inside the solve
  // the switches, read by the caller
  bool vec_floor_set = false;       // BSN_VEC_FLOOR (A/B and the accuracy sweeps of the tests)
  double vec_floor_env = 0.0;
  bool start_slices_set = false;    // BSN_START_SLICES (ablation build)
  int start_slices_env = 0;
  bool zq_split = false;            // BSN_ZQ_SPLIT (ablation build)
};

struct SolvePlan {
  SvdOptions so;
  int op_slices = 0;         // bsn_op::slices: digits of the streaming products (after a solve: the digits it ended on)
  bool warm_on = false;      // the warm start will run (enough variants over all ranks)
  bool wants_smaj = false;   // the product passes of this solve are k_prodT's: it wants the sample-major copy
  bool tile_ok = false;      // one-block passes on a layout the tiled copy serves (taken when there is no sample-major copy)
};

// the operator covers a range of variants that k_prodT can read from the sample-major copy: whole 512-variant chunks
inline bool fits_prodT(const SolveFacts &f) { return f.cols_contig && (f.col0 & 511) == 0; }

inline SolvePlan plan_solve(const SolveFacts &f) {
  SolvePlan p;
  SvdOptions &so = p.so;
  so.k = f.k;
  so.tol = f.tol > 0 ? f.tol : 1e-4;
  // Digit slices per fp64 value and vectors per pass.  Rounding a basis block to 8 S bits leaves a
  // relative residual of about 1.2 * 2^(-8 S) on a converged pair (the Ritz VALUES are not
  // affected, svd_driver.hpp), so S is the smallest width whose floor is below tol / 4; the
  // block then fills the 16 MFMA columns of one column block (8 x 2, 5 x 3, 4 x 4, 3 x 5, 2 x 7).
  // A block chosen by the caller gets as many slices as its column blocks hold anyway.
  int s_tol = 2;
  while (s_tol < 7 && 1.2 * std::ldexp(1.0, -8 * s_tol) > so.tol / 4) s_tol++;
  if (f.slices > 0) s_tol = f.slices;
  // One column block (16 MFMA columns) holds b1 vectors, two hold b2.  A pass with two column blocks costs
  // 1.3x a pass with one (the two-block kernels are bound by the matrix pipe and the VALU issue port, not by
  // HBM), but the solve needs fewer block steps: measured at 400K x 1M, tol 1e-4 (profiles/r03_block_vs_k.txt):
  // k = 20: 4 steps of 16 vectors = 8.1 passes, 204 ms, against 6 steps of 8 = 12.1 passes, 219 ms;
  // k <= 10: 5 steps of 8 = 193 ms against 4 steps of 16 = 208 ms.  The default is chosen for the time to
  // the solution, not for pass throughput.
  const int b1 = std::max(1, std::min(8, 16 / s_tol)), b2 = std::max(b1, std::min(kOrthMaxB, 32 / s_tol));
  // (Without the warm start — fewer than 262 144 variants over all ranks — the wide block saves one step of
  // seven instead of two of six and loses: 50 against 35 ms on a 125 000-variant matrix.)
  p.warm_on = f.warm_start >= 0 && f.m_total / warm_den_of(f.warm_denominator) >= 16384;
  const int bb = f.block > 0 ? (f.block > kOrthMaxB ? kOrthMaxB : f.block) : (4 * f.k >= 7 * b1 && p.warm_on ? b2 : b1);
  int ss = s_tol;
  if (f.slices <= 0) {
    const int nb = (bb * s_tol + 15) / 16;
    ss = std::max(s_tol, std::min(7, 16 * nb / bb));
  }
  so.block = bb;
  p.op_slices = ss;
  // precision schedule (svd_driver.hpp): wider panels for the early steps when the vectors are wanted beyond the floor
  // of `ss` digits; a caller who fixed the digits gets them at every step unless he also names a floor
  double vf = f.vec_floor;
  // (round 6: 1e-7, a tenth of north_star's 1e-6.  Round 5's 2.5e-7 left the vectors the ARITHMETIC limits — small matrices
  // that take 20 - 30 block steps, where the leading pairs converge far below tol — at 1.5 - 1.8e-6 on the oracle's
  // shapes; 1e-7 keeps the panels at 24 bits one or two steps longer there (0.5 - 0.97e-6: what uniform 24-bit panels
  // give) and leaves the 400K x 1M solve on the same three wide steps, its vectors being where the Lanczos process
  // is at tol: profiles/r06_vectors_small.txt, r06_vectors_c3.txt)
  if (vf == 0.0) vf = f.slices > 0 ? -1.0 : 1e-7;
  if (f.vec_floor_set) vf = f.vec_floor_env;
  so.slices_base = ss;
  so.slices_max = ss;
  so.vec_floor = 0.0;
  if (vf > 0) {
    int sm = ss;
    while (sm < 7 && 1.2 * std::ldexp(1.0, -8 * sm) > vf) sm++;
    so.slices_max = sm;
    so.vec_floor = vf;
  }
  // the START block only chooses where the iteration begins: an 8-bit grid serves, and the first full crossproduct
  // pass — the one that also counts the codes — then carries `block` digit columns instead of twice as many
  // (16 vectors: one column block, 21 instead of 26 ms per 100 GB; same residuals, same vectors)
  so.slices_start = f.slices > 0 ? 0 : 1;
  if (f.start_slices_set) so.slices_start = f.start_slices_env;
  // columns standardised by bed_scaleBinom: a random vector is amplified by sqrt(n) (svd_driver.hpp)
  // (the product pass scheduled apart from the grids, svd_driver.hpp: measured at 400K x 1M — 12 ms saved, the
  // leading vectors at 9e-7 instead of 1.6e-7; at k = 10, 6e-6: the rounding of Z is heavier-tailed than the model,
  // so the split stays an experiment, BSN_ZQ_SPLIT=1)
  so.noise_gain = (f.fused && f.zq_split) ? std::sqrt((double)f.n) : 0.0;
  // a solve streams the image a dozen times: the ONE-block kernels, which are bound by HBM, get their layout (a
  // second copy in 64-variant x 256-B tiles, one extra pass of copying, kept on the handle) when the device has the
  // room: 2 - 4 % per pass.  The two-block kernels are bound by instruction issue and gain nothing from it (k_prod<2>
  // 23.65 ms on the plain image against 23.75 on the copy, k_cprod<2> 21.65 against 21.52: profiles/r03_shape_sweeps.txt),
  // so the default solve at k >= 14 leaves the other half of the HBM alone; a copy that exists is used either way.
  // ... and a solve with passes of two or three column blocks (16 vectors; 8 vectors on the 24-bit panels of the
  // precision schedule) the sample-major copy: its product passes then run as k_prodT (k_cprod's shape; DESIGN.md
  // 3.3b) instead of k_prod<2> with its transposes and 128 accumulators — and three column blocks exist on that copy
  // only.  One second copy per handle: when the sample-major one is not to be had (no room, BSN_NO_SMAJ) the
  // one-block passes of the solve still get theirs.
  // (m >= 4096 is asked here — no copy is BUILT for a small operator — and not by on_prodT below: kept as found)
  p.wants_smaj = so.block * so.slices_max > 16 && fits_prodT(f) && f.m >= 4096;
  p.tile_ok = so.block * so.slices_base <= 16 && f.cols_contig && (f.col0 & 63) == 0 && f.m >= 4096;
  so.resid_floor = 1.2 * std::ldexp(1.0, -8 * p.op_slices);
  // (two iterations since round 5: + 2.5 ms, every residual of the 400K x 1M solve 4 - 10 x lower at the same step)
  so.warm = f.warm_start < 0 ? 0 : (f.warm_start == 0 ? 2 : f.warm_start);
  so.max_basis = f.max_basis;
  so.max_restarts = f.max_restarts == 0 ? 100 : f.max_restarts;
  so.seed = f.seed ? f.seed : 1;
  so.verbose = f.verbose;
  return p;
}

// bsn_svd_info::tiled == 2, given that the sample-major copy exists: the product passes of a solve with these options ran
// as k_prodT, one launch of two or three column blocks.  (<= 48, three column blocks, is asked here and not by wants_smaj,
// which is what decides about BUILDING the copy: kept as found)
inline bool on_prodT(const SvdOptions &so, const SolveFacts &f) {
  return so.block * so.slices_max > 16 && so.block * so.slices_max <= 48 && fits_prodT(f);
}

// A Krylov space exhausted on rounded products, or requested triplets below what the rounded products resolve — sigma
// below 1.5e-4 sigma_1 on 16-bit panels: the driver leaves them out of its convergence test (they cannot meet it there)
// and says so; their VALUES need the wide products.  Rare: k beyond the numerical rank at 16 bits.  Only in the
// automatic mode: a caller who fixed the digits keeps them.
inline bool needs_resolve(const SvdResult &r, const SolveFacts &f, const SolvePlan &p) {
  return ((r.exhausted && r.exhausted_resid > 1e-9) || r.below_resolution > 0) && f.slices <= 0 && p.op_slices < 7;
}

// ... the second solve: 56-bit digits at every step, at most four vectors per pass (only matrices whose rank fits the
// basis get here, so it is cheap)
inline SolvePlan plan_resolve(SolvePlan p) {
  p.op_slices = 7;
  p.so.slices_base = p.so.slices_max = 7;
  p.so.vec_floor = 0.0;
  p.so.block = std::min(p.so.block, 32 / 7);
  p.so.resid_floor = 1.2 * std::ldexp(1.0, -8 * p.op_slices);
  return p;
}

}  // namespace bsn
