// prod_plan.hpp — the launch geometry of the streaming products (matvec.hip: prod_planes, op_cprod) and which instance of
// k_cprod / k_prod / k_prodT a launch takes, decided from plain facts.
// No HIP in here but the __host__ __device__ mark of prodt_slab and cprod_slab, which k_prodT and k_cprod compile as they
// stand: tests/native pins the geometry and the choices on the CPU (tests/test_prod_plan_cpu.py, tests/test_prodt_grid_cpu.py,
// tests/test_cprod_grid_cpu.py).
#pragma once
#include <algorithm>
#include <cstdint>

#include "byte_plan.hpp"

#if defined(__HIPCC__)
#define BSN_PLAN_HD __host__ __device__ inline
#else
#define BSN_PLAN_HD inline
#endif

namespace bsn {
// Column blocks of 16 digit columns per launch.  Three (48 columns: 16 vectors x 3 slices, the early steps of a solve
// whose vectors are wanted beyond the 16-bit floor, svd_driver.hpp) exist for the two shapes such a solve runs on —
// k_cprod on the 2-bit image and k_prodT on its sample-major copy; everything else stays at two.
constexpr int kMaxCols = 48;
constexpr int kMetaVecs = 32;   // vectors per launch at most
inline int pick_nb(int ncols_needed) { return ncols_needed <= 16 ? 1 : ncols_needed <= 32 ? 2 : 3; }

// vectors per crossproduct launch: three column blocks on a 2-bit image unless the launch also counts the codes
inline int cprod_vmax(int bits, bool stats_pending, int S) {
  const int nbmax = (bits == 2 && !stats_pending) ? 3 : 2;
  int v = 16 * nbmax / S;
  if (v > kMetaVecs) v = kMetaVecs;
  return v < 1 ? 1 : v;
}

// ---- Y = A~ X: the geometry of one prod_planes call ---------------------------------------------------------------
struct ProdFacts {
  int bits = 2;                  // bsn_bed::bits: 2 (genotype codes) or 8 (dosage grid)
  int64_t n = 0, m = 0;          // samples of the image; variants of the operator
  int64_t pitch = 0;             // bytes per variant of the image
  int64_t col0 = 0;              // first variant of a contiguous operator
  bool cols_contig = false;
  bool have_smaj = false;        // the sample-major copy exists and BSN_NO_SMAJ is unset
  int mode = 1;                  // 1: the scaled product; 2: raw plane weights
  bool raw_na = false;           // lutP / lutQ are the raw-code / missing-value pair of the scaled product
  bool has_q = true;             // the second plane is computed (complete data drops the missing-value plane)
  bool no_sparse = false;        // BSN_NO_SPARSE_PROD
  int nvec = 1, S = 1;           // vectors of the panel, digit slices per vector
  int ncu = 256;                 // compute units of the device
  bool segmented = false;        // a pass in segments of sample blocks (op_prod_segments): k_prodT only
  int ky = 0, ky_t = 0;          // profiling build: the slab sweeps BSN_KY (k_prod) / BSN_KY_T (k_prodT); 0 = the rule
  int ky_whole = 0;              // profiling build: BSN_KY_WHOLE, the slabs of k_prodT's whole-round blocks; 0 = the rule
};

enum class ProdRefusal { none, pitch_limit, nothing_queued };

struct ProdPlan {
  ProdRefusal refuse = ProdRefusal::none;   // pitch_limit: an error; nothing_queued: the caller takes the plain pass
  bool smaj = false;        // the pass runs as k_prodT on the sample-major copy (ONE launch)
  int vmax = 1;             // vectors per launch
  int64_t m_pad = 0;        // variants padded to whole steps (64) or chunks (512: k_prodT)
  int64_t wgx = 0;          // workgroups along the samples
  int ky = 1;               // slabs of variants (the grid's y; int32 partial sums per slab)
  int smaj_cps = 0;         // k_prodT: chunks of 512 variants per slab
  // k_prodT: sample blocks 0 .. wgx_whole - 1 fill whole rounds of the CUs and take ky_whole slabs of cps_whole chunks;
  // ky x smaj_cps is then the split of the blocks wgx_whole .. wgx - 1 alone.  wgx_whole = 0: every block takes ky x smaj_cps
  int64_t wgx_whole = 0;
  int ky_whole = 0, cps_whole = 0;
  int64_t mc = 0;           // k_prod / k_prod8: variants per slab
  bool sparse_ok = false;   // k_prodT<3> may run in its sparse form (prodt_sparse.hpp)
};

// Slabs of the sample blocks of k_prodT that fill whole rounds of the CUs (0: no second split, every block takes ky slabs).
// Measured at 400 000 x 1 000 000 against 2, 3 and the split of every block: profiles/prodt_whole_rounds_ab.txt.
constexpr int kProdTWholeSlabs = 2;

// k_prodT's grid has ONE dimension: first the whole-round blocks slab by slab (as the two-dimensional grid ran them: all the
// blocks of a slab side by side, so the workgroups in flight read the same chunks of the digit panel), then the remainder
// blocks slab by slab — last, so that the CUs which finish their long workgroups first pick up the short ones.
struct ProdTGrid {
  int wgx, wgx_whole;       // sample blocks; those of the whole rounds
  int ky_whole, cps_whole;  // slabs / chunks per slab of blocks 0 .. wgx_whole - 1
  int ky, cps;              // of blocks wgx_whole .. wgx - 1
  int nchunks;              // chunks of 512 variants of the pass
};
struct ProdTSlab {
  int bx, slab;             // sample block; slab (the accumulator's first index)
  int ch_begin, ch_end;     // its chunks
};
inline ProdTGrid prodt_grid(const ProdPlan &p) {   // (of a plan with p.smaj)
  return {(int)p.wgx, (int)p.wgx_whole, p.ky_whole, p.cps_whole, p.ky, p.smaj_cps, (int)(p.m_pad / 512)};
}
BSN_PLAN_HD int64_t prodt_workgroups(const ProdTGrid &g) {
  return (int64_t)g.wgx_whole * g.ky_whole + (int64_t)(g.wgx - g.wgx_whole) * g.ky;
}
// workgroup wg of the grid -> (sample block, slab, first chunk, end chunk); shared by k_prodT and tests/native
BSN_PLAN_HD ProdTSlab prodt_slab(const ProdTGrid &g, uint32_t wg) {
  const uint32_t nwhole = (uint32_t)g.wgx_whole * (uint32_t)g.ky_whole;
  ProdTSlab s;
  int cps;
  if (wg < nwhole) {
    s.slab = (int)(wg / (uint32_t)g.wgx_whole);
    s.bx = (int)(wg - (uint32_t)s.slab * (uint32_t)g.wgx_whole);
    cps = g.cps_whole;
  } else {
    const uint32_t r = wg - nwhole, nrest = (uint32_t)(g.wgx - g.wgx_whole);
    s.slab = (int)(r / nrest);
    s.bx = g.wgx_whole + (int)(r - (uint32_t)s.slab * nrest);
    cps = g.cps;
  }
  s.ch_begin = s.slab * cps;
  s.ch_end = s.ch_begin + cps < g.nchunks ? s.ch_begin + cps : g.nchunks;
  return s;
}

inline ProdPlan plan_prod(const ProdFacts &f) {
  ProdPlan p;
  // k_prod addresses a 64-variant step with 32-bit offsets from its first row
  if (f.pitch >= ((int64_t)1 << 24)) {
    p.refuse = ProdRefusal::pitch_limit;
    return p;
  }
  const int nvec = f.nvec, S = f.S;
  const int64_t npad = f.bits == 8 ? f.pitch : f.pitch * 4;   // samples a variant row is padded to
  // Two or three column blocks over a contiguous range of variants that starts on a 512-variant chunk, and the handle
  // has its sample-major copy: the product runs as k_prodT (k_cprod's shape, contraction over the contiguous index).
  const bool smaj_ok = f.bits == 2 && f.have_smaj && f.cols_contig && (f.col0 & 511) == 0 && f.mode == 1 && f.raw_na;
  const int vmax_smaj = std::min(kMetaVecs, (smaj_ok && nvec * S > 32 ? kMaxCols : 32) / S);
  const bool smaj = smaj_ok && nvec <= vmax_smaj && pick_nb(nvec * S) >= 2;   // (ONE launch: the geometry below is k_prodT's)
  // (a panel that needs several launches stays on k_prod, which has two column blocks at most: 16 vectors x 56 bits with
  // the copy in place used to cut itself into launches of three — "three column blocks without the sample-major copy")
  const int vmax = smaj ? vmax_smaj : std::max(1, std::min(kMetaVecs, 32 / S));
  p.smaj = smaj;
  p.vmax = vmax;
  if (f.segmented && !smaj) {
    p.refuse = ProdRefusal::nothing_queued;
    return p;
  }
  const int64_t unit = smaj ? 512 : 64;
  const int64_t m_pad = (f.m + unit - 1) / unit * unit;
  // K split so that the grid has a few thousand workgroups
  int64_t wgx = f.bits == 8 ? npad / 256 : npad / 1024;  // workgroups along the samples
  int ky = (int)((4096 + wgx - 1) / wgx);
  const int64_t steps = m_pad / 64;
  int smaj_cps = 0;   // k_prodT: chunks of 512 variants per slab
  const int nb_max = pick_nb((nvec < vmax ? nvec : vmax) * S);   // column blocks of the (first, largest) launch
  if (smaj) {
    // one 1024-thread workgroup per CU is resident: among 6 .. 24 slabs the split whose grid fills whole rounds of
    // the chip best, less what the slabs cost (below); a slab stays below 2.5e6 variants
    const int ncu = f.ncu;
    wgx = (f.n + 511) / 512;
    const int64_t nchunks = m_pad / 512;
    // every slab writes its own n x 16 NB int32 partial sums and the finalize kernel reads them back — 0.15 % of the
    // image's bytes per slab at 400K x 1M, 1.2 % on the 125 000-variant shard of an 8-GPU run, where 18 slabs (the best
    // fill) measured 3.93 ms per pass against 3.80 - 3.82 with 8 - 10 (round 6, profiles/r06_shard_slabs.txt: the traffic
    // weighs about 0.3 of its bytes — the writes drain beside the stream).  At 400 000 x 1 000 000 on 256 CUs the rule
    // gives 18 slabs of 109 chunks (782 x 18 workgroups = 54.98 rounds) for two and for three column blocks.  Since the
    // second split below only the blocks beyond the last whole round take this split (14 of the 782); the rule and its
    // fields are as they were, and where there is no second split they describe every block.
    const double slab_cost = 0.3 * 2.0 * (double)npad * 16.0 * nb_max * 4.0 / ((double)m_pad * (double)(f.pitch));
    int best = 1;
    double best_score = -1e300;
    for (int c = 1; c <= 24 && c <= nchunks; c++) {
      if (c < 6 && c < nchunks && nchunks >= 6) continue;
      const int64_t W = wgx * c;
      const double fill = (double)W / ((double)ncu * (double)((W + ncu - 1) / ncu));
      const double score = fill - slab_cost * c;
      if (score > best_score + 1e-9) best_score = score, best = c;
    }
    ky = best;
    if (f.ky_t > 0) ky = std::max(1, std::min(f.ky_t, (int)nchunks));  // slab sweep of k_prodT (correct results)
    const int64_t ky_min2 = (m_pad + 2499999) / 2500000;
    if (ky < ky_min2) ky = (int)ky_min2;
    smaj_cps = (int)((nchunks + ky - 1) / ky);
    ky = (int)((nchunks + smaj_cps - 1) / smaj_cps);
    // The split above exists only because the sample blocks alone do not fill whole rounds (782 = 3.05 x 256).  The first
    // wgx / ncu rounds of blocks are whole rounds whatever their slab count, so they take kProdTWholeSlabs slabs (each
    // block streams all, or half, ... of the variants in one workgroup: 1 / ky of the partial sums, of k_prod_final's
    // reads and of the workgroup prologues) and ky x smaj_cps is the split of the remainder blocks alone, which are
    // launched last (prodt_slab).  Not for a pass in segments (their blocks are pieces x bs, interleaved) nor where the
    // blocks are less than one round.  ONE slab is not the best count: a workgroup then holds its CU for a third of the
    // pass, and the kernels a solve queues on its second stream beside the pass (svd.hip: the early Rayleigh-Ritz guess)
    // get a CU only where a workgroup ends.  A/B of 1, 2, 3 and the split of every block: profiles/prodt_whole_rounds_ab.txt.
    if (!f.segmented && kProdTWholeSlabs + f.ky_whole > 0 && wgx >= ncu) {
      p.wgx_whole = wgx / ncu * ncu;
      int kw = f.ky_whole > 0 ? f.ky_whole : kProdTWholeSlabs;   // (BSN_KY_WHOLE: the sweep of the profiling build)
      // (a slab of whole chunks below 2.5e6 variants: 4 882 chunks at most, which is at least ky_min2 slabs)
      kw = (int)std::max<int64_t>(std::min<int64_t>(kw, nchunks), (nchunks + 4881) / 4882);
      p.cps_whole = (int)((nchunks + kw - 1) / kw);
      p.ky_whole = (int)((nchunks + p.cps_whole - 1) / p.cps_whole);
    }
  }
  if (!smaj) {   // (k_prodT's slab count and chunks per slab were fixed together above: clamping one would drop chunks)
    if (ky > steps) ky = (int)steps;
    if (ky > 64) ky = 64;
  }
  if (ky < 1) ky = 1;
  if (f.bits == 2 && nb_max == 1) {
    // (one column block: the kernel is bound by HBM; with two it is bound by instruction issue, more slabs only help
    // there — 400 000 x 125 000, 16 vectors: 4 slabs 3.45 ms, 5: 3.19, 9: 3.13, 11: 3.12 — and the rule above stays)
    // ... but every slab writes (and the finalize kernel reads back) its own n x 16 NB accumulators: on a matrix with
    // few samples per variant that is real traffic (50 000 x 200 000: 64 slabs = 16 % of the image), so the split is
    // capped at 4 % of the image bytes; and two workgroups per CU are resident, so among the splits left the one
    // whose grid fills whole rounds of 512 best wins (same matrix: 10 slabs = 490 workgroups, 0.72 - 0.75 ms per
    // call against 0.80 - 0.84 with 64 and 0.86 with 11 = 539; profiles/r03_c2_grid_sweep.txt)
    const int ncol_max = 16 * nb_max;
    int64_t cap = (int64_t)(0.04 * (double)m_pad / (32.0 * ncol_max));
    if (cap < 1) cap = 1;
    if (ky > cap) ky = (int)cap;
    int best = ky;
    double best_fill = 0.0;
    for (int c = ky; c >= 1 && 2 * c >= ky; c--) {
      const int64_t W = wgx * c;
      const double fill = (double)W / (512.0 * (double)((W + 511) / 512));
      if (fill > best_fill + 1e-9) best_fill = fill, best = c;
    }
    ky = best;
  }
  if (!smaj && f.ky > 0) {   // grid-shape sweep of k_prod (correct results)
    ky = f.ky;
    if (ky > steps) ky = (int)steps;
    if (ky < 1) ky = 1;
  }
  // int32 accumulators: a slab adds at most 768 per variant (planes up to 4, digits up to 128); on a byte image
  // 127 * 128 (grid indices up to 127), which leaves 132 104 variants per slab (byte_plan.hpp)
  const int64_t ky_min = f.bits == 8 ? byte_min_slabs(m_pad) : (m_pad + 2499999) / 2500000;
  if (ky < ky_min && !smaj) ky = (int)ky_min;
  const int64_t mc = slab_variants(steps, ky);
  if (!smaj) ky = (int)((m_pad + mc - 1) / mc);
  // k_prodT<3> with the missing-value plane runs in its sparse form (one matrix instruction for both planes,
  // prodt_sparse.hpp: 27.8 against 29.5 ms per pass at 400K x 1M); with two column blocks the 18-instruction decode
  // outweighs the two matrix instructions it saves per tile (23.3 against 22.4 ms, profiles/sparse_prod_ab.txt) and the
  // dense kernel stays.  BSN_NO_SPARSE_PROD=1: the dense two-plane kernel (A/B switch, bit-identical; read on every call)
  // Its per-slice sums differ from the dense kernel's by carries between the digit slices, and k_prod_final adds the
  // slices in fp64: the same Y needs that sum exact — 3 m_pad 2^(8S-1) below 2^53 for the largest panel the scale admits
  // (codes up to 3, integers below 2^(8S-1), m_pad variants).  True for every 24-bit panel; the 56-bit panels of a wide
  // solve keep the dense kernel.  (S <= 8: the power of two is exact in a double, so is the product's scaling by it.)
  p.sparse_ok = smaj && f.has_q && !f.no_sparse &&
                3.0 * (double)m_pad * (double)((uint64_t)1 << (8 * S - 1)) < 9007199254740992.0;
  p.m_pad = m_pad;
  p.wgx = wgx;
  p.ky = ky;
  p.smaj_cps = smaj_cps;
  p.mc = mc;
  return p;
}

// ---- which instance a launch takes ------------------------------------------------------------------------------
// k_cprod<NB, NPLANE, 512, RAW0, STATS, contig, tiles, waves, 1, tag, tiled, sgb, naskip>.  Shapes (profiles/r02_ablation.txt,
// r03_shape_sweeps.txt, r04_two_block_kernels.txt): one column block — 8 waves x 2 tiles on the plain image, 8 x 4 on the
// tiled copy (2 % faster there; the counting variant needs 150 registers with 4 tiles and keeps 2); two and three column
// blocks — 16 waves x 2 tiles share one digit panel (half the L2 reads of it), contiguous variants with the explicit MFMA /
// decode interleave + raised priority through the MFMA phase (sgb = 3: 2 %).
struct CprodKernel {
  int NB;
  bool contig;
  int tiles, waves, tag;
  bool tiled;
  int sgb;
  bool naskip;
};
inline bool operator==(const CprodKernel &a, const CprodKernel &b) {
  return a.NB == b.NB && a.contig == b.contig && a.tiles == b.tiles && a.waves == b.waves && a.tag == b.tag &&
         a.tiled == b.tiled && a.sgb == b.sgb && a.naskip == b.naskip;
}
struct CprodFacts {
  int NB = 1;               // column blocks of the launch
  bool plain = true;        // the plain pass (two planes, raw codes, no counting): the one with skipping kernels
  bool stats = false;       // the launch counts the codes
  bool cols_contig = false;
  bool tiled = false;       // the streaming-layout copy serves this operator (64-aligned contiguous variants)
  bool warm = false;        // a warm-start launch: its own kernel name (tag = 1) where one column block has one
  bool na_skip = false;     // op_na_blocks chose the kernels that skip the missing-value plane of clean K-steps
};
inline CprodKernel choose_cprod(const CprodFacts &f) {
  if (f.plain && f.na_skip && f.NB >= 2) return {f.NB, f.cols_contig, 2, 16, 0, false, 0, true};
  if (f.NB == 3) return {3, f.cols_contig, 2, 16, 0, false, f.cols_contig ? 3 : 0, false};   // plain image only
  if (f.tiled) return f.NB == 1 ? CprodKernel{1, true, f.stats ? 2 : 4, 8, f.warm ? 1 : 0, true, 0, false}
                                : CprodKernel{2, true, 2, 16, 0, true, 3, false};
  if (f.NB == 1) return {1, f.cols_contig, 2, 8, f.cols_contig && f.warm ? 1 : 0, false, 0, false};
  return {2, f.cols_contig, 2, 16, 0, false, f.cols_contig ? 3 : 0, false};
}

// ---- Z = A~' X: the grid of one k_cprod launch ---------------------------------------------------------------------
// A workgroup of k_cprod owns a block of variants (256 with one column block, 512 with two or three) for the whole sample
// range, so the blocks alone leave the last round of the CUs partly empty: 1 954 blocks of 512 variants are 7.63 rounds of
// 256 CUs.  As for k_prodT, the blocks that fill whole rounds stay as they are — one workgroup, all 512-sample chunks, sums
// straight into acc_out — and only the blocks beyond the last whole round are cut along the samples into `slabs` slabs of
// `cps` chunks, whose int32 partial sums k_cprod_final adds.  A launch with less than one round of blocks (the warm start of
// a solve: 1 / 16 of the variants) is all remainder.  No atomics, no workgroup waits for another.
struct CprodGridFacts {
  int64_t m = 0;            // variants of the launch
  int per_wg = 512;         // variants of a workgroup (16 x tiles x waves of the instance)
  int nchunks = 1;          // chunks of 512 samples of the image
  int64_t pitch = 128;      // bytes per variant of the image
  int NB = 1, nplane = 2;   // column blocks, planes of the launch
  int ncu = 256;            // compute units (BSN_PLAN_CUS overrides the device's)
  int resident = 1;         // workgroups of the launched instance a CU holds (asked of the runtime)
  bool one_split = false;   // BSN_CPROD_ONE_SPLIT=1, or an instance without the geometry: one workgroup per block
  int slabs = 0;            // BSN_CPROD_SLABS: the slab count of the remainder blocks instead of the rule's (1: none); 0 = the rule
};
struct CprodGrid {
  int blocks = 0, blocks_whole = 0;   // blocks of variants; those of the whole rounds (== blocks: the geometry as it was)
  int slabs = 0, cps = 0;             // slabs / chunks per slab of blocks blocks_whole .. blocks - 1 (0, 0 without a remainder)
  int nchunks = 0;                    // chunks of 512 samples
  int64_t m_rem = 0;                  // variants from the first remainder block on (the partial region's variant count)
};
struct CprodSlab {
  int block, slab;          // block of variants; slab (the partial region's first index; 0 for a whole-round block)
  int ch_begin, ch_end;     // its chunks
};
constexpr int kCprodMaxSlabs = 24;
BSN_PLAN_HD int64_t cprod_workgroups(const CprodGrid &g) {
  return (int64_t)g.blocks_whole + (int64_t)(g.blocks - g.blocks_whole) * g.slabs;
}
// int32 words of the partial region [slab][plane][variant - first remainder variant][16 NB]
inline int64_t cprod_partial_words(const CprodGrid &g, int nplane, int NB) {
  return (int64_t)g.slabs * nplane * g.m_rem * 16 * NB;
}
// workgroup wg of the one-dimensional grid -> (block, slab, first chunk, end chunk); shared by k_cprod and tests/native.
// The whole-round blocks first, then the remainder slab by slab — last, so that the CUs which finish first pick them up.
BSN_PLAN_HD CprodSlab cprod_slab(const CprodGrid &g, uint32_t wg) {
  CprodSlab s;
  if (wg < (uint32_t)g.blocks_whole) {
    s.block = (int)wg, s.slab = 0, s.ch_begin = 0, s.ch_end = g.nchunks;
    return s;
  }
  const uint32_t r = wg - (uint32_t)g.blocks_whole, nrest = (uint32_t)(g.blocks - g.blocks_whole);
  s.slab = (int)(r / nrest);
  s.block = g.blocks_whole + (int)(r - (uint32_t)s.slab * nrest);
  s.ch_begin = s.slab * g.cps;
  s.ch_end = s.ch_begin + g.cps < g.nchunks ? s.ch_begin + g.cps : g.nchunks;
  return s;
}
inline CprodGrid plan_cprod(const CprodGridFacts &f) {
  CprodGrid g;
  g.blocks = (int)((f.m + f.per_wg - 1) / f.per_wg);
  g.nchunks = f.nchunks;
  g.blocks_whole = g.blocks;
  const int64_t slots = (int64_t)std::max(1, f.ncu) * std::max(1, f.resident);
  const int64_t whole = g.blocks / slots * slots, rest = g.blocks - whole;
  if (f.one_split || rest == 0 || f.nchunks <= 1) return g;
  // The remainder is cut only where it leaves CUs EMPTY.  Where a CU holds several workgroups (three of the one-block kernel)
  // and every CU still has one, the launch is bound by HBM, not by the places taken: 489 blocks on 256 CUs x 3 (a 125 000-
  // variant shard) cut into 14 slabs ran 6 % SLOWER (2.24 -> 2.39 ms, profiles/cprod_whole_rounds_ab.txt).
  if (rest >= std::max(1, f.ncu) && f.slabs == 0) return g;
  // plan_prod's rule on the remainder alone: among 1 .. 24 slabs the count whose workgroups fill whole rounds best — the
  // remainder then takes rounds / c of a whole block's time, fill is what of that the slots work — less what the slabs
  // cost: every slab writes its nplane x 16 NB int32 sums per variant and k_cprod_final reads them back, against the `pitch`
  // bytes the variant streams.  One slab is the unsplit block, which writes acc_out as ever and costs nothing.
  // The weight of that cost is 1.0.  k_prodT's 0.3 chose 24 slabs for the 245 two-block workgroups of that shard — fill
  // 0.957 -> 0.999 — and the launch with its finalize took 2.83 ms instead of 2.39: 0.9 % per slab where 0.3 says 0.15 %, a
  // weight of 1.8; the sweep at 1M variants (BSN_CPROD_SLABS: 1, 3, 5, 7, 11, 14, 22 — the solve follows the fill) has 3
  // and 11 slabs level, a weight of 0.7.  400 000 x 1 000 000 on 256 CUs: the 162 remainder blocks in 3 slabs of 261 chunks
  // with three column blocks, in 11 of 72 with two; the 67 one-block blocks beyond five rounds of 768 in 11; the 244 one-block
  // workgroups of the warm start in 3.  The shard keeps one workgroup per block.  (profiles/cprod_whole_rounds_ab.txt)
  const double slab_cost = 1.0 * 2.0 * (double)f.nplane * 16.0 * f.NB * 4.0 / (double)f.pitch;
  int best = 1;
  double best_score = -1e300;
  for (int c = 1; c <= kCprodMaxSlabs && c <= f.nchunks; c++) {
    const int cps = (f.nchunks + c - 1) / c;
    if ((f.nchunks + cps - 1) / cps != c) continue;   // (a count that whole chunks cannot make)
    const int64_t W = rest * c;
    const double fill = (double)W / ((double)slots * (double)((W + slots - 1) / slots));
    const double score = fill - (c > 1 ? slab_cost * c : 0.0);
    if (score > best_score + 1e-9) best_score = score, best = c;
  }
  // (BSN_CPROD_SLABS: a count of the caller's — tests at shapes too small for the rule to split, sweeps; whole chunks per slab)
  if (f.slabs > 0) {
    const int c = std::min(f.slabs, f.nchunks), cps = (f.nchunks + c - 1) / c;
    best = (f.nchunks + cps - 1) / cps;
  }
  if (best == 1) return g;   // the split would not pay
  g.blocks_whole = (int)whole;
  g.cps = (f.nchunks + best - 1) / best;
  g.slabs = best;
  g.m_rem = f.m - whole * f.per_wg;
  return g;
}

// k_prod<NB, contig, rawp, hasq, tag, tiled> on the variant-major image (or its streaming-layout copy)
struct ProdKernel {
  int NB;
  bool contig, rawp, hasq;
  int tag;
  bool tiled;
};
inline bool operator==(const ProdKernel &a, const ProdKernel &b) {
  return a.NB == b.NB && a.contig == b.contig && a.rawp == b.rawp && a.hasq == b.hasq && a.tag == b.tag && a.tiled == b.tiled;
}
// rawp: the P plane is the code itself; warm-start launches of it run under their own name (tag = 1)
inline ProdKernel choose_prod(int NB, bool cols_contig, bool tiled, bool rawp, bool has_q, bool warm) {
  return {NB, cols_contig, rawp, has_q, rawp && warm ? 1 : 0, cols_contig && tiled};
}

// k_prodT<NB, hasq, 2, 16, tag, sgb, naskip, sparse> on the sample-major copy
struct ProdTKernel {
  int NB;
  bool hasq;
  int tag, sgb;
  bool naskip, sparse;
};
inline bool operator==(const ProdTKernel &a, const ProdTKernel &b) {
  return a.NB == b.NB && a.hasq == b.hasq && a.tag == b.tag && a.sgb == b.sgb && a.naskip == b.naskip && a.sparse == b.sparse;
}
// The sparse form only with three column blocks and where the host rule does not take the skipping kernels (nearly
// complete data, 1e-4 missing: 186.5 ms per solve on them against 198.7 on the sparse form); the skipping kernels do
// without the explicit MFMA / decode schedule (sgb = 0) and have no warm-start name, nor has dense k_prodT<3>.
inline ProdTKernel choose_prodT(int NB, bool has_q, bool warm, bool na_skip, bool sparse_ok) {
  if (has_q && sparse_ok && NB == 3 && !na_skip) return {3, true, warm ? 1 : 0, 3, false, true};
  if (has_q && na_skip) return {NB, true, 0, 0, true, false};
  return {NB, has_q, NB == 2 && warm ? 1 : 0, 3, false, false};
}

}  // namespace bsn
