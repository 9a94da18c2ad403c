// ld_plan.hpp — which kernel a windowed-LD band takes (ld.hip: band_run), decided once per call from plain facts.
// No HIP in here: tests/native pins the whole table on the CPU (tests/test_ld_plan_cpu.py).
#pragma once
#include <algorithm>
#include <cstdint>

#include "byte_plan.hpp"

namespace bsn {
// the fp64 epilogue of a pair (ld.hip: pair_value; BandOut::mode carries the same numbers to the device)
enum class LdMode : int {
  cor = 0,        // r of corMat0 with threshold, src/corr.cpp:76-86
  r2 = 1,         // r2 of ld_scores0, src/ld-scores.cpp:52-78
  clump_fbm = 2,  // r2 of clumping_chr: the cross product only, src/clumping.cpp:66-73
  clump_bed = 3   // r2 of bed_clumping_chr: four of the six sums, src/clumping-bed.cpp:69-73
};

// what bsn_ld_last_stats reports; bigsnpr_amd/ld.py (last_stats: `names`, `products`) is indexed by these numbers
enum LdKernel : int {
  kLdSixFused = 0,     // k_pair_stats<FUSE>: six int8 products, fp64 epilogue in the kernel (small band, no K split)
  kLdSixSplit = 1,     // k_pair_stats + k_band_fill: six int8 products, K split (small band, few tile pairs)
  kLdXyI8 = 2,         // k_pair_xy64 (2-bit image) / k_pair_xy8 (byte image) + fill: the cross product alone on the int8 pipe
  kLdByteNa = 3,       // k_pair_stats8 + k_band_fill8na: byte image with missing values, eight int8 products
  kLdSharedI8 = 4,     // k_pair_stats_b: six int8 products, column operand decoded once per workgroup (beyond the FP4 limit)
  // 5 was never assigned
  kLdSharedF4 = 6,     // k_pair_stats_f4<SQ>: six products of look-up planes on the FP4 pipe
  kLdXyF4 = 7,         // k_pair_xy_f4 + k_band_fill: the cross product alone on the FP4 pipe
  kLdQuadF4 = 8,       // k_quad_xy_f4 + k_band_fill: the same for 2 x 2 tile pairs per workgroup
  kLdSharedF4Four = 9, // k_pair_stats_f4<!SQ>: the four products of the bed clumping formula, look-up planes
  kLdRawSix = 10,      // k_pair_stats_f4<SQ, RAW>: six products of look-up-free planes + per-variant totals
  kLdRawFour = 11      // k_pair_stats_f4<!SQ, RAW>: the four products of the bed clumping formula, look-up-free planes
};

enum class LdPath {
  byte_na,        // byte image, missing values among the selected samples
  byte_xy,        // byte image, cross product only
  shared_decode,  // 2-bit image, six / four sums, enough 128 x 32 blocks to fill the chip without a K split
  xy,             // 2-bit image, cross product only
  small_band      // 2-bit image, six sums, too few blocks for shared_decode (or a scattered ind.col)
};

struct BandFacts {
  int bits = 2;                 // bsn_bed::bits: 2 (genotype codes) or 8 (dosage grid)
  int64_t pitch = 0, n = 0;     // bytes per variant of the image; samples of the image
  LdMode mode = LdMode::cor;
  bool complete = false;        // no missing value among the selected samples of the selected variants
  bool contig = false;          // every 128-variant tile lies within 2 GB of its first variant, ascending
  bool all_rows = false;        // every sample of the image is selected
  bool have_cnn = false;        // the per-variant non-missing counts are on the device (raw-plane kernel)
  int64_t npairs_b = 0;         // 128 x 32 blocks of the whole band
  bool i8 = false, lut = false, no_quad = false;   // BSN_LD_I8, BSN_LD_LUT, BSN_LD_NO_QUAD
};

struct BandPlan {
  LdPath path;
  LdKernel kernel;          // what the path reports; xy and small_band decide per batch (xy_kernel, small_band_kernel)
  bool f4 = false;          // the FP4 matrix pipe (its fp32 sums are exact)
  bool raw = false;         // shared_decode: planes without look-ups
  bool nomask = false;      // every sample selected and the kernel's planes ignore the pad samples: no keep-mask
  bool quad_all = false;    // xy: batches of >= 64 tile pairs go to k_quad_xy_f4
};

inline BandPlan plan_band(const BandFacts &f) {
  BandPlan p;
  const bool xy_only = f.complete || f.mode == LdMode::clump_fbm;   // FBM clumping reads the cross product only (src/clumping.cpp:66-73)
  const bool bed_formula = f.mode == LdMode::clump_bed;
  if (f.bits == 8) {
    p.path = xy_only ? LdPath::byte_xy : LdPath::byte_na;
    p.kernel = xy_only ? kLdXyI8 : kLdByteNa;
  } else if (!xy_only && f.contig && f.npairs_b >= 1024) {
    p.path = LdPath::shared_decode;
    // the FP4 matrix pipe while the sums stay exact in fp32 (at most 4 n < 2^24, pad samples counted); BSN_LD_I8=1: the int8 kernel
    p.f4 = f.pitch * 4 <= 4194303 && !f.i8;
    // planes without look-ups while 9 n < 2^24 (BSN_LD_LUT=1: the look-up kernel)
    p.raw = p.f4 && f.pitch * 4 <= 1864135 && !f.lut && f.have_cnn;
    // every sample selected: no keep-mask (the pad samples are code 0 and add nothing to the raw products)
    p.nomask = p.raw && f.all_rows;
    p.kernel = p.raw ? (bed_formula ? kLdRawFour : kLdRawSix) : p.f4 ? (bed_formula ? kLdSharedF4Four : kLdSharedF4) : kLdSharedI8;
  } else if (xy_only) {
    p.path = LdPath::xy;
    p.f4 = f.n <= 4194303 && !f.i8;   // (round 6) 4 n < 2^24
    p.nomask = p.f4 && f.all_rows;    // pad samples are code 0 and add nothing to a cross product
    p.quad_all = p.f4 && f.bits == 2 && !f.no_quad;
    p.kernel = p.f4 ? kLdXyF4 : kLdXyI8;
  } else {
    p.path = LdPath::small_band;
    p.kernel = kLdSixSplit;
  }
  return p;
}

// xy, per batch of np tile pairs: 2 x 2 blocks of tile pairs per workgroup once there are enough of them to fill the chip
inline LdKernel xy_kernel(const BandPlan &p, int64_t np) { return p.quad_all && np >= 64 ? kLdQuadF4 : p.kernel; }
// small_band, per batch: the whole sample range in one workgroup -> the epilogue runs in the kernel
inline LdKernel small_band_kernel(int ksplit) { return ksplit == 1 ? kLdSixFused : kLdSixSplit; }

// K split: `want` workgroups per tile pair to fill the chip when there are few pairs, none of them with less than
// `min_bytes` of a variant's `pitch` bytes; a split is a multiple of `align` bytes
struct KSplit { int splits; int64_t bytes; };
inline KSplit k_split(int64_t pitch, int64_t want, int64_t align, int64_t min_bytes) {
  const int64_t s = std::max<int64_t>(1, std::min(want, pitch / min_bytes));
  const int64_t bytes = ((pitch + s - 1) / s + align - 1) / align * align;
  return KSplit{(int)((pitch + bytes - 1) / bytes), bytes};
}

// Byte image, cross product only (k_pair_xy8), a batch of np tile pairs.  `splits` is the number of splits PER SLICE and the
// grid's y is splits * byte_slices(pitch): slice s of a pair has an int32 plane of its own, so a split never straddles a slice.
// One slice: any 64-byte-aligned split of the row; several: a power-of-two number of splits per 131 072-byte slice.
inline KSplit byte_xy_split(int64_t pitch, int64_t np) {
  const int nslice = byte_slices(pitch);
  const int64_t want = std::max<int64_t>(1, 8192 / (np * nslice));
  if (nslice == 1) return k_split(pitch, want, 64, 256);
  KSplit ks{1, kSliceBytes};
  while (ks.splits * 2 <= want && ks.splits < 512) ks.splits *= 2, ks.bytes /= 2;
  return ks;
}
// Byte image with missing values (k_pair_stats8, four workgroups per split), a batch of np tile pairs: `splits` over the whole
// row, enough to fill the chip.  A split may straddle a slice boundary but is never LONGER than a slice: its int32 sums
// are added to int64 statistics, so only the length counts.
inline KSplit byte_na_split(int64_t pitch, int64_t np) {
  const int64_t ks = std::max<int64_t>(byte_slices(pitch), std::min<int64_t>(std::max<int64_t>(1, 4096 / (np * 4)), pitch / 256));
  const int64_t bytes = std::min(((pitch + ks - 1) / ks + 63) / 64 * 64, kSliceBytes);
  return KSplit{(int)((pitch + bytes - 1) / bytes), bytes};
}

}  // namespace bsn
