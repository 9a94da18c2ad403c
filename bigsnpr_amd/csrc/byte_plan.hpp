// byte_plan.hpp — the size argument of the byte image's exact-integer kernels (bsn_bed::bits == 8), in one place.
// A genotype is an int8 grid index k, |k| <= 127 (0x80 = missing); the other MFMA operand is another such index
// (windowed LD, ld.hip) or a balanced base-256 digit in [-128, 127] (products, matvec.hip: k_quant).  One int32
// accumulator therefore takes at most 127 * 128 = 16 256 per term and holds floor((2^31 - 1) / 16 256) = 132 104 terms.
// No HIP in here: tests/native pins these on the CPU (tests/test_ld_plan_cpu.py).
#pragma once
#include <cstdint>

namespace bsn {
constexpr int64_t kByteTermMax = 127 * 128;
// contraction over samples (k_pair_xy8, k_pair_stats8, k_cprod8): the sample range in slices of 2^17 samples, one int32
// partial sum per slice (127 * 128 * 131 072 = 2^31 - 2^24), the slices added in 64 bits
constexpr int64_t kSliceBytes = 131072;
// k_pair_xy8's statistics block has six planes per tile pair; the products keep the same limit, so that a byte image
// that windowed LD accepts is one the products accept
constexpr int kByteMaxSlices = 6;
inline int byte_slices(int64_t pitch) { return (int)((pitch + kSliceBytes - 1) / kSliceBytes); }

// contraction over variants (k_prod8): a K-slab of at most 132 104 variants per int32 accumulator, in whole 64-variant
// steps: 2 064 of them
constexpr int64_t kByteSlabVariants = ((((int64_t)1 << 31) - 1) / kByteTermMax) / 64 * 64;
// the fewest slabs that keep every slab of m_pad variants (a multiple of 64) within that
inline int64_t byte_min_slabs(int64_t m_pad) { return (m_pad + kByteSlabVariants - 1) / kByteSlabVariants; }
// variants per slab when `steps` 64-variant steps are cut into `ky` slabs (prod_planes: mc)
inline int64_t slab_variants(int64_t steps, int64_t ky) { return (steps + ky - 1) / ky * 64; }
}  // namespace bsn
