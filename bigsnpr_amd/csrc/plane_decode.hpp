// plane_decode.hpp — the 2-bit device codes of 16 genotypes (one 32-bit word of the image) as int8 MFMA operand planes.
// Shared by the windowed-LD kernels (ld.hip: samples are the contraction index) and the kinship kernels (king.hip:
// variants are, on the sample-major copy).  Field e of byte b of the word goes to byte b of register e of the plane: the
// same permutation of the 16 positions for both operands of a product, so it cancels in every sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bsn {

typedef int v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t lut4b(uint32_t lut, uint32_t sel) {
  return __builtin_amdgcn_perm(lut, lut, sel);
}
// device code (bsn_internal.hpp: 0, 1, 2 = allele count, 3 = missing) -> plane value
constexpr uint32_t kLX = 0x00020100u;   // code 0,1,2,3 -> 0, 1, 2, 0
constexpr uint32_t kLX2 = 0x00040100u;  //               -> 0, 1, 4, 0
constexpr uint32_t kLM = 0x00010101u;   //               -> 1, 1, 1, 0
constexpr uint32_t kLH = 0x00000100u;   //               -> 0, 1, 0, 0  (heterozygous)

// the four 2-bit fields of every byte of w, one field per register
struct Fields {
  uint32_t s0, s1, s2, s3;
};
__device__ __forceinline__ Fields fields(uint32_t w) {
  return Fields{w & 0x03030303u, (w >> 2) & 0x03030303u, (w >> 4) & 0x03030303u, (w >> 6) & 0x03030303u};
}
__device__ __forceinline__ v4i plane(uint32_t lut, const Fields &f) {
  return v4i{(int)lut4b(lut, f.s0), (int)lut4b(lut, f.s1), (int)lut4b(lut, f.s2), (int)lut4b(lut, f.s3)};
}

struct Planes {
  v4i x, x2, m;
};
__device__ __forceinline__ Planes decode3(uint32_t w) {
  const Fields f = fields(w);
  Planes p;
  p.x = plane(kLX, f);
  p.x2 = plane(kLX2, f);
  p.m = plane(kLM, f);
  return p;
}

}  // namespace bsn
