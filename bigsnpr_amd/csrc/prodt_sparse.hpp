// prodt_sparse.hpp — the decode of k_prodT's sparse form (matvec.hip): one dword of the sample-major image (16 variants
// of one sample, variant e in bits 2e, 2e+1; code 3 = missing) becomes the A operand of ONE
// v_smfmac_i32_16x16x128_i8 — 16 compressed int8 values and a 32-bit index register.  Shared by the kernel, by
// tools/ubench/smfmac_parts.hip and by the CPU statement (tests/native/prodt_sparse_ref.cpp): the three cannot drift apart.
//
// The product adds, per genotype, code x A-digits for a present value and 1 x B-digits for a missing one (A the image of
// w_j, B of c_j w_j, k_quant mode 1): of the pair (code term, missing term) at most one is non-zero.  Interleaved along K
// as (A_e, B_e, A_e', B_e') every group of four dense K holds at most two non-zeros, which is the 2:4 pattern of the
// instruction for EVERY input.  Compressed value e is the code (0, 1, 2; 1 for a missing value), its 2-bit index
// 2 (e & 1) + missing: the first value of a group selects slot 0 / 1, the second slot 2 / 3 — distinct and ascending
// (the instruction, as measured, asks for neither).
// The values are in the variants' natural order, so the index is a mask of the dword itself.
//
// 18 VALU per dword as compiled: 6 for index and codes, and per byte of codes a multiply by 0x1001 (b | b << 12: two 8-bit
// copies that do not overlap), a shift-or by 6 and a mask (the compiler makes it two multiplies and one v_bitop3).
// (ONE multiply by 0x041041 would add the four shifted copies of the byte at once, but the copies overlap by two bits,
// and codes 2 in the first and the fourth field of a byte then carry into the second field's byte: 0b10 + 0b10 at bits
// 6, 7.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BSN_SPARSE_HD __host__ __device__ __forceinline__
#else
#define BSN_SPARSE_HD inline
#endif

namespace bsn {

// a[r]: compressed values of variants 4r .. 4r+3 (byte i = variant 4r + i); idx: bits 2e, 2e+1 = index of value e
BSN_SPARSE_HD void prodt_sparse_decode(const uint32_t w, uint32_t (&a)[4], uint32_t &idx) {
  const uint32_t miss = (w & (w >> 1)) & 0x55555555u;   // bit 2e: variant e is missing
  idx = miss | 0x88888888u;
  const uint32_t v = w ^ (miss << 1);                    // code 3 -> 1
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint32_t x = ((v >> (8 * r)) & 0xFFu) * 0x1001u;   // (an SDWA byte select on the device)
    a[r] = ((x << 6) | x) & 0x03030303u;
  }
}

// The digits that go with it: the 32 dense K of a dword are (A_e, B_e) of its 16 variants, dense K 2e + p.  In the
// digit panel (k_quant, PERM = 2) the 16-byte row of "plane" h holds variants 8h .. 8h+7: byte 2 (e & 7) + p of row e >> 3.
// (Which lane of the B operand reads which row is the instruction's layout, measured by tools/ubench/smfmac_parts.hip:
// the compressed values of lane group ga are dense K 32 ga .. 32 ga + 31, and register half h of lane group gb of B is
// dense K 64 h + 16 gb .. + 15 — k_prodT's xrow.)
BSN_SPARSE_HD int prodt_sparse_row(const int e) { return e >> 3; }
BSN_SPARSE_HD int prodt_sparse_byte(const int e, const int p) { return 2 * (e & 7) + p; }

}  // namespace bsn
