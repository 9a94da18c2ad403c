// Host statement of k_prodT's sparse form over bigsnpr_amd/csrc/prodt_sparse.hpp (the header the kernel compiles):
// the decode of a genotype dword, and "compressed values + index x interleaved digits" as the instruction defines it.
#include <stdint.h>

#include "prodt_sparse.hpp"

extern "C" {

// a: 4 dwords per input dword, idx: one
void pts_decode(const uint32_t *w, int64_t n, uint32_t *a, uint32_t *idx) {
  for (int64_t i = 0; i < n; i++) {
    uint32_t av[4];
    bsn::prodt_sparse_decode(w[i], av, idx[i]);
    for (int r = 0; r < 4; r++) a[4 * i + r] = av[r];
  }
}

// One lane group of v_smfmac_i32_16x16x128_i8 on the operands the kernel builds: the 16 variants of dword w against
// their digits dA[e], dB[e] (one digit slice of A and of B).  The B operand is written through prodt_sparse_row /
// prodt_sparse_byte (32 bytes: two rows of 16); compressed value p with index iv multiplies dense K 4 (p / 2) + iv.
// Returns the sum; *legal = 0 if a group's two indices are not distinct and ascending.
int64_t pts_dot(uint32_t w, const int8_t *dA, const int8_t *dB, int *legal) {
  int8_t b[32];
  for (int e = 0; e < 16; e++) {
    b[16 * bsn::prodt_sparse_row(e) + bsn::prodt_sparse_byte(e, 0)] = dA[e];
    b[16 * bsn::prodt_sparse_row(e) + bsn::prodt_sparse_byte(e, 1)] = dB[e];
  }
  uint32_t a[4], idx;
  bsn::prodt_sparse_decode(w, a, idx);
  int64_t s = 0;
  *legal = 1;
  for (int p = 0; p < 16; p++) {
    const int iv = (idx >> (2 * p)) & 3;
    s += (int64_t)(int8_t)(a[p / 4] >> (8 * (p & 3))) * b[4 * (p / 2) + iv];
    if ((p & 1) && iv <= (int)((idx >> (2 * (p - 1))) & 3)) *legal = 0;
  }
  return s;
}

}  // extern "C"
