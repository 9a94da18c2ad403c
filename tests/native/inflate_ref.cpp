// inflate_ref.cpp — the CPU statement of bsn_inflate: inflate_step.hpp, the header k_inflate is compiled from, with its
// serial sink, over K independent streams (OpenMP over streams when the compiler has it).  tests/native/bgen_ref.py builds
// it with -ffp-contract=off; tests/test_inflate_cpu.py holds it against zlib.decompress, tests/test_gpu_bgen.py holds the
// device against it.
#include <stdint.h>

#include "inflate_step.hpp"

extern "C" {

// one stream; room and expected length given apart
int inflate_one_ref(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_cap, int64_t expected_len) {
  return bsn::inflate::inflate_stream(in, in_len, out, out_cap, expected_len);
}

// the signature of bsn_inflate: the room of a stream is also its expected length
void inflate_ref(const uint8_t *in, const int64_t *in_off, int64_t K, uint8_t *out, const int64_t *out_off, int32_t *status,
                 int nthreads) {
#if defined(_OPENMP)
#pragma omp parallel for schedule(dynamic) num_threads(nthreads > 0 ? nthreads : 1)
#endif
  for (int64_t k = 0; k < K; k++) {
    const int64_t cap = out_off[k + 1] - out_off[k];
    status[k] = bsn::inflate::inflate_stream(in + in_off[k], in_off[k + 1] - in_off[k], out + out_off[k], cap, cap);
  }
  (void)nthreads;
}

}  // extern "C"
