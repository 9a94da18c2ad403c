// inflate_fuzz.cpp — a stand-alone program over inflate_step.hpp, meant to be compiled with -fsanitize=address,undefined
// and run as a program (tests/test_inflate_cpu.py does both).  It reads a file of streams
//   uint32 count, then per stream: uint32 in_len, uint32 out_cap, uint32 expected_len, int32 status (-1: any), the bytes
// runs each of them with buffers of exactly in_len and out_cap bytes, checks the status where one is given, and then
// runs 2000 single-bit and single-byte mutations (fixed seed) of the streams whose status is 0.  Every call must come
// back with a status between 0 and 7; the sanitizers see every read and write.  Exit status 0 = all of that held.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "inflate_step.hpp"

struct Stream {
  std::vector<uint8_t> in;
  uint32_t cap, expected;
  int32_t status;
};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rng() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static int run(const std::vector<uint8_t> &in, uint32_t cap, uint32_t expected) {
  uint8_t *a = new uint8_t[in.size() ? in.size() : 1];   // exactly in_len bytes (one when empty: never read)
  if (!in.empty()) memcpy(a, in.data(), in.size());
  uint8_t *o = new uint8_t[cap ? cap : 1];
  const int st = bsn::inflate::inflate_stream(a, (int64_t)in.size(), o, (int64_t)cap, (int64_t)expected);
  delete[] a;
  delete[] o;
  return st;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  std::vector<Stream> all(count);
  for (auto &s : all) {
    uint32_t h[4];
    if (fread(h, 4, 4, f) != 4) return 2;
    s.in.resize(h[0]);
    s.cap = h[1], s.expected = h[2], s.status = (int32_t)h[3];
    if (h[0] && fread(s.in.data(), 1, h[0], f) != h[0]) return 2;
  }
  fclose(f);
  int failures = 0;
  std::vector<size_t> good;
  for (size_t k = 0; k < all.size(); k++) {
    const int st = run(all[k].in, all[k].cap, all[k].expected);
    if (st < 0 || st > 7 || (all[k].status >= 0 && st != all[k].status)) {
      printf("stream %zu: status %d, expected %d\n", k, st, all[k].status);
      failures++;
    }
    if (all[k].status == 0 && !all[k].in.empty()) good.push_back(k);
  }
  int hist[8] = {0};
  for (int t = 0; t < 2000 && !good.empty(); t++) {
    const Stream &s = all[good[rng() % good.size()]];
    std::vector<uint8_t> in = s.in;
    const size_t at = rng() % in.size();
    if (t & 1)
      in[at] ^= (uint8_t)(1u << (rng() % 8));
    else
      in[at] = (uint8_t)rng();
    const int st = run(in, s.cap, s.expected);
    if (st < 0 || st > 7) {
      printf("mutation %d: status %d\n", t, st);
      failures++;
    } else {
      hist[st]++;
    }
  }
  printf("streams %zu, mutations by status:", all.size());
  for (int k = 0; k < 8; k++) printf(" %d", hist[k]);
  printf("\nfailures %d\n", failures);
  return failures ? 1 : 0;
}
