// impute_check.cpp — a stand-alone program over impute_step.hpp: the mode rule and its ties, the two roundings where the
// double operations and the exact rational part ways, the draw, a variant without any call, and the rewrite of packed
// 2-bit columns whose sample count is no multiple of 4 or 16.  Meant to be compiled with -fsanitize=address,undefined and
// run as a program (tests/test_impute_cpu.py does both).  Exit status 0 = every check held.
#include <stdio.h>

#include <vector>

#include "impute_step.hpp"

using namespace bsn::impute;

static int failures = 0;
#define CHECK(cond)                                          \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAILED line %d: %s\n", __LINE__, #cond);       \
      failures++;                                            \
    }                                                        \
  } while (0)

static void mode_rule() {
  CHECK(mode_call(5, 3, 1) == 0 && mode_call(3, 5, 1) == 1 && mode_call(1, 3, 5) == 2 && mode_call(3, 1, 5) == 2);
  CHECK(mode_call(4, 4, 2) == 0);   // c0 == c1 > c2
  CHECK(mode_call(2, 4, 4) == 1);   // c1 == c2 > c0
  CHECK(mode_call(4, 2, 4) == 0);   // c0 == c2 > c1
  CHECK(mode_call(3, 3, 3) == 0);   // all equal
  CHECK(mode_call(0, 0, 0) == 0);   // no call at all
  CHECK(rule(kMode, 8, 0, 191).val == 0 && rule(kMode, 112, 44, 198).val == 1);
}

// c1, c2 with c1 + 2 c2 = s and c1 + c2 <= c
static Rule mean_rule(int method, int64_t c, int64_t s) {
  const int64_t c2 = s > c ? s - c : 0, c1 = s - 2 * c2;
  CHECK(c1 >= 0 && c1 + c2 <= c);
  return rule(method, c1, c2, c);
}

static void rounding() {
  CHECK(mean_rule(kMean2, 40, 23).val == 57);    // 100 * (23.0 / 40) = 57.49999999999999; the exact tie would give 58
  CHECK(mean_rule(kMean2, 40, 49).val == 123);   // 122.50000000000001; the exact tie would give 122
  CHECK(mean_rule(kMean2, 40, 51).val == 127);   // 127.49999999999999; the exact tie would give 128
  CHECK(mean_rule(kMean2, 8, 1).val == 12);      // exactly 12.5: ties to even, not half up
  CHECK(mean_rule(kMean2, 8, 5).val == 62);      // exactly 62.5
  CHECK(mean_rule(kMean0, 2, 1).val == 0);       // 0.5 -> 0
  CHECK(mean_rule(kMean0, 2, 3).val == 2);       // 1.5 -> 2
  CHECK(rule(kMean0, 112, 44, 198).val == 1 && rule(kMean2, 112, 44, 198).val == 101);
  CHECK(rule(kMean2, 0, 0, 5).val == 0 && rule(kMean2, 0, 5, 5).val == 200);
  CHECK(fbm_byte(kMean2, 101) == 108 && fbm_byte(kMean0, 1) == 5 && fbm_byte(kMode, 2) == 6 && fbm_byte(kRandom, 0) == 4);
  CHECK(fbm_byte(kZero, 0) == 3 && fbm_byte(kMean2, -1) == 3);
  CHECK(grid_index(0) == -100 && grid_index(200) == 100 && grid_index(-1) == -128);
}

static void no_call() {
  CHECK(rule(kZero, 0, 0, 0).val == 0 && rule(kMode, 0, 0, 0).val == 0);
  for (int method : {kMean0, kMean2, kRandom}) {
    const Rule r = rule(method, 0, 0, 0);
    CHECK(r.val == -1 && r.af == 0.0);
    CHECK(fbm_byte(method, r.val) == 3);
  }
}

static void draws() {
  const uint64_t seed = 0x9E3779B97F4A7C15ull;
  CHECK(rule(kRandom, 2, 1, 4).af == 0.5);
  int hist[3] = {0, 0, 0}, same = 0;
  for (uint64_t i = 0; i < 4000; i++) {
    const int d = draw(seed, i, 7, 0.25);
    CHECK(d >= 0 && d <= 2);
    if (d >= 0 && d <= 2) hist[d]++;
    CHECK(d == draw(seed, i, 7, 0.25));                 // a function of (seed, i, j, af)
    same += d == draw(seed, i, 8, 0.25);
    CHECK(draw(seed, i, 7, 0.0) == 0 && draw(seed, i, 7, 1.0) == 2);   // u lies in the open interval
  }
  // Binomial(2, 1/4): 2250 / 1500 / 250 expected of 4000; eight standard deviations of slack
  CHECK(hist[0] > 2000 && hist[0] < 2500 && hist[1] > 1250 && hist[1] < 1750 && hist[2] > 130 && hist[2] < 370);
  CHECK(same < 3600);   // another variant, other draws (equal by chance 0.47 of the time)
  CHECK(draw(seed, 5, (1ull << 32) + 7, 0.5) >= 0 && draw(seed, (1ull << 32) + 5, 7, 0.5) >= 0);
}

// a packed column of n samples in the device coding, pad fields zero; code(i) gives sample i
template <class F>
static std::vector<uint32_t> pack(int64_t n, F code) {
  std::vector<uint32_t> w((size_t)((n + 15) / 16), 0u);
  for (int64_t i = 0; i < n; i++) w[(size_t)(i / 16)] |= (uint32_t)code(i) << (2 * (i % 16));
  return w;
}
static int field(const std::vector<uint32_t> &w, int64_t i) { return (int)((w[(size_t)(i / 16)] >> (2 * (i % 16))) & 3u); }

static void packed_columns() {
  for (int64_t n : {1, 3, 5, 17, 31, 67}) {   // no multiple of 4, none of 16
    auto code = [n](int64_t i) { return (i == 0 || i == n - 1 || i % 5 == 2) ? 3 : (int)(i % 3); };
    const std::vector<uint32_t> src = pack(n, code);
    for (uint32_t v = 0; v < 3; v++) {
      std::vector<uint32_t> dst(src.size());
      for (size_t k = 0; k < src.size(); k++) dst[k] = fill_word(src[k], v);
      for (int64_t i = 0; i < 16 * (int64_t)src.size(); i++) {
        if (i >= n) CHECK(field(dst, i) == 0);                       // pad fields stay zero
        else CHECK(field(dst, i) == (code(i) == 3 ? (int)v : code(i)));
      }
    }
    const uint64_t seed = 42;
    std::vector<uint32_t> dst(src.size());
    for (size_t k = 0; k < src.size(); k++) dst[k] = fill_word_random(src[k], seed, 16 * (uint64_t)k, 3, 0.4);
    for (int64_t i = 0; i < 16 * (int64_t)src.size(); i++) {
      if (i >= n) CHECK(field(dst, i) == 0);
      else CHECK(field(dst, i) == (code(i) == 3 ? draw(seed, (uint64_t)i, 3, 0.4) : code(i)));
    }
  }
  CHECK(missing_mask(0xFFFFFFFFu) == 0x55555555u && missing_mask(0xAAAAAAAAu) == 0 && missing_mask(0x55555555u) == 0);
  CHECK(fill_word(0xFFFFFFFFu, 2) == 0xAAAAAAAAu && fill_word(0xFFFFFFFFu, 0) == 0);
}

int main() {
  mode_rule();
  rounding();
  no_call();
  draws();
  packed_columns();
  printf(failures ? "%d checks failed\n" : "all checks held\n", failures);
  return failures ? 1 : 0;
}
