// hwe_step.hpp — the exact test of Hardy–Weinberg equilibrium of one variant (Wigginton, Cutler & Abecasis 2005; what
// PLINK's --hwe / --hardy compute) and the comparisons of the quality-control filters of bed_plinkQC (--mind, --geno,
// --maf, --hwe).  Shared by the kernels (qc.hip) and the CPU statement (tests/native/hwe_ref.cpp): the two cannot drift
// apart.  DESIGN.md 3.5o.
//
// The test.  Given N = hom1 + het + hom2 genotypes with rare = 2 min(hom1, hom2) + het copies of the rarer allele, the
// number of heterozygotes h has P(h) proportional to 2^h / (homr! h! homc!), homr = (rare - h) / 2 and
// homc = N - h - homr the rarer and the commoner homozygote.  The p-value is the sum of the P(h) that do not exceed the
// observed one over the sum of all.  No array of terms exists: the observed term is 1, one walk goes DOWN from it
//   term(h - 2) = term(h) * h (h - 1) / (4 (homr + 1) (homc + 1)),
// a separate walk goes UP
//   term(h + 2) = term(h) * 4 homr homc / ((h + 2) (h + 1)),
// homr and homc following h.  Each walk adds every term to its own total and, when term <= 1 + kTie, to its own tail
// (kTie guards ties against rounding, as PLINK 1.9 does; a rule of this statement).  With midp a term within kTie of 1
// adds half of itself, and so does the observed one.  A walk ends when h would leave [rare mod 2, rare], when its term
// falls below DBL_MIN (what remains is below 1e-307 of the observed term) or when it reaches inf.
//   p = ((1 or 0.5) + tail_down + tail_up) / (1 + total_down + total_up), at most 1;
// an infinite sum gives p = 0 (the true value is then below about 1e-300).  N = 0: NaN; rare = 0: 1.
//
// Bit equality of host and device.  h, homr and homc are held as doubles (integers below 2^53, exact); a step is the
// numerator product, the denominator product, ONE division, one multiplication and the additions, each correctly rounded
// on both sides and never contracted (the pragma below on the device, -ffp-contract=off on the host).  The two walks are
// separate accumulations combined in a fixed order, so a variant may be given one lane or two without changing a bit.
#pragma once
#include <stdint.h>

#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#define BSN_HWE_HD __host__ __device__ __forceinline__
#else
#define BSN_HWE_HD inline
#endif

namespace bsn {
namespace hwe {

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

constexpr double kTie = 1e-8;

struct Walk {
  double total, tail;
  int64_t steps;
};

// a term other than the observed one into a walk's sums
BSN_HWE_HD void add_term(Walk &w, double term, bool midp) {
  w.total = w.total + term;
  if (midp && fabs(term - 1.0) <= kTie)
    w.tail = w.tail + 0.5 * term;
  else if (term <= 1.0 + kTie)
    w.tail = w.tail + term;
}

// the terms of h = het - 2, het - 4, ...
BSN_HWE_HD Walk walk_down(double het, double homr, double homc, bool midp) {
  Walk w = {0.0, 0.0, 0};
  double term = 1.0, h = het;
  while (h >= 2.0) {
    const double num = h * (h - 1.0);
    const double den = (4.0 * (homr + 1.0)) * (homc + 1.0);
    term = term * (num / den);
    if (term < DBL_MIN) break;
    h = h - 2.0;
    homr = homr + 1.0;
    homc = homc + 1.0;
    w.steps++;
    add_term(w, term, midp);
    if (!(term <= DBL_MAX)) break;
  }
  return w;
}

// the terms of h = het + 2, het + 4, ... up to rare
BSN_HWE_HD Walk walk_up(double het, double homr, double homc, double rare, bool midp) {
  Walk w = {0.0, 0.0, 0};
  double term = 1.0, h = het;
  while (h <= rare - 2.0) {
    const double num = (4.0 * homr) * homc;
    const double den = (h + 2.0) * (h + 1.0);
    term = term * (num / den);
    if (term < DBL_MIN) break;
    h = h + 2.0;
    homr = homr - 1.0;
    homc = homc - 1.0;
    w.steps++;
    add_term(w, term, midp);
    if (!(term <= DBL_MAX)) break;
  }
  return w;
}

// what the walks start from: N, rare, homr, homc as doubles.  ok: a test exists (counts not negative, N > 0, rare > 0);
// otherwise `fixed` is the result (NaN or 1).
struct Start {
  double het, homr, homc, rare, fixed;
  bool ok;
};

BSN_HWE_HD Start start(int32_t hom1, int32_t het, int32_t hom2) {
  Start s;
  const int64_t N = (int64_t)hom1 + het + hom2;
  const int64_t lo = hom1 < hom2 ? hom1 : hom2, hi = hom1 < hom2 ? hom2 : hom1;
  s.het = (double)het;
  s.homr = (double)lo;
  s.homc = (double)hi;
  s.rare = (double)(2 * lo + het);
  s.ok = false;
  if (hom1 < 0 || het < 0 || hom2 < 0 || N == 0)
    s.fixed = NAN;
  else if (2 * lo + het == 0)
    s.fixed = 1.0;
  else
    s.ok = true, s.fixed = 0.0;
  return s;
}

BSN_HWE_HD double combine(const Walk &down, const Walk &up, bool midp) {
  const double tail = ((midp ? 0.5 : 1.0) + down.tail) + up.tail;
  const double total = (1.0 + down.total) + up.total;
  if (!(total <= DBL_MAX)) return 0.0;
  const double p = tail / total;
  return p > 1.0 ? 1.0 : p;
}

// the p-value of one variant; steps (may be NULL): the number of terms the two walks formed
BSN_HWE_HD double hwe_exact(int32_t hom1, int32_t het, int32_t hom2, bool midp, int64_t *steps = nullptr) {
  if (steps) *steps = 0;
  const Start s = start(hom1, het, hom2);
  if (!s.ok) return s.fixed;
  const Walk down = walk_down(s.het, s.homr, s.homc, midp);
  const Walk up = walk_up(s.het, s.homr, s.homc, s.rare, midp);
  if (steps) *steps = down.steps + up.steps;
  return combine(down, up, midp);
}

// ---- the filters of bed_plinkQC: every comparison is one double expression ---------------------------------------------
// a sample with `na` missing calls among m variants (--mind), a variant with `na` missing calls among n samples (--geno)
BSN_HWE_HD bool too_many_missing(int64_t na, int64_t of, double rate) { return (double)na > rate * (double)of; }
BSN_HWE_HD double missing_rate(int64_t na, int64_t of) { return (double)na / (double)of; }

// minor allele frequency from the counts of 0, 1, 2; no call: NaN
BSN_HWE_HD double maf_from_counts(int64_t c0, int64_t c1, int64_t c2) {
  const int64_t a = c1 + 2 * c2, b = c1 + 2 * c0;
  return (double)(a < b ? a : b) / (double)(2 * (c0 + c1 + c2));
}
// (a NaN frequency fails every active threshold)
BSN_HWE_HD bool maf_too_low(double maf_j, double maf) { return maf > 0.0 && !(maf_j >= maf); }
BSN_HWE_HD bool hwe_rejected(double p, double hwe) { return hwe > 0.0 && p < hwe; }

#if defined(__clang__)
#pragma clang fp contract(on)
#endif

}  // namespace hwe
}  // namespace bsn
