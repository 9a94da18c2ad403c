// ldsplit_step.hpp — the per-element rules of snp_ldsplit (R/split-LD.R, src/split-LD.cpp of the reference): how one stored
// entry of `corr` enters a column's suffix sum, how a partial sum of E is rounded, and the order in which two candidates
// of the recurrence compare.  Shared by the kernels (ldsplit.hip) and by the CPU statement (tests/native/ldsplit_ref.cpp):
// the two cannot drift apart.
//
// Bit equality of host and device.  x * x is rounded before it is added (no contraction: the pragma below on the device,
// -ffp-contract=off on the host); every other operation is one fp64 addition, one fp64 -> fp32 -> fp64 round trip or a
// comparison.  Sums of squared block sizes are integers far below 2^53.
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#define BSN_LDSPLIT_HD __host__ __device__ __forceinline__
#else
#define BSN_LDSPLIT_HD inline
#endif

namespace bsn {
namespace ldsplit {

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

BSN_LDSPLIT_HD double inf() { return __builtin_huge_val(); }

// The running sum l of a column, walked from its last stored entry towards the diagonal, after the entry x: r2 = x * x
// counts when r2 >= thr_r2 (a NaN fails the comparison and is ignored), and r2 > max_r2 forbids every split that would
// put the two variants into different blocks.
BSN_LDSPLIT_HD double take_entry(double l, double x, double thr_r2, double max_r2) {
  const double r2 = x * x;
  if (r2 >= thr_r2) {
    if (r2 > max_r2) l = inf();
    else l = l + r2;
  }
  return l;
}

// a partial sum of E is kept as a float
BSN_LDSPLIT_HD float keep(double e) { return (float)e; }

// A candidate of row `row` at one level: the block row .. col, followed by the best k - 1 blocks from col + 1 on.
// col = -1 is "none": what best_ind reports as NA.
struct Cand {
  double c1, c2;
  int32_t col;
};

BSN_LDSPLIT_HD Cand none() { return Cand{inf(), inf(), -1}; }

// e: the stored float E(row, col); p1, p2: C1 and C2 of row col + 1 at the previous level (+Inf for col + 1 = m).
// A candidate that does not compare below (Inf, Inf) replaces nothing in the sequential loop: it is "none".
BSN_LDSPLIT_HD Cand candidate(float e, double p1, double p2, int32_t row, int32_t col) {
  const double size = (double)(col - row + 1);
  Cand c;
  c.c1 = (double)e + p1;
  c.c2 = size * size + p2;
  c.col = col;
  if (!(c.c1 < inf()) && !(c.c2 < inf())) c = none();
  return c;
}

// The sequential loop visits col from m - 1 downwards, replaces on cost1 <, and on cost1 == only when cost2 <: it keeps
// the lexicographic minimum of (cost1, cost2), exact ties going to the largest col.  As an order on candidates this is
// associative and commutative, so partial minima may be combined in any grouping.
BSN_LDSPLIT_HD bool better(const Cand &a, const Cand &b) {
  if (a.c1 < b.c1) return true;
  if (a.c1 > b.c1) return false;
  if (a.c2 < b.c2) return true;
  if (a.c2 > b.c2) return false;
  return a.col > b.col;
}

// the early stop behind level k: C1(0, k) is beyond max_cost and no better than the level before
BSN_LDSPLIT_HD bool stop_after(double c_k, double c_prev, double max_cost) { return c_k > max_cost && c_k > c_prev; }

// K blocks are reported when their cost is within max_cost and a path exists
BSN_LDSPLIT_HD bool reported(double cost, int32_t first_best, double max_cost) { return cost <= max_cost && first_best >= 0; }

#if defined(__clang__)
#pragma clang fp contract(on)
#endif

}  // namespace ldsplit
}  // namespace bsn
