// knn_plan.hpp — the launch geometry of the nearest-neighbour scan (knn.hip: k_knn_scan, k_knn_merge), decided from plain
// facts.  No HIP in here: tests/native/knn_ref.cpp compiles it as it stands and tests/test_knn_cpu.py pins the choices on
// the CPU, like prod_plan.hpp.
//
// One lane holds one query; a workgroup holds a block of `qb` queries, as many as its lists of k (squared distance, index)
// pairs leave room for in LDS beside the data tile.  A query set whose blocks alone do not cover the compute units is
// scanned in S slabs of data points — the grid is blocks x S — and a merge kernel takes the k smallest of the S sorted
// partial lists of every query, by the same total order: the result does not depend on S (knn_step.hpp).
#pragma once
#include <algorithm>
#include <cstdint>

namespace bsn {
namespace knn {

constexpr int kTile = 32;                              // data points per LDS tile of the scan
constexpr int kListBytes = 12;                         // one place of a list: a double and an int32
constexpr int kLdsBytes = 64 * 1024;                   // LDS of one workgroup
constexpr int64_t kMinSlabPoints = 128;                // the planner's own rule cuts no slab shorter than this
constexpr int64_t kPartialCap = (int64_t)256 << 20;    // bytes of the partial lists (nq * S * k * 12) at most
constexpr int64_t kMaxSlabs = 1024;                    // S at most, forced or not

// coordinates as the scan holds them: p rounded up to a multiple of 4 with zero coordinates (they change no bit of a
// squared distance: knn_step.hpp, step)
inline int padded_p(int p) { return (p + 3) / 4 * 4; }

// queries of one workgroup: 256, 128 or 64 — the most whose lists fit the LDS beside a tile of 32 points of 64 coordinates
inline int query_block(int k) {
  const int tile = kTile * 64 * 8;
  for (int qb = 256; qb > 64; qb /= 2)
    if (qb * k * kListBytes + tile <= kLdsBytes) return qb;
  return 64;
}

struct Plan {
  int qb = 64;            // queries per workgroup
  int64_t nqb = 0;        // query blocks
  int S = 1;              // slabs of data points; 1: no partial lists, no merge
  int64_t n = 0;
  // slab s covers the data points lo(s) .. lo(s + 1) - 1: all of 0 .. n, no overlap, none empty (S <= n)
  int64_t lo(int s) const { return n * (int64_t)s / S; }
  int64_t partial_bytes(int64_t nq, int k) const { return S > 1 ? nq * (int64_t)S * k * kListBytes : 0; }
};

// forced >= 1: the slab count asked for (BSN_KNN_SLABS); below 1: the rule — blocks x S covers the compute units, no slab
// shorter than kMinSlabPoints.  Either way S is at most n and kMaxSlabs, and the partial lists stay within
// kPartialCap.
inline Plan plan(int64_t n, int64_t nq, int k, int ncu, int64_t forced) {
  Plan P;
  P.n = n;
  P.qb = query_block(k);
  P.nqb = (nq + P.qb - 1) / P.qb;
  int64_t S;
  if (forced >= 1) {
    S = forced;
  } else {
    S = P.nqb >= ncu ? 1 : (ncu + P.nqb - 1) / P.nqb;
    S = std::min<int64_t>(S, std::max<int64_t>(1, n / kMinSlabPoints));
  }
  S = std::min<int64_t>(S, std::max<int64_t>(1, kPartialCap / (nq * (int64_t)k * kListBytes)));
  S = std::min<int64_t>(std::min<int64_t>(S, n), kMaxSlabs);
  P.S = (int)std::max<int64_t>(S, 1);
  return P;
}

}  // namespace knn
}  // namespace bsn
