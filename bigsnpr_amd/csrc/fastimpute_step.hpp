// fastimpute_step.hpp — the statement of snp_fastImpute for one target variant (R/impute.R:29-160 of the reference, with
// xgboost's exact greedy tree rule written out): who trains and who validates, the starting margin, the quantised
// gradients of a round, the scan of one feature's candidates at one node with its tie rule, the leaf weight, the
// routing of a sample and the call a margin gives.  Shared by the kernels (fastimpute.hip), the CPU statement
// (tests/native/fastimpute_ref.cpp) and the stand-alone check (tests/native/fastimpute_check.cpp): the three cannot
// drift apart.  DESIGN.md 3.5q.
//
// Bit equality of host and device.  exp and log are gibbs_step.hpp's (no libm), every fp64 operation is rounded on its
// own (the pragma below on the device, -ffp-contract=off on the host), and every SUM over samples is a sum of int64:
// gradients and hessians are quantised to multiples of 2^-30 before they are added, so a histogram is the same integers
// in any order of summation, on any number of lanes.  A sum enters fp64 as (double)sum * 2^-30.
#pragma once
#include <stdint.h>

#include "impute_step.hpp"

namespace bsn {
namespace fimp {

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// the parameters the reference passes to xgboost (R/impute.R:66-75): binary:logistic, max_depth 4, 10 rounds, eta 0.3,
// lambda 1, gamma 0, min_child_weight 1
constexpr int kRounds = 10;
constexpr int kMaxDepth = 4;                       // a node at this depth is a leaf
constexpr int kNodes = (2 << kMaxDepth) - 1;       // heap numbering: root 0, children 2 k + 1 and 2 k + 2
constexpr int kLevelNodes = 1 << (kMaxDepth - 1);  // most nodes that can split at one level
constexpr double kEta = 0.3;
constexpr double kLambda = 1.0;
constexpr double kMinChildWeight = 1.0;
constexpr double kMinLossChg = 1e-6;
constexpr double kQuant = 1073741824.0;              // 2^30
constexpr double kUnquant = 9.313225746154785e-10;   // 2^-30

// third word of the Philox counter of the training split ("FIMP")
constexpr uint32_t kCounterTag = 0x46494D50u;

// roles of a sample of the target variant
constexpr int kTrain = 0, kValid = 1, kFill = 2;

// is observed sample i of target j a training sample?  One Philox call: key = seed, counter = (i, j, tag, high halves).
BSN_IMPUTE_HD bool draws_train(uint64_t seed, uint64_t i, uint64_t j, double p_train) {
  const gibbs::Philox o = gibbs::philox4x32_10((uint32_t)i, (uint32_t)j, kCounterTag,
                                               (uint32_t)(i >> 32) ^ ((uint32_t)(j >> 32) << 16), (uint32_t)seed,
                                               (uint32_t)(seed >> 32));
  return gibbs::unit_open(o.v[0], o.v[1]) < p_train;
}

// the margin every sample starts from: c1, c2 calls 1 and 2 among the T training samples
BSN_IMPUTE_HD double start_margin(int64_t c1, int64_t c2, int64_t T) {
  double base = (0.5 * (double)c1 + (double)c2) / (double)T;
  if (base < 1e-7) base = 1e-7;
  if (base > 1.0 - 1e-7) base = 1.0 - 1e-7;
  return gibbs::log_det(base) - gibbs::log_det(1.0 - base);
}

BSN_IMPUTE_HD double prob(double margin) { return 1.0 / (1.0 + gibbs::exp_det(-margin)); }

// gradient and hessian of the logistic loss at `margin` for the call `code` (label code / 2), in units of 2^-30
BSN_IMPUTE_HD void grad(double margin, int code, int32_t *gq, int32_t *hq) {
  const double p = prob(margin);
  const double g = p - 0.5 * (double)code;
  double h = p * (1.0 - p);
  if (h < 1e-16) h = 1e-16;
  *gq = (int32_t)impute::round_even(g * kQuant);
  const int32_t q = (int32_t)impute::round_even(h * kQuant);
  *hq = q < 1 ? 1 : q;
}

BSN_IMPUTE_HD int call_of(double margin) { return (int)impute::round_even(2.0 * prob(margin)); }

BSN_IMPUTE_HD double real(int64_t sum) { return (double)sum * kUnquant; }

BSN_IMPUTE_HD double gain(int64_t G, int64_t H) {
  const double g = real(G), h = real(H);
  return g * g / (h + kLambda);
}

BSN_IMPUTE_HD double leaf_weight(int64_t G, int64_t H) { return kEta * (-real(G) / (real(H) + kLambda)); }

// does a sample whose feature has `code` (3 = missing) go left at threshold t + 0.5 (t = 0, 1, 2)?
BSN_IMPUTE_HD bool goes_left(int code, int t, int dir) { return code == 3 ? dir == 1 : code <= t; }

// the best split of a node so far; feat < 0: none, the node is a leaf.  GL, HL: the sums of its left child.
struct Best {
  double chg;
  int32_t feat, t, dir;
  int64_t GL, HL;
};

BSN_IMPUTE_HD Best no_split() {
  Best b;
  b.chg = kMinLossChg;   // a split has to exceed this
  b.feat = -1, b.t = 0, b.dir = 0;
  b.GL = 0, b.HL = 0;
  return b;
}

// The six candidates of feature position `feat` at a node with sums G, H, in the order (t, dir); gc / hc: the node's
// sums over its training samples whose feature has code 0, 1, 2, missing.  A candidate replaces `b` only when it is
// strictly better, so with features scanned in ascending position the smallest (feat, t, dir) wins among equals.
BSN_IMPUTE_HD void scan_feature(const int64_t gc[4], const int64_t hc[4], int64_t G, int64_t H, int32_t feat, Best *b) {
  const double node = gain(G, H);
  int64_t gl = 0, hl = 0;
  for (int t = 0; t < 3; t++) {
    gl += gc[t];
    hl += hc[t];
    for (int dir = 0; dir < 2; dir++) {
      const int64_t GL = dir ? gl + gc[3] : gl, HL = dir ? hl + hc[3] : hl;
      const int64_t GR = G - GL, HR = H - HL;
      if (!(real(HL) >= kMinChildWeight && real(HR) >= kMinChildWeight)) continue;
      const double chg = (gain(GL, HL) + gain(GR, HR)) - node;
      if (chg > b->chg) {
        b->chg = chg;
        b->feat = feat, b->t = t, b->dir = dir;
        b->GL = GL, b->HL = HL;
      }
    }
  }
}

// b of a later feature against a of an earlier one (the merge of a parallel search)
BSN_IMPUTE_HD bool better(const Best &b, const Best &a) { return b.chg > a.chg; }

#if defined(__clang__)
#pragma clang fp contract(on)
#endif

}  // namespace fimp
}  // namespace bsn
