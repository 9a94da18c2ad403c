// qp_step.hpp — ancestry proportions from allele frequencies (Privé 2022; snp_ancestry_summary, R/ancestry-summary.R:31-74
// of the reference): the quadratic program behind it for ONE frequency vector, the correlations it reports, and the row
// slabs of the moment pass.  Shared by the kernels (ancestry.hip) and the CPU statement (tests/native/ancestry_ref.cpp):
// the two cannot drift apart.  DESIGN.md 3.5s.  quadprog::solve.QP, which the reference calls, is external to its tree:
// parity with its numbers is not pinned, the minimiser (unique: D is positive definite) is.
//
// The problem.   minimise  1/2 w'D w - d'w   over w in R^K
//                subject to  w_k >= 0 for all k,   and   sum w = 1 (sum_to_one)   or   sum w <= 1 (otherwise)
// D (K x K, symmetric positive definite) is shared by every problem of a call; d differs per problem.  The constraints
// are numbered 0: -sum w >= -1 (normal -1, an equality when sum_to_one) and k + 1: w_k >= 0 (normal e_k).
//
// The method: the dual active-set method of Goldfarb & Idnani (Math. Programming 27, 1983), exact and finite.
//   Once per call (factor(), host): D = L L' (Cholesky) and J0 = L^-T, so that D^-1 = J0 J0'.
//   State: x; the active set A (q constraints, in the order they were added) with multipliers u; J (K x K) and R (q x q,
//   upper triangular) with J'N = [R; 0], N the active normals, and J J' = D^-1.  Start: x = J0 J0'd (the unconstrained
//   minimiser), A empty, J = J0.
//   Step 1 (choose).  s_0 = 1 - sum x, s_k+1 = x_k.  With sum_to_one constraint 0 is added first, whatever the sign of
//     s_0, and never leaves.  Otherwise p = the inactive constraint with the smallest s_p / |n_p| (|n_0| = sqrt K, else
//     1) among those below -kFeasTol; TIE RULE: the smallest number wins.  None: x is the minimiser — up to the rounding
//     of the path, |D^-1 d| eps, which is far above |x| eps when D is ill-conditioned.  So x is refined ONCE on its active
//     face, x -= J2 J2'(D x - d) and then x -= J1 R^-T s_A (a Newton step for the reduced gradient, and back onto the
//     active constraints), and step 1 is taken again; if it still finds no violated constraint the method ends.
//   Step 2 (direction).  dv = J'n_p; z = J2 dv2 (primal direction, J2 / dv2 the columns / entries q .. K - 1);
//     r = R^-1 dv1 (dual direction).  n_p'z = |dv2|^2.  n_p is taken as DEPENDENT on the active normals when
//     |dv2|^2 <= kDepTol |dv|^2 (always so when q = K).
//   Step 3 (length).  t1 = min u_j / r_j over the active inequalities with r_j > 0, l the first position that attains it
//     (infinite if none); t2 = -s_p / |dv2|^2 (infinite if dependent).  Both infinite: no feasible point — cannot
//     happen for these constraints; answered like the cap.  t = min(t1, t2); TIE RULE: t1 == t2 is a full step.
//     u -= t r on A, u_p += t, and unless dependent x += t z.  A multiplier of an inequality that rounding left below 0
//     is raised to 0.
//     Full step (t = t2): p joins A — Givens rotations of the columns q .. K - 1 of J take dv2 to (|dv2|, 0, ..), R gains
//     the column (dv1, |dv2|) — back to step 1.   Partial step (t = t1): constraint A[l] leaves — its column leaves R,
//     Givens rotations of the rows l, l + 1, .. restore the triangle, the same rotations go to the columns of J — s_p is
//     taken again from x, back to step 2 with the same p.
//   Every execution of step 2 counts as one step.  Cap: iter_cap(K) = 10 (K + 1) steps; a problem that reaches it, or
//   breaks down, answers with a NaN row and kNotSolved.  A problem with a NaN or an infinity in d is answered with a NaN
//   row and kNanInput before any step.
//   Result: w_k = 0 exactly where the bound k is active, else max(x_k, 0) (x_k >= -kFeasTol there).
//
// One statement for a group of lanes and for one CPU thread, as oadp_step.hpp: written for a group G of G::width lanes
// that work on the same problem (`lane`, `width`, sum(), sync()).  Lane i owns row i of J: the rotations of J need no
// ordering between lanes.  What is sequential by nature (the rotation chains, R, the back substitution, the lists) is
// done by lane 0 between two sync(); every lane then reads the same values from the work space and takes the same
// decisions.  The device instantiates it with 8, 16, 32 or 64 lanes of one wave, the CPU statement with Solo.  The two
// differ in the order of the sums that go through sum() only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#define BSN_QP_HD __host__ __device__ __forceinline__
#else
#define BSN_QP_HD inline
#endif

namespace bsn {
namespace qp {

constexpr int kMaxK = 60;                             // as OADP: one problem's work space stays below 64 KiB of LDS
constexpr double kFeasTol = 1.4210854715202004e-14;   // 2^-46: a constraint counts as violated below -kFeasTol
constexpr double kDepTol = 1e-26;                     // |dv2|^2 <= kDepTol |dv|^2: n_p depends on the active normals
constexpr int kNanInput = -1, kNotSolved = -2;        // step counts of a NaN row
constexpr int64_t kSlabRows = 4096;                   // rows of one slab of the moment pass (k_anc_moments)
constexpr int kMaxL = 64;                             // loadings the moment pass takes

BSN_QP_HD constexpr int iter_cap(int K) { return 10 * (K + 1); }

// doubles of work space per problem: x, J and R (K x K each), six vectors of K, two lists of K + 1 ints.  x comes first:
// the solution stays in ws[0 .. K) for the caller
BSN_QP_HD constexpr size_t work_doubles(int K) { return (size_t)2 * K * K + (size_t)7 * K + (size_t)(K + 1); }
static_assert((work_doubles(kMaxK) + kMaxK) * 8 <= 65536, "a problem's work space (and its d) exceeds the default LDS limit");

// slabs of the moment pass: forced >= 1 (BSN_ANC_SLABS) asks for that many, else kSlabRows rows each
inline int64_t slab_len(int64_t M, int64_t forced) {
  if (forced < 1) return kSlabRows;
  const int64_t len = (M + forced - 1) / forced;
  return len < 1 ? 1 : len;
}
inline int64_t slab_count(int64_t M, int64_t forced) {
  const int64_t len = slab_len(M, forced);
  return M < 1 ? 1 : (M + len - 1) / len;
}

// NULL, or why K is refused.  Host side, before any launch.
inline const char *check_k(int64_t K) {
  if (K < 1) return "snp_ancestry_summary: at least one reference group is needed.";
  if (K > kMaxK) return "snp_ancestry_summary: more than 60 reference groups are not supported.";
  return nullptr;
}

// Host side, once per call: J0 = L^-T (K x K column-major, upper triangular, zeros below) of D = L L'.  D: column-major,
// its lower triangle is read.  false: D is not (numerically) positive definite.
inline bool factor(int K, const double *D, double *J0) {
  // L into the lower triangle of J0
  for (int j = 0; j < K; j++) {
    double s = D[(size_t)j * K + j];
    for (int k = 0; k < j; k++) s -= J0[(size_t)k * K + j] * J0[(size_t)k * K + j];
    if (!(s > 0.0) || !(s - s == 0.0)) return false;
    const double ljj = sqrt(s);
    J0[(size_t)j * K + j] = ljj;
    for (int i = j + 1; i < K; i++) {
      double a = D[(size_t)j * K + i];
      for (int k = 0; k < j; k++) a -= J0[(size_t)k * K + i] * J0[(size_t)k * K + j];
      a /= ljj;
      if (!(a - a == 0.0)) return false;
      J0[(size_t)j * K + i] = a;
    }
  }
  // L^-1 in place (lower), column by column
  for (int j = 0; j < K; j++) {
    J0[(size_t)j * K + j] = 1.0 / J0[(size_t)j * K + j];
    for (int i = j + 1; i < K; i++) {
      double a = 0.0;
      for (int k = j; k < i; k++) a -= J0[(size_t)k * K + i] * J0[(size_t)j * K + k];
      J0[(size_t)j * K + i] = a / J0[(size_t)i * K + i];
    }
  }
  // transpose into the upper triangle
  for (int j = 0; j < K; j++)
    for (int i = j + 1; i < K; i++) {
      J0[(size_t)i * K + j] = J0[(size_t)j * K + i];
      J0[(size_t)j * K + i] = 0.0;
    }
  return true;
}

// the group of the CPU statement: one lane
struct Solo {
  static constexpr int width = 1;
  static constexpr int lane = 0;
  BSN_QP_HD double sum(double x) const { return x; }
  BSN_QP_HD void sync() const {}
};

// One problem.  D: K x K column-major (symmetric); J0: factor()'s result; d[k * ldd], k < K, not in ws; ws:
// work_doubles(K) doubles that the group shares; w[k * ldw]: the result (also left in ws[0 .. K)).  Every lane of the
// group makes the call with the same arguments.  Returns the number of steps, or kNanInput / kNotSolved (a NaN row).
template <class G>
BSN_QP_HD int solve_one(const G &g, int K, const double *D, const double *J0, const double *d, int64_t ldd, bool sum_to_one,
                        double *ws, double *w, int64_t ldw) {
  double *x = ws, *J = x + K, *R = J + (size_t)K * K, *dv = R + (size_t)K * K, *z = dv + K, *r = z + K, *u = r + K, *cs = u + K,
         *sn = cs + K;
  int *act = (int *)(sn + K);   // act[0 .. q): the active constraints in the order they were added
  int *pos = act + (K + 1);     // pos[c]: where constraint c stands in act, -1: inactive

  double chk = 0.0;
  for (int k = g.lane; k < K; k += G::width) {
    const double v = d[k * ldd];
    z[k] = v;
    chk += v - v;   // 0, or NaN for a NaN or an infinity
  }
  chk = g.sum(chk);
  if (!(chk == 0.0)) {   // (the same decision in every lane)
    for (int k = g.lane; k < K; k += G::width) x[k] = w[k * ldw] = NAN;
    return kNanInput;
  }
  for (int i = g.lane; i < K; i += G::width)
    for (int c = 0; c < K; c++) J[(size_t)c * K + i] = J0[(size_t)c * K + i];
  for (int c = g.lane; c <= K; c += G::width) pos[c] = -1;
  g.sync();
  // x = J0 (J0'd): lane c takes column c, then lane i row i
  for (int c = g.lane; c < K; c += G::width) {
    double a = 0.0;
    for (int i = 0; i <= c; i++) a += J[(size_t)c * K + i] * z[i];
    r[c] = a;
  }
  g.sync();
  for (int i = g.lane; i < K; i += G::width) {
    double a = 0.0;
    for (int c = i; c < K; c++) a += J[(size_t)c * K + i] * r[c];
    x[i] = a;
  }
  g.sync();

  const double inv_norm0 = 1.0 / sqrt((double)K);
  const int cap = iter_cap(K);
  int q = 0, steps = 0, p = -1;
  double sp = 0.0, up = 0.0;
  bool solved = false, refined = false;
  while (steps < cap) {
    if (p < 0) {   // step 1
      double sx = 0.0;
      for (int k = g.lane; k < K; k += G::width) sx += x[k];
      const double s0 = 1.0 - g.sum(sx);
      if (sum_to_one && pos[0] < 0) {
        p = 0;
        sp = s0;
      } else {
        double worst = -kFeasTol;
        if (pos[0] < 0 && s0 * inv_norm0 < worst) worst = s0 * inv_norm0, p = 0, sp = s0;
        for (int k = 0; k < K; k++) {
          const double v = x[k];
          if (pos[k + 1] < 0 && v < worst) worst = v, p = k + 1, sp = v;
        }
        if (p < 0 && !refined) {
          // No constraint is violated.  x carries the rounding of the path, |D^-1 d| eps — far above |x| eps when D is
          // ill-conditioned.  One step of refinement on the active face: x -= J2 J2'(D x - d) (a Newton step for the
          // reduced gradient; it does not leave the active constraints), then x -= J1 R^-T s_A puts x back on the active
          // constraints (it moves the gradient inside the span of the active normals only: D J1 = N R^-1).  Then step 1
          // is taken again.
          refined = true;
          for (int k = g.lane; k < K; k += G::width) {
            double a = -d[k * ldd];
            for (int j = 0; j < K; j++) a += D[(size_t)j * K + k] * x[j];
            z[k] = a;
          }
          g.sync();
          for (int c = q + g.lane; c < K; c += G::width) {
            double a = 0.0;
            for (int i = 0; i < K; i++) a += J[(size_t)c * K + i] * z[i];
            dv[c] = a;
          }
          g.sync();
          sx = 0.0;
          for (int i = g.lane; i < K; i += G::width) {
            double a = 0.0;
            for (int c = q; c < K; c++) a += J[(size_t)c * K + i] * dv[c];
            x[i] -= a;
            sx += x[i];
          }
          const double s0r = 1.0 - g.sum(sx);
          g.sync();
          if (g.lane == 0)
            for (int j = 0; j < q; j++) {
              double a = act[j] == 0 ? -s0r : -x[act[j] - 1];
              for (int i = 0; i < j; i++) a -= R[(size_t)j * K + i] * r[i];
              r[j] = a / R[(size_t)j * K + j];
            }
          g.sync();
          for (int i = g.lane; i < K; i += G::width) {
            double a = 0.0;
            for (int c = 0; c < q; c++) a += J[(size_t)c * K + i] * r[c];
            x[i] += a;
          }
          g.sync();
          continue;
        }
        if (p < 0) {
          solved = !(s0 != s0);   // a NaN that arose on the way makes every comparison false: not solved
          for (int k = 0; k < K; k++) solved = solved && x[k] == x[k];
          break;
        }
        refined = false;
      }
      up = 0.0;
    }
    steps++;

    // step 2: dv = J'n_p (lane c: column c), then z = J2 dv2 (lane i: row i) and r = R^-1 dv1 (lane 0)
    for (int c = g.lane; c < K; c += G::width) {
      double a = 0.0;
      if (p == 0)
        for (int i = 0; i < K; i++) a -= J[(size_t)c * K + i];
      else
        a = J[(size_t)c * K + (p - 1)];
      dv[c] = a;
    }
    g.sync();
    for (int i = g.lane; i < K; i += G::width) {
      double a = 0.0;
      for (int c = q; c < K; c++) a += J[(size_t)c * K + i] * dv[c];
      z[i] = a;
    }
    if (g.lane == 0)
      for (int i = q - 1; i >= 0; i--) {
        double a = dv[i];
        for (int j = i + 1; j < q; j++) a -= R[(size_t)j * K + i] * r[j];
        r[i] = a / R[(size_t)i * K + i];
      }
    double dd = 0.0, dn = 0.0;
    for (int c = 0; c < K; c++) {
      const double v = dv[c] * dv[c];
      dn += v;
      if (c >= q) dd += v;
    }
    g.sync();
    const bool dependent = !(dd > kDepTol * dn);

    // step 3
    double t1 = INFINITY;
    int l = -1;
    for (int j = 0; j < q; j++) {
      if (sum_to_one && act[j] == 0) continue;
      const double rj = r[j];
      if (rj > 0.0) {
        const double v = u[j] / rj;
        if (v < t1) t1 = v, l = j;
      }
    }
    const double t2 = dependent ? INFINITY : -sp / dd;
    if (!(t1 < INFINITY) && !(fabs(t2) < INFINITY)) break;   // no feasible point, or a NaN: not solved
    const bool full = !(t1 < t2);
    const double t = full ? t2 : t1;
    if (!dependent)
      for (int i = g.lane; i < K; i += G::width) x[i] += t * z[i];
    up += t;

    if (full) {
      if (g.lane == 0) {
        for (int j = 0; j < q; j++) {
          u[j] -= t * r[j];
          if (!(sum_to_one && act[j] == 0) && u[j] < 0.0) u[j] = 0.0;
          R[(size_t)q * K + j] = dv[j];
        }
        double carry = dv[K - 1];
        for (int c = K - 1; c > q; c--) {
          const double a = dv[c - 1], h = sqrt(a * a + carry * carry);
          if (h > 0.0)
            cs[c] = a / h, sn[c] = carry / h;
          else
            cs[c] = 1.0, sn[c] = 0.0;
          carry = h;
        }
        R[(size_t)q * K + q] = carry;
        u[q] = up;
        act[q] = p;
        pos[p] = q;
      }
      g.sync();
      for (int i = g.lane; i < K; i += G::width) {
        double carry = J[(size_t)(K - 1) * K + i];
        for (int c = K - 1; c > q; c--) {
          const double a = J[(size_t)(c - 1) * K + i];
          J[(size_t)c * K + i] = cs[c] * carry - sn[c] * a;
          carry = cs[c] * a + sn[c] * carry;
        }
        J[(size_t)q * K + i] = carry;
      }
      q++;
      p = -1;
      g.sync();
    } else {
      if (g.lane == 0) {
        for (int j = 0; j < q; j++) {
          u[j] -= t * r[j];
          if (!(sum_to_one && act[j] == 0) && u[j] < 0.0) u[j] = 0.0;
        }
        pos[act[l]] = -1;
        for (int j = l; j + 1 < q; j++) {
          act[j] = act[j + 1];
          u[j] = u[j + 1];
          pos[act[j]] = j;
          for (int i = 0; i <= j + 1; i++) R[(size_t)j * K + i] = R[(size_t)(j + 1) * K + i];
        }
        for (int i = l; i + 1 < q; i++) {
          const double a = R[(size_t)i * K + i], b = R[(size_t)i * K + i + 1], h = sqrt(a * a + b * b);
          const double c_ = h > 0.0 ? a / h : 1.0, s_ = h > 0.0 ? b / h : 0.0;
          cs[i] = c_;
          sn[i] = s_;
          R[(size_t)i * K + i] = h;
          R[(size_t)i * K + i + 1] = 0.0;
          for (int j = i + 1; j + 1 < q; j++) {
            const double e = R[(size_t)j * K + i], f = R[(size_t)j * K + i + 1];
            R[(size_t)j * K + i] = c_ * e + s_ * f;
            R[(size_t)j * K + i + 1] = c_ * f - s_ * e;
          }
        }
      }
      g.sync();
      for (int i = g.lane; i < K; i += G::width)
        for (int c = l; c + 1 < q; c++) {
          const double a = J[(size_t)c * K + i], b = J[(size_t)(c + 1) * K + i];
          J[(size_t)c * K + i] = cs[c] * a + sn[c] * b;
          J[(size_t)(c + 1) * K + i] = cs[c] * b - sn[c] * a;
        }
      q--;
      g.sync();
      if (p == 0) {
        double sx = 0.0;
        for (int k = g.lane; k < K; k += G::width) sx += x[k];
        sp = 1.0 - g.sum(sx);
      } else {
        sp = x[p - 1];
      }
    }
  }

  g.sync();
  for (int k = g.lane; k < K; k += G::width) {
    const double v = !solved ? NAN : pos[k + 1] >= 0 ? 0.0 : fmax(x[k], 0.0);
    x[k] = v;
    w[k * ldw] = v;
  }
  g.sync();
  return solved ? steps : kNotSolved;
}

// Pearson correlation of two vectors of length M from their moments
BSN_QP_HD double pearson(double M, double sab, double sa, double sb, double saa, double sbb) {
  const double cov = sab - sa * sb / M, va = saa - sa * sa / M, vb = sbb - sb * sb / M;
  return cov / (sqrt(va) * sqrt(vb));
}

// The correlations of one frequency vector f of length M, from moments only: G0 = X0'X0 (K x K), c0 = the column sums of
// X0, xf[k * ldxf] = (X0'f)_k, sf = sum f, sff = sum f^2.  cor_each[k * ldc] = cor(X0[, k], f); returns
// cor_pred = cor(X0 w, f).  w: K values that the group shares (solve_one's ws).
template <class G>
BSN_QP_HD double cor_one(const G &g, int K, double M, const double *G0, const double *c0, const double *xf, int64_t ldxf, double sf,
                         double sff, const double *w, double *cor_each, int64_t ldc) {
  double pf = 0.0, ps = 0.0, pp = 0.0;
  for (int k = g.lane; k < K; k += G::width) {
    const double xfk = xf[k * ldxf], wk = w[k];
    cor_each[k * ldc] = pearson(M, xfk, c0[k], sf, G0[(size_t)k * K + k], sff);
    double gw = 0.0;
    for (int j = 0; j < K; j++) gw += G0[(size_t)j * K + k] * w[j];
    pf += wk * xfk;
    ps += wk * c0[k];
    pp += wk * gw;
  }
  pf = g.sum(pf);
  ps = g.sum(ps);
  pp = g.sum(pp);
  return pearson(M, pf, ps, sf, pp, sff);
}

}  // namespace qp
}  // namespace bsn
