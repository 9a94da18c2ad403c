// ldsplit_ref.cpp — the CPU statement of snp_ldsplit's dynamic program for the tests and tools/probe_ldsplit.py: the
// sequential loops of DESIGN.md section 3.5e (rules 1 - 6), one thread, with C(m, .) = +Inf spelt out.  The per-element
// rules (how an entry enters a suffix sum, the float rounding of E, the early stop, when K blocks are reported) come from
// bigsnpr_amd/csrc/ldsplit_step.hpp, which the kernels include too; the replacement rule of a level is written here as the
// sequential if / else-if over col = m - 1 .. 0, NOT through the header's order on candidates: the device's gather in that
// order has to reproduce it.
//
// Build: g++ -O2 -ffp-contract=off -std=c++17 -fPIC -shared -I bigsnpr_amd/csrc
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "ldsplit_step.hpp"

namespace {

using bsn::ldsplit::inf;

struct Lower {   // the part of each column below its diagonal, with the suffix sums of rule 1
  int64_t m;
  const int64_t *p;
  const int32_t *i;
  std::vector<int64_t> first;   // the entry behind the diagonal
  std::vector<double> S;
  // L(c, row), row > c
  double L(int64_t c, int64_t row) const {
    if (row >= m) return 0;
    const int32_t *a = i + first[(size_t)c], *b = i + p[c + 1];
    const int32_t *at = std::lower_bound(a, b, (int32_t)row);
    return at < b ? S[(size_t)(at - i)] : 0.0;
  }
};

}  // namespace

extern "C" {

// counters [8] (may be NULL): [0] rows of a level whose winner shares its cost1 with a candidate of larger cost2,
// [1] rows of a level with two or more candidates equal to the winner in both costs, [2] rows with best_ind set and
// C = +Inf, [3] walks of E that the position window ended, [4] level 0 cut by the position window (0 / 1), [5] walks of E
// that max_cost ended, [6] finite C(0, k) over the levels, [7] columns that store nothing below the diagonal.
// Returns 0, or 1 + the first column without a non-zero diagonal.
int64_t lds_split(const int64_t *p, const int32_t *i, const double *x, int64_t m, double thr_r2, double max_r2, int32_t min_size,
                  int32_t max_size, int32_t max_K, double max_cost, const double *pos, double *C_out, int32_t *best_out,
                  double *cost_out, double *cost2_out, double *perc_out, int32_t *ok_out, int32_t *all_last_out,
                  int32_t *levels_out, int64_t *counters) {
  int64_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<double> zero;
  if (!pos) {
    zero.assign((size_t)m, 0.0);
    pos = zero.data();
  }
  // rule 1
  Lower lw{m, p, i, std::vector<int64_t>((size_t)m), std::vector<double>((size_t)p[m], 0.0)};
  int64_t nnz_lower = 0;
  for (int64_t c = 0; c < m; c++) {
    const int32_t *a = i + p[c], *b = i + p[c + 1];
    const int32_t *d = std::lower_bound(a, b, (int32_t)c);
    if (d == b || *d != c || x[d - i] == 0) return 1 + c;
    lw.first[(size_t)c] = (d - i) + 1;
    nnz_lower += p[c + 1] - (d - i);
    if (lw.first[(size_t)c] == p[c + 1]) cnt[7]++;
    double l = 0;
    for (int64_t e = p[c + 1] - 1; e >= lw.first[(size_t)c]; e--) {
      l = bsn::ldsplit::take_entry(l, x[e], thr_r2, max_r2);
      lw.S[(size_t)e] = l;
    }
  }
  // rule 2
  std::vector<std::vector<float>> E((size_t)m);
  for (int64_t col = 0; col < m; col++) {
    double e = 0;
    int32_t count = 0;
    const double pos_min = pos[col] - 1;
    for (int64_t row = col; row >= 0; row--) {
      if (pos[row] < pos_min) {
        cnt[3]++;
        break;
      }
      e = e + lw.L(row, col + 1);
      if (e > max_cost) {
        cnt[5]++;
        break;
      }
      count++;
      if (count >= min_size) {
        E[(size_t)col].push_back(bsn::ldsplit::keep(e));
        if (count == max_size) break;
      }
    }
  }
  // rule 3: row m of every level is +Inf
  const size_t ld = (size_t)m + 1;
  std::vector<double> C1(ld * (size_t)max_K, inf()), C2(ld * (size_t)max_K, inf());
  std::vector<int32_t> best((size_t)m * (size_t)max_K, -1);
  {
    const double pos_min = pos[m - 1] - 1;
    for (int64_t size = min_size; size <= max_size; size++) {
      const int64_t row = m - size;
      if (pos[row] < pos_min) {
        cnt[4] = 1;
        break;
      }
      best[(size_t)row] = (int32_t)m;
      C1[(size_t)row] = 0;
      C2[(size_t)row] = (double)size * (double)size;
    }
  }
  int32_t levels = max_K;
  for (int32_t k = 1; k < max_K; k++) {
    double *c1 = C1.data() + ld * (size_t)k, *c2 = C2.data() + ld * (size_t)k;
    const double *p1 = c1 - ld, *p2 = c2 - ld;
    int32_t *bi = best.data() + (size_t)m * (size_t)k;
    for (int64_t col = m - 1; col >= 0; col--) {
      int64_t row = col - min_size + 1;
      for (size_t t = 0; t < E[(size_t)col].size(); t++, row--) {
        const double size = (double)(col - row + 1);
        const double cost1 = (double)E[(size_t)col][t] + p1[col + 1];
        if (cost1 < c1[row]) {
          bi[row] = (int32_t)(col + 1);
          c1[row] = cost1;
          c2[row] = size * size + p2[col + 1];
        } else if (cost1 == c1[row]) {
          const double cost2 = size * size + p2[col + 1];
          if (cost2 < c2[row]) {
            bi[row] = (int32_t)(col + 1);
            c2[row] = cost2;
          }
        }
      }
    }
    if (counters) {   // what decided each row of this level
      for (int64_t row = 0; row < m; row++) {
        if (bi[row] < 0) continue;
        if (!(c1[row] < inf())) cnt[2]++;
        int same = 0, by2 = 0;
        for (int64_t t = 0; t <= (int64_t)max_size - min_size; t++) {
          const int64_t col = row + min_size - 1 + t;
          if (col >= m || (size_t)t >= E[(size_t)col].size()) continue;
          const double size = (double)(col - row + 1);
          const double a1 = (double)E[(size_t)col][(size_t)t] + p1[col + 1], a2 = size * size + p2[col + 1];
          if (a1 == c1[row] && a1 < inf()) {
            if (a2 == c2[row]) same++;
            else if (a2 < inf()) by2++;
          }
        }
        if (by2) cnt[0]++;
        if (same >= 2) cnt[1]++;
      }
    }
    if (bsn::ldsplit::stop_after(c1[0], p1[0], max_cost)) {
      levels = k + 1;
      break;
    }
  }
  for (int32_t k = 0; k < max_K; k++)
    if (C1[ld * (size_t)k] < inf()) cnt[6]++;
  // rule 6
  const double count_all = 2.0 * (double)nnz_lower - (double)m;
  for (int32_t kk = 0; kk < max_K; kk++) {
    const double cost = C1[ld * (size_t)kk];
    std::vector<int32_t> last;
    bool good = kk < levels && bsn::ldsplit::reported(cost, best[(size_t)m * (size_t)kk], max_cost);
    double sq = 0;
    if (good) {
      int64_t j = 0;
      for (int32_t k = kk; k >= 0; k--) {
        const int64_t nj = best[(size_t)j + (size_t)m * (size_t)k];
        if (nj <= j || nj > m || (k > 0 && nj == m)) {
          good = false;
          break;
        }
        last.push_back((int32_t)nj);
        sq = sq + (double)(nj - j) * (double)(nj - j);
        j = nj;
      }
    }
    double within = count_all;
    if (good) {
      size_t g = 0;
      for (int64_t j = 0; j < m; j++) {
        while (j >= last[g]) g++;   // the block of j ends before row last[g]; the last block ends at m
        for (int64_t e = p[j + 1] - 1; e >= lw.first[(size_t)j] && i[e] >= last[g]; e--) within = within - 2;
      }
    }
    if (cost_out) cost_out[kk] = cost;
    if (cost2_out) cost2_out[kk] = good ? sq : inf();
    if (perc_out) perc_out[kk] = good ? within / count_all : -1.0;
    if (ok_out) ok_out[kk] = good ? 1 : 0;
    if (all_last_out)
      for (int32_t b = 0; b < max_K; b++)
        all_last_out[(size_t)kk * (size_t)max_K + (size_t)b] = good && b <= kk ? last[(size_t)b] : -1;
  }
  for (int32_t k = 0; k < max_K; k++)
    for (int64_t r = 0; r < m; r++) {
      if (C_out) C_out[(size_t)r + (size_t)m * (size_t)k] = C1[(size_t)r + ld * (size_t)k];
      if (best_out) best_out[(size_t)r + (size_t)m * (size_t)k] = best[(size_t)r + (size_t)m * (size_t)k];
    }
  if (levels_out) *levels_out = levels;
  if (counters) std::copy(cnt, cnt + 8, counters);
  return 0;
}

// The levels as the kernels compute them — every row gathers its candidates and keeps the minimum in the header's order,
// the t range dealt out to `split` partial minima that are combined afterwards — on the host, from the same E: what
// tests/test_ldsplit_cpu.py compares with the sequential loops above.  C_out, best_out [m x max_K]; returns the levels run.
int32_t lds_gather(const int64_t *p, const int32_t *i, const double *x, int64_t m, double thr_r2, double max_r2, int32_t min_size,
                   int32_t max_size, int32_t max_K, double max_cost, const double *pos, int32_t split, double *C_out,
                   int32_t *best_out) {
  using namespace bsn::ldsplit;
  std::vector<double> zero;
  if (!pos) {
    zero.assign((size_t)m, 0.0);
    pos = zero.data();
  }
  std::vector<int64_t> first((size_t)m);
  std::vector<double> S((size_t)p[m], 0.0);
  for (int64_t c = 0; c < m; c++) {
    first[(size_t)c] = (std::lower_bound(i + p[c], i + p[c + 1], (int32_t)c) - i) + 1;
    double l = 0;
    for (int64_t e = p[c + 1] - 1; e >= first[(size_t)c]; e--) S[(size_t)e] = l = take_entry(l, x[e], thr_r2, max_r2);
  }
  const int64_t W = (int64_t)max_size - min_size + 1;
  std::vector<float> E((size_t)(W * m));
  std::vector<int32_t> len((size_t)m);
  for (int64_t col = 0; col < m; col++) {
    double e = 0;
    int32_t count = 0, n = 0;
    for (int64_t row = col; row >= 0; row--) {
      if (pos[row] < pos[col] - 1) break;
      if (col + 1 < m) {
        const int32_t *b = i + p[row + 1], *at = std::lower_bound(i + first[(size_t)row], b, (int32_t)(col + 1));
        if (at < b) e = e + S[(size_t)(at - i)];
      }
      if (e > max_cost) break;
      count++;
      if (count >= min_size) {
        E[(size_t)((count - min_size) * m + col)] = keep(e);
        n++;
        if (count == max_size) break;
      }
    }
    len[(size_t)col] = n;
  }
  std::vector<double> C2((size_t)(2 * m));
  for (int64_t k = 0; k < (int64_t)max_K * m; k++) {
    C_out[k] = inf();
    best_out[k] = -1;
  }
  for (int64_t row = 0; row < m; row++) {
    const int64_t size = m - row;
    const bool in = size >= min_size && size <= max_size && !(pos[row] < pos[m - 1] - 1);
    C2[(size_t)row] = in ? (double)size * (double)size : inf();
    if (in) {
      C_out[row] = 0;
      best_out[row] = (int32_t)m;
    }
  }
  for (int32_t k = 1; k < max_K; k++) {
    const double *p1 = C_out + (int64_t)(k - 1) * m, *p2 = C2.data() + (int64_t)((k - 1) & 1) * m;
    double *c1 = C_out + (int64_t)k * m, *c2 = C2.data() + (int64_t)(k & 1) * m;
    for (int64_t row = 0; row < m; row++) {
      std::vector<Cand> part((size_t)split, none());
      for (int64_t t = 0; t < W; t++) {
        const int64_t col = row + min_size - 1 + t;
        if (col >= m || t >= len[(size_t)col]) continue;
        const bool last = col + 1 == m;
        const Cand c = candidate(E[(size_t)(t * m + col)], last ? inf() : p1[col + 1], last ? inf() : p2[col + 1], (int32_t)row,
                                 (int32_t)col);
        if (better(c, part[(size_t)(t % split)])) part[(size_t)(t % split)] = c;
      }
      Cand b = part[0];
      for (int32_t w = 1; w < split; w++)
        if (better(part[(size_t)w], b)) b = part[(size_t)w];
      c1[row] = b.c1;
      c2[row] = b.c2;
      best_out[row + (int64_t)k * m] = b.col < 0 ? -1 : b.col + 1;
    }
    if (stop_after(c1[0], p1[0], max_cost)) return k + 1;
  }
  return max_K;
}

}  // extern "C"
