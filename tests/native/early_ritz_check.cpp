// Stand-alone check of the early Rayleigh-Ritz step of svd_driver.hpp (early_grams / early_grams_wait / prefinalize):
// block_lanczos_svd over a small dense backend (plain loops, exact fp64 products) that implements the three hooks, run
// once with the hooks answering and once with them reporting "not supported".  For every case
//   - d, u, v, niter and converged of the two runs are the same bytes,
//   - prefinalize is never handed a basis smaller than k,
//   - a finalize that finds its guess standing receives the S and dinv of that guess, byte for byte,
//   - every guess that does not stand (dropped by the driver, overtaken by the next step, basis rewritten by a
//     restart) is followed by a finalize that does the whole work,
//   - the hooks are called in the order the driver documents.
// Built plainly and with -fsanitize=address,undefined by tests/test_early_ritz_cpu.py; exit status 0 = all cases pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "svd_driver.hpp"

using namespace bsn;

struct DenseBackend : SvdBackend {
  std::vector<double> A;   // n x m_local, column-major
  std::vector<double> Q, Z, W;
  bool hooks = false;
  // what the hooks saw
  std::string order;       // one letter per call: c = At_Qblock, g = early_grams, p = A_Zblock, w = early_grams_wait,
                           // f = prefinalize, x = prefinalize(drop), s = step_fused, r = restart, F = finalize
  bool pending = false;    // early_grams was answered, early_grams_wait is due
  double *eZ = nullptr, *eQ = nullptr;
  int ep = 0, ep0 = 0, ecb = 0;
  bool grams_done = false;
  bool standing = false;   // a guess is standing: finalize with the same arguments only "waits"
  int g_pp = 0, g_k = 0;
  std::vector<double> g_S, g_dinv, g_u, g_v;
  int n_guess = 0, n_kept = 0, n_full = 0, n_small_basis = 0, n_bad_order = 0, n_mismatch = 0;

  void alloc(int cap, int b) override {
    Q.assign((size_t)n * cap, 0.0);
    Z.assign((size_t)m_local * cap, 0.0);
    W.assign((size_t)n * b, 0.0);
  }
  void random_W(int b, uint32_t seed) override {
    uint64_t s = 0x9E3779B97F4A7C15ull * (seed + 1);
    for (size_t t = 0; t < (size_t)n * b; t++) {
      s ^= s << 13; s ^= s >> 7; s ^= s << 17;
      W[t] = (double)(s >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
    }
    standing = false;
  }
  bool subset(bool) override { return true; }   // the "subset" of the warm start is the whole matrix
  void At_Qblock(int p0, int cb) override {
    order += 'c';
    if (standing) n_bad_order++;   // the solve goes on: the driver has dropped the guess of the previous step before Z is written
    for (int c = 0; c < cb; c++)
      for (int64_t j = 0; j < m_local; j++) {
        double s = 0;
        for (int64_t i = 0; i < n; i++) s += A[i + j * n] * Q[i + (size_t)(p0 + c) * n];
        Z[j + (size_t)(p0 + c) * m_local] = s;
      }
  }
  void A_Zblock(int p0, int cb) override {
    order += 'p';
    std::fill(W.begin(), W.begin() + (size_t)n * cb, 0.0);
    for (int c = 0; c < cb; c++)
      for (int64_t j = 0; j < m_local; j++) {
        const double zz = Z[j + (size_t)(p0 + c) * m_local];
        for (int64_t i = 0; i < n; i++) W[i + (size_t)c * n] += A[i + j * n] * zz;
      }
  }
  void round_W(int) override {}
  void ZtZ(int p, int p0, int cb, double *G) override {
    for (int c = 0; c < cb; c++)
      for (int a = 0; a < p; a++) {
        double s = 0;
        for (int64_t j = 0; j < m_local; j++) s += Z[j + (size_t)a * m_local] * Z[j + (size_t)(p0 + c) * m_local];
        G[a + (size_t)c * p] = s;
      }
  }
  void QtQ(int p, int p0, int cb, double *M) override {
    for (int c = 0; c < cb; c++)
      for (int a = 0; a < p; a++) {
        double s = 0;
        for (int64_t i = 0; i < n; i++) s += Q[i + (size_t)a * n] * Q[i + (size_t)(p0 + c) * n];
        M[a + (size_t)c * p] = s;
      }
  }
  void QtW(int p, int cb, double *C) override {
    for (int c = 0; c < cb; c++)
      for (int a = 0; a < p; a++) {
        double s = 0;
        for (int64_t i = 0; i < n; i++) s += Q[i + (size_t)a * n] * W[i + (size_t)c * n];
        C[a + (size_t)c * p] = s;
      }
  }
  void W_minus_QC(int p, int cb, const double *C) override {
    for (int c = 0; c < cb; c++)
      for (int a = 0; a < p; a++) {
        const double f = C[a + (size_t)c * p];
        for (int64_t i = 0; i < n; i++) W[i + (size_t)c * n] -= Q[i + (size_t)a * n] * f;
      }
  }
  void WtW(int cb, double *G) override {
    for (int c = 0; c < cb; c++)
      for (int a = 0; a < cb; a++) {
        double s = 0;
        for (int64_t i = 0; i < n; i++) s += W[i + (size_t)a * n] * W[i + (size_t)c * n];
        G[a + (size_t)c * cb] = s;
      }
  }
  void W_times(int cb, int r, const double *M) override {
    std::vector<double> row(cb), out(r);
    for (int64_t i = 0; i < n; i++) {
      for (int j = 0; j < cb; j++) row[j] = W[i + (size_t)j * n];
      for (int c = 0; c < r; c++) {
        double s = 0;
        for (int j = 0; j < cb; j++) s += row[j] * M[j + (size_t)c * cb];
        out[c] = s;
      }
      for (int c = 0; c < r; c++) W[i + (size_t)c * n] = out[c];
    }
  }
  void W_to_Q(int p0, int r) override { std::memcpy(&Q[(size_t)p0 * n], W.data(), sizeof(double) * (size_t)n * r); }

  // ---- the three hooks ----
  bool early_grams(int p, int p0, int cb, double *blkZ, double *blkQ) override {
    if (!hooks) return false;
    order += 'g';
    if (order.size() < 2 || order[order.size() - 2] != 'c') n_bad_order++;   // right behind At_Qblock
    pending = true;
    eZ = blkZ; eQ = blkQ; ep = p; ep0 = p0; ecb = cb;
    return true;
  }
  bool early_grams_wait() override {
    if (!hooks || !pending) return false;
    order += 'w';
    if (order.size() < 2 || order[order.size() - 2] != 'p') n_bad_order++;   // once A_Zblock has been queued
    pending = false;
    ZtZ(ep, ep0, ecb, eZ);   // (a device would have queued them in early_grams: Z and Q have not changed since)
    QtQ(ep, ep0, ecb, eQ);
    grams_done = true;
    return true;
  }
  void form(int pp, int k, const double *S, const double *dinv, double *u, double *v) const {
    for (int t = 0; t < k; t++) {
      for (int64_t i = 0; u && i < n; i++) {
        double s = 0;
        for (int a = 0; a < pp; a++) s += Q[i + (size_t)a * n] * S[a + (size_t)t * pp];
        u[i + (size_t)t * n] = s;
      }
      for (int64_t j = 0; v && j < m_local; j++) {
        double s = 0;
        for (int a = 0; a < pp; a++) s += Z[j + (size_t)a * m_local] * (S[a + (size_t)t * pp] * dinv[t]);
        v[j + (size_t)t * m_local] = s;
      }
    }
  }
  void prefinalize(int pp, int k, const double *S, const double *dinv, double *u, double *v) override {
    if (!hooks) return;
    if (!S) {
      order += 'x';
      standing = false;
      return;
    }
    order += 'f';
    if (order.size() < 2 || order[order.size() - 2] != 'w') n_bad_order++;   // between the two halves of the step
    if (pp < k) n_small_basis++;
    n_guess++;
    g_pp = pp; g_k = k;
    g_S.assign(S, S + (size_t)pp * k);
    g_dinv.assign(dinv, dinv + k);
    // the guess is formed NOW, from the basis as it is under the product pass, into buffers of its own: a finalize
    // that finds it standing hands these out, so a basis that changed behind a standing guess would show
    g_u.assign((size_t)n * k, 0.0);
    g_v.assign((size_t)m_local * k, 0.0);
    form(pp, k, S, dinv, g_u.data(), g_v.data());
    (void)u; (void)v;
    standing = true;
  }
  int step_fused(int p, int p0, int cb, double *blkZ, double *blkQ, std::vector<double> &Rout) override {
    order += 's';
    if (!grams_done) {
      ZtZ(p, p0, cb, blkZ);
      QtQ(p, p0, cb, blkQ);
    }
    grams_done = false;
    // two projections against Q, then modified Gram-Schmidt inside the panel; a column with nothing left: -2
    std::vector<double> Wsave(W.begin(), W.begin() + (size_t)n * cb), C((size_t)p * cb);
    double w0 = 0;
    for (int c = 0; c < cb; c++) {
      double s = 0;
      for (int64_t i = 0; i < n; i++) s += W[i + (size_t)c * n] * W[i + (size_t)c * n];
      w0 = std::max(w0, s);
    }
    for (int pass = 0; pass < 2; pass++) {
      QtW(p, cb, C.data());
      W_minus_QC(p, cb, C.data());
    }
    Rout.assign((size_t)cb * cb, 0.0);
    for (int j = 0; j < cb; j++) {
      double *wj = &W[(size_t)j * n];
      for (int i = 0; i < j; i++) {
        const double *wi = &W[(size_t)i * n];
        double r = 0;
        for (int64_t t = 0; t < n; t++) r += wi[t] * wj[t];
        Rout[i + (size_t)j * cb] = r;
        for (int64_t t = 0; t < n; t++) wj[t] -= r * wi[t];
      }
      double s = 0;
      for (int64_t t = 0; t < n; t++) s += wj[t] * wj[t];
      if (!(s > 1e-24 * w0)) {
        std::copy(Wsave.begin(), Wsave.end(), W.begin());
        return -2;
      }
      const double nrm = std::sqrt(s);
      Rout[j + (size_t)j * cb] = nrm;
      for (int64_t t = 0; t < n; t++) wj[t] /= nrm;
    }
    return cb;
  }
  bool restart(int pp, int keep, const double *S, int rn, const double *Mk) override {
    (void)rn; (void)Mk;
    order += 'r';
    if (standing) n_bad_order++;   // the driver drops a guess before it lets the basis be rewritten
    std::vector<double> Qn((size_t)n * keep, 0.0), Zn((size_t)m_local * keep, 0.0);
    for (int t = 0; t < keep; t++)
      for (int a = 0; a < pp; a++) {
        const double f = S[a + (size_t)t * pp];
        for (int64_t i = 0; i < n; i++) Qn[i + (size_t)t * n] += Q[i + (size_t)a * n] * f;
        for (int64_t j = 0; j < m_local; j++) Zn[j + (size_t)t * m_local] += Z[j + (size_t)a * m_local] * f;
      }
    std::copy(Qn.begin(), Qn.end(), Q.begin());
    std::copy(Zn.begin(), Zn.end(), Z.begin());
    return true;
  }
  void finalize(int pp, int k, const double *S, const double *dinv, double *u, double *v) override {
    order += 'F';
    if (standing) {
      // kept: the arguments must be the guess's, byte for byte
      if (pp != g_pp || k != g_k || std::memcmp(S, g_S.data(), (size_t)pp * k * 8) != 0 ||
          std::memcmp(dinv, g_dinv.data(), (size_t)k * 8) != 0)
        n_mismatch++;
      std::copy(g_u.begin(), g_u.end(), u);
      std::copy(g_v.begin(), g_v.end(), v);
      n_kept++;
      standing = false;
      return;
    }
    n_full++;
    form(pp, k, S, dinv, u, v);
  }
};

// A = sum_i s_i x_i y_i' with random x_i, y_i: a spectrum that decays like s
static std::vector<double> make_matrix(int64_t n, int64_t m, const std::vector<double> &s, uint64_t seed) {
  std::vector<double> A((size_t)n * m, 0.0), x((size_t)n), y((size_t)m);
  uint64_t r = 0x2545F4914F6CDD1Dull * (seed + 7);
  auto rnd = [&]() {
    r ^= r << 13; r ^= r >> 7; r ^= r << 17;
    return (double)(r >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
  };
  for (size_t t = 0; t < s.size(); t++) {
    for (auto &e : x) e = rnd();
    for (auto &e : y) e = rnd();
    for (int64_t j = 0; j < m; j++)
      for (int64_t i = 0; i < n; i++) A[i + j * n] += s[t] * x[i] * y[j];
  }
  return A;
}

struct Run {
  std::vector<double> d, u, v;
  SvdResult res;
  DenseBackend bk;
};

static void solve(Run &r, const std::vector<double> &A, int64_t n, int64_t m, const SvdOptions &opt, bool hooks) {
  r.bk.A = A;
  r.bk.n = n;
  r.bk.m_local = r.bk.m_total = m;
  r.bk.hooks = hooks;
  r.d.assign((size_t)opt.k, -1.0);
  r.u.assign((size_t)n * opt.k, -1.0);
  r.v.assign((size_t)m * opt.k, -1.0);
  r.res = block_lanczos_svd(r.bk, opt, r.d.data(), r.u.data(), r.v.data());
}

static int failures = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      failures++;                                \
      std::printf("  FAILED: " __VA_ARGS__);     \
      std::printf("  [%s]\n", #cond);            \
    }                                            \
  } while (0)

enum Want { kKept, kDropped, kAny };

static void run_case(const char *name, const std::vector<double> &A, int64_t n, int64_t m, const SvdOptions &opt,
                     Want last, bool want_restart, bool want_one_step) {
  Run on, off;
  solve(on, A, n, m, opt, true);
  solve(off, A, n, m, opt, false);
  const DenseBackend &b = on.bk;
  std::printf("%s: niter %d, restarts %d, converged %d, basis %d; guesses %d, kept %d, full finalize %d; calls %s\n", name,
              on.res.niter, on.res.restarts, on.res.converged, on.res.basis, b.n_guess, b.n_kept, b.n_full, b.order.c_str());
  CHECK(on.res.niter == off.res.niter && on.res.converged == off.res.converged && on.res.restarts == off.res.restarts &&
            on.res.basis == off.res.basis,
        "the two runs took different paths\n");
  CHECK(std::memcmp(on.d.data(), off.d.data(), on.d.size() * 8) == 0, "d differs\n");
  CHECK(std::memcmp(on.u.data(), off.u.data(), on.u.size() * 8) == 0, "u differs\n");
  CHECK(std::memcmp(on.v.data(), off.v.data(), on.v.size() * 8) == 0, "v differs\n");
  CHECK(std::memcmp(&on.res.max_rel_resid, &off.res.max_rel_resid, 8) == 0, "the residual estimate differs\n");
  CHECK(off.bk.n_guess == 0 && off.bk.n_kept == 0 && off.bk.n_full == 1, "hooks off: the parent's order\n");
  CHECK(off.bk.order.find_first_of("gwfx") == std::string::npos, "hooks off: a hook was used\n");
  CHECK(b.n_small_basis == 0, "prefinalize with a basis smaller than k\n");
  CHECK(b.n_mismatch == 0, "a kept guess and its finalize differ in S or dinv\n");
  CHECK(b.n_bad_order == 0, "%d hook calls out of order\n", b.n_bad_order);
  // exactly one finalize; it is full unless the last guess stood
  CHECK(b.n_kept + b.n_full == 1, "finalize calls\n");
  CHECK(b.n_guess >= 1, "no guess was made\n");
  if (last == kKept) CHECK(b.n_kept == 1 && b.n_full == 0, "the last guess should have stood\n");
  if (last == kDropped) CHECK(b.n_kept == 0 && b.n_full == 1, "a discarded guess must be followed by a full finalize\n");
  if (want_restart) CHECK(on.res.restarts > 0 && b.order.find("xr") != std::string::npos, "no restart under a dropped guess\n");
  if (want_one_step) CHECK(on.res.niter == 1 && on.res.converged == 1 && b.n_guess == 1, "not a one-step solve\n");
  CHECK(on.res.converged == 1, "not converged\n");
  // the triplets are triplets: |A' u - d v| small (a sanity check of the test's own backend)
  double worst = 0;
  for (int t = 0; t < opt.k; t++) {
    if (!(on.d[t] > 1e-8 * on.d[0])) continue;
    double num = 0;
    for (int64_t j = 0; j < m; j++) {
      double s = 0;
      for (int64_t i = 0; i < n; i++) s += A[i + j * n] * on.u[i + (size_t)t * n];
      const double e = s - on.d[t] * on.v[j + (size_t)t * m];
      num += e * e;
    }
    worst = std::max(worst, std::sqrt(num) / on.d[t]);
  }
  CHECK(worst < 1e-6, "A' u != d v: %.3e\n", worst);
}

int main() {
  {   // ordinary: 60 x 90, k = 5, block 4
    std::vector<double> s;
    for (int i = 0; i < 30; i++) s.push_back(std::pow(0.6, i));
    SvdOptions o;
    o.k = 5; o.block = 4; o.tol = 1e-8;
    run_case("ordinary", make_matrix(60, 90, s, 1), 60, 90, o, kKept, false, false);
  }
  {   // restart: a basis of 12 vectors for k = 5, block 4 on a slowly decaying spectrum
    std::vector<double> s;
    for (int i = 0; i < 40; i++) s.push_back(std::pow(0.85, i));
    SvdOptions o;
    o.k = 5; o.block = 4; o.tol = 1e-8; o.max_basis = 12;
    run_case("restart", make_matrix(60, 90, s, 2), 60, 90, o, kAny, true, false);
  }
  {   // rank-deficient: rank 6, k = 10 — the panels run out of directions, the step takes the careful path
    std::vector<double> s;
    for (int i = 0; i < 6; i++) s.push_back(1.0 / (1 + i));
    SvdOptions o;
    o.k = 10; o.block = 4; o.tol = 1e-8;
    run_case("rank-deficient", make_matrix(60, 90, s, 3), 60, 90, o, kDropped, false, false);
  }
  {   // one step: three dominant directions over a tail 300 times smaller, two warm-start iterations, k = block = 3: the first block step
      // finds its start block converged, and p >= k there
    std::vector<double> s = {100.0, 80.0, 60.0};
    for (int i = 0; i < 20; i++) s.push_back(0.2);
    SvdOptions o;
    o.k = 3; o.block = 3; o.tol = 1e-6; o.warm = 2;
    run_case("one-step", make_matrix(60, 90, s, 4), 60, 90, o, kKept, false, true);
  }
  if (failures) {
    std::printf("%d checks FAILED\n", failures);
    return 1;
  }
  std::printf("all early Rayleigh-Ritz checks passed\n");
  return 0;
}
