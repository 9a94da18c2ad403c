// svd.hip — HIP backend of the block-Lanczos partial SVD (svd_driver.hpp) and the
// bsn_bed_randomsvd entry point (replaces bed_randomSVD -> bigstatsr::big_randomSVD,
// R/autoSVD.R:205-219).  The two matrix passes per step are op_cprod / op_prod
// (matvec.hip); the tall-skinny fp64 panel algebra between them is svd_panel.hip, and what a
// call solves with (block, digits, schedule, second copy) is decided in svd_plan.hpp.
#include <chrono>
#include <unistd.h>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cmath>
#include <cstring>
#include <memory>
#include <functional>

#include "bsn_internal.hpp"
#include "orth_small.hpp"
#include "svd_driver.hpp"
#include "svd_panel.hpp"
#include "svd_plan.hpp"

namespace bsn {

// Panels of length n (samples) are held by SAMPLE BLOCKS when the solve is distributed: rank r owns
// rows [r nr, (r+1) nr) of the basis Q and of the working panel W, orthogonalises them locally and
// shares only the small coefficient matrices (p x b, b x b) — the n-side algebra is divided by the
// number of ranks instead of being replicated.  The variants (columns of G, rows of Z) are sharded
// as before.  Per block step (round 3: two small sums over the ranks instead of eight, every
// collective on the solve's own stream):
//   Z_g = A_g' Qfull           local crossproduct pass; Qfull = newest basis block, all n rows
//   Wfull = A_g Z_g            local product pass, partial sums over this rank's variants
//   W_r = reduce-scatter(Wfull) by sample blocks
//   all-reduce #1 of [Z'Z block | Q'Q block | Q'W | W'W], project + normalise W_r (orth_small.hpp)
//   all-reduce #2 of [Q'W | W'W] of the new W_r, project + normalise again
//   Qfull = round(all-gather(W_r)); Q_r gets its rows
// Without a communicator (and without the test hook) nr = n and every collective is skipped: the
// single-GPU path is the same code.
// The working panel W is not a buffer of its own: it IS the next free columns of Q (W = Q[:, p : p+cb]),
// so [Q W]' W is one tall product over contiguous columns and a finished block needs no copy.
// device buffers of a solve; lives on the bed handle between solves (grow-only)
struct SvdWorkspace {
  DevBuf<double> Q, Z, partial, dsmall, Wsave, dorth, Wfull, Wblk, Qfull, dS, dU, dV, dUfull, dM;
  // pinned host staging for the small matrices that cross the bus every block step (Gram blocks,
  // orthogonalisation coefficients): copies to pageable memory go through the runtime's own staging
  // and were measured to cost milliseconds each once a process has run a few solves
  double *h_pin = nullptr;
  size_t h_pin_n = 0;
  hipEvent_t ev_small = nullptr;   // the small matrices of a block step have reached the host
  // early Rayleigh-Ritz (HipSvdBackend::early_grams / prefinalize): "the Gram blocks of this step have reached the host"
  // (recorded on the solve's stream: Z and the stored Q are final there too), "S of the guess has left its staging
  // buffer" and "u, v of the guess are on the host" (both on the handle's second stream); the staging buffer of S
  hipEvent_t ev_early = nullptr, ev_guess_up = nullptr;
  double *h_guess = nullptr;
  size_t h_guess_n = 0;
  // sharded solve, product pass in segments (A_Zblock): the stream the reduce-scatters run on, one event per segment
  // ("its partial sums are ready") and one for "all segments have arrived"; the segments' sample lists and receive buffer
  hipStream_t st_comm = nullptr;
  hipEvent_t ev_seg[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_arrived = nullptr;
  DevBuf<int32_t> seg_rows;
  DevBuf<double> Wrecv;
  int64_t seg_n = -1, seg_nr = -1;
  int seg_world = -1;
  double *pinned(size_t count) {
    if (count > h_pin_n) {
      if (h_pin) (void)hipHostFree(h_pin);
      h_pin = nullptr;
      BSN_HIP(hipHostMalloc((void **)&h_pin, count * sizeof(double), hipHostMallocDefault));
      h_pin_n = count;
    }
    return h_pin;
  }
  ~SvdWorkspace() {
    for (auto &e : ev_seg)
      if (e) (void)hipEventDestroy(e);
    if (ev_arrived) (void)hipEventDestroy(ev_arrived);
    if (st_comm) (void)hipStreamDestroy(st_comm);
    if (ev_small) (void)hipEventDestroy(ev_small);
    if (ev_early) (void)hipEventDestroy(ev_early);
    if (ev_guess_up) (void)hipEventDestroy(ev_guess_up);
    if (h_guess) (void)hipHostFree(h_guess);
    if (h_pin) (void)hipHostFree(h_pin);
  }
};

struct HipSvdBackend : SvdBackend {
  SvdWorkspace &ws;
  explicit HipSvdBackend(SvdWorkspace &w)
      : ws(w), Q(w.Q), Z(w.Z), partial(w.partial), dsmall(w.dsmall), Wsave(w.Wsave), dorth(w.dorth),
        Wfull(w.Wfull), Wblk(w.Wblk), Qfull(w.Qfull) {}
  bsn_op *op = nullptr;
  hipStream_t st = nullptr;
  bsn_allreduce_fn hook = nullptr;
  void *ctx = nullptr;
  bsn_comm *comm = nullptr;
  int rank = 0, world = 1;
  bool dist = false;
  int64_t nr = 0, row0 = 0;  // rows of a sample block, first row of this rank's block
  DevBuf<double> &Q, &Z, &partial, &dsmall, &Wsave, &dorth, &Wfull, &Wblk, &Qfull;
  double *Wc = nullptr;      // the working panel: columns wcol .. of Q
  int wcol = 0;
  std::vector<double> horth;
  int cap = 0, b = 0;
  int kmax = 0;
  bool mx_valid = false;     // the column maxima of W (rounding) came out of the last k_update
  bool no_fused = false;     // BSN_NO_FUSED_STEP=1: the step-by-step path only (A/B, debugging)
  bool speculate = true;     // queue the start of the next step behind the orthonormalisation (BSN_NO_SPECULATION=1: off)
  bool spec_rounded = false; // ... and it has been: the driver's next round_W is a no-op
  // Early Rayleigh-Ritz (svd_driver.hpp; one GPU, resident image, fused step; BSN_NO_EARLY_RITZ=1: off).  The Gram blocks
  // of a step are queued between its two passes and u, v of the guess "the solve ends at this step" are formed and
  // sent to the host on the handle's second stream while the product pass runs on the solve's.
  bool early_on = false;
  bool grams_early = false;  // the Gram blocks of this step are in the arena already: fused() does not compute them
  double *eg_Z = nullptr, *eg_Q = nullptr;
  int eg_p = 0, eg_cb = 0;
  bool guess_live = false;      // u, v of the last prefinalize are (or will be) what a finalize with the same arguments gives
  bool guess_inflight = false;  // the second stream may still be working on a guess: dS / dU / dV / u / v are not free
  int guess_pp = 0, guess_k = 0;
  double *guess_u = nullptr, *guess_v = nullptr;
  std::vector<double> guess_S, guess_dinv;
  // bsn_svd_info::early_ritz.  n_guess runs on through the 56-bit repeat of a solve on this backend (like niter, which
  // the caller sums over both attempts); guess_used is set by every finalize, so it is the last attempt's
  int n_guess = 0, guess_used = 0;
  void guess_wait() {
    if (!guess_inflight) return;
    BSN_HIP(hipStreamSynchronize(upload_stream(op->bed)));
    guess_inflight = false;
  }
  ~HipSvdBackend() {   // (an error thrown under a guess in flight: the caller's u / v and the workspace stay in use until it ends)
    if (guess_inflight && op && op->bed && op->bed->stream_up) (void)hipStreamSynchronize(op->bed->stream_up);
  }
  int n_small_ar = 0;        // small all-reduces issued (diagnostics)
  // warm start on a leading subset of this rank's variants
  int64_t m_op_full = 0, m_sub = 0;
  bool fused_stats = false;
  int warm_launches = 0, warm_den = 16;
  bool subset(bool on) override {
    if (ooc) return false;   // (a warm start on the leading variants would walk the first slab twice: not worth the special case)
    if (on) {
      m_op_full = op->m;
      // small matrices: a full pass is cheap and the thinned matrix too noisy.  The thinned operator is
      // the sum over ranks of the shards' subsets, so the size that matters is the one over all ranks;
      // the decision is taken from quantities that are identical on every rank (a rank that skipped the
      // warm start while the others run its collectives would hang them).
      const int64_t m_lo = m_total / (world > 0 ? world : 1);
      const int64_t ms = (m_lo / warm_den) / 256 * 256;
      if (m_total / warm_den < 16384 || ms < 256) return false;
      m_sub = ms < op->m ? ms : op->m;
      op->m = m_sub;
      op->prof_kind_override = 3;
      roctx_push("svd:warm start (leading 1/16 of the variants)");
      return true;
    }
    roctx_pop();
    op->m = m_op_full;
    op->prof_kind_override = -1;
    warm_launches += 2;
    if (fused_stats) {  // the counting pass saw the subset only: count again on the first full pass
      op->stats_pending = true;
      op->na_poll = false;
      op->no_na = false;
    }
    return true;
  }
  // host wall time per phase (BSN_TIMING=1): where a solve's time outside the streaming kernels goes
  bool timing = false;
  double t_phase[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // alloc, At_Q, A_Z, grams, orth, round/copy, finalize, other
  int n_sync = 0;  // host synchronisations with the solve's stream
  struct Tick {
    HipSvdBackend *b;
    int ph;
    std::chrono::steady_clock::time_point t0;
    Tick(HipSvdBackend *b_, int ph_) : b(b_), ph(ph_), t0(std::chrono::steady_clock::now()) {
      static const char *names[8] = {"svd:alloc", "svd:crossprod pass (Z = A'Q)", "svd:product pass (W = A Z)", "svd:gram blocks",
                                     "svd:orthonormalise", "svd:round / copy block", "svd:form u, v", "svd:other"};
      roctx_push(names[ph & 7]);
    }
    ~Tick() {
      roctx_pop();
      if (b->timing)
        b->t_phase[ph] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
  };
  void sync_stream() {
    BSN_HIP(hipStreamSynchronize(st));
    n_sync++;
  }

  void setup_ranks() {
    if (comm) {
      rank = comm->rank;
      world = comm->world;
    }
    dist = comm != nullptr || hook != nullptr;
    if (!dist) world = 1, rank = 0;
    nr = dist ? (n + world - 1) / world : n;
    // RCCL path with sample blocks of at least 4096 rows: whole workgroup blocks of 512 samples per rank, so that the
    // product pass can be cut into segments of blocks whose reduce-scatters overlap the next segment (A_Zblock); the
    // padding (< 512 rows per rank) is zero rows like the padding of the last block has always been
    if (dist && comm && nr >= 4096) nr = (nr + 511) / 512 * 512;
    row0 = (int64_t)rank * nr;
  }
  void alloc(int cap_, int b_) override {
    Tick tk(this, 0);
    if (b_ > kMaxB) fail("block size must be <= %d", kMaxB);
    cap = cap_;
    b = b_;
    Q.ensure((size_t)nr * (cap + kMaxB));   // the working panel sits behind the basis
    Z.ensure((size_t)m_local * cap);
    {
      const int64_t rows_max = nr > m_local ? nr : m_local;
      partial.ensure((size_t)((rows_max + kGemmRows - 1) / kGemmRows) * ((cap + kMaxB + 15) / 16) * 2 * 256);
    }
    dsmall.ensure((size_t)(cap + 4) * 64);
    Wsave.ensure((size_t)nr * kMaxB);
    dorth.ensure((size_t)16 + 3 * kMaxB * kMaxB + (size_t)7 * (cap + kMaxB + 4) * kMaxB);
    ws.dM.ensure((size_t)kOrthMaxP * kOrthMaxP);
    if (dist) {
      const int wide = kmax > kMaxB ? kmax : kMaxB;
      Wfull.ensure((size_t)n * wide);
      Wblk.ensure((size_t)world * nr * wide);
      Qfull.ensure((size_t)n * kMaxB);
    }
    Wc = Q.p;
    wcol = 0;
  }

  // ---- collectives (all on the solve's stream: one communicator, one stream, issue order = stream order) ----
  // sum of a small device matrix over the ranks, in place
  void ar_small(double *d, int64_t count) {
    if (!dist) return;
    n_small_ar++;
    if (comm) {
      comm_allreduce_sum(comm, d, count, st);
    } else {
      sync_stream();
      hook(d, count, ctx);
    }
  }
  void reduce_scatter_W(int cb) {  // Wfull (n x cb partial sums) -> W (nr x cb, summed over ranks)
    const int64_t tot = (int64_t)world * cb * nr;
    panel_block(st, Wfull.p, n, cb, nr, world, Wblk.p);
    BSN_HIP(hipGetLastError());
    if (comm) {
      comm_reduce_scatter_sum(comm, Wblk.p, Wc, nr * cb, st);
    } else {
      sync_stream();
      hook(Wblk.p, tot, ctx);
      BSN_HIP(hipMemcpyAsync(Wc, Wblk.p + (int64_t)rank * cb * nr, (size_t)nr * cb * 8,
                             hipMemcpyDeviceToDevice, st));
    }
  }
  // src (nr x cb local rows) -> dst (n x cb, all rows, column-major)
  void all_gather_rows(const double *src, int cb, double *dst) {
    const int64_t tot = (int64_t)world * cb * nr;
    if (comm) {
      comm_all_gather(comm, src, Wblk.p, nr * cb, st);
    } else {
      BSN_HIP(hipMemsetAsync(Wblk.p, 0, (size_t)tot * 8, st));
      BSN_HIP(hipMemcpyAsync(Wblk.p + (int64_t)rank * cb * nr, src, (size_t)nr * cb * 8, hipMemcpyDeviceToDevice, st));
      sync_stream();
      hook(Wblk.p, tot, ctx);
    }
    panel_unblock(st, Wblk.p, n, cb, nr, dst);
    BSN_HIP(hipGetLastError());
  }

  // ---- backend interface ------------------------------------------------------------------
  void random_W(int bb, uint32_t seed) override {
    Wc = Q.p;
    wcol = 0;
    mx_valid = false;
    spec_rounded = false;
    guess_live = false;
    grams_early = false;
    op->preq_X = nullptr;
    panel_random(st, Wc, nr, nr, bb, seed, row0, n);
    BSN_HIP(hipGetLastError());
  }
  // the newest basis block with all n rows: Q itself on one GPU, the gathered copy otherwise
  const double *newest_block(int p0) const { return dist ? Qfull.p : Q.p + (int64_t)p0 * nr; }
  // ---- out-of-core handle (round 5): both passes of a block step WALK THE FILE in slabs of variants --------------
  // The reference maps a .bed of any size and solves on it (src/bed-acc.h:46, R/autoSVD.R:205-219).  Here a file
  // whose image does not fit the device is served slab by slab (bsn_internal.hpp): every slab is uploaded into the
  // one resident slab image (pread -> page-locked double buffer -> DMA, on the solve's stream) and the same streaming
  // kernels run on it — Z[slab rows] = A_slab' Q for the crossproduct pass, W += A_slab Z[slab rows] for the product
  // pass (added on the device).  The counts of the codes ride along the first crossproduct walk slab by slab.
  // Each pass moves the whole file over PCIe (about 40 GB/s against 4 - 5 TB/s from HBM): the solve is paced by the
  // link, 2.5 s per pass per 100 GB; what it buys is that no matrix is refused for its size.
  bool ooc = false;
  // (round 6) a solve over a LIST of variants in file order (ind.col = ind.keep of bed_autoSVD, R/autoSVD.R:296-301): slab
  // sl serves positions [sel_at[sl], sel_at[sl + 1]) of the list, sel_local = their indices inside the slab image
  const int64_t *ooc_cols = nullptr;
  std::vector<int64_t> sel_at, sel_local;
  std::unique_ptr<bsn_op> sop;        // the operator over the resident slab
  long long ooc_na_total = 0, ooc_n_bad = 0;
  bool ooc_stats_walk = false;        // this crossproduct walk also counts the codes (first full pass of the solve)
  // positions [*at, *at + returned count) of the operator's variants live in slab sl (uploaded here); 0: none of them do
  int64_t slab_selection(int64_t sl, int64_t *at) {
    if (!ooc_cols) {
      int64_t j0 = 0;
      const int64_t cnt = slab_upload(op->bed, sl, &j0);
      *at = j0;
      sel_local.clear();
      return cnt;
    }
    if (sel_at.empty()) {   // the list is in file order (checked by the entry point): one contiguous run of it per slab
      const int64_t nslab = slab_count(op->bed), sc = op->bed->slab_cols;
      sel_at.assign((size_t)nslab + 1, 0);
      for (int64_t t = 0; t < m_local; t++) sel_at[(size_t)(ooc_cols[t] / sc) + 1]++;
      for (int64_t q = 0; q < nslab; q++) sel_at[(size_t)q + 1] += sel_at[(size_t)q];
    }
    const int64_t a = sel_at[(size_t)sl], cnt = sel_at[(size_t)sl + 1] - a;
    *at = a;
    if (cnt <= 0) return 0;
    int64_t j0 = 0;
    slab_upload(op->bed, sl, &j0);
    sel_local.resize((size_t)cnt);
    for (int64_t t = 0; t < cnt; t++) sel_local[(size_t)t] = ooc_cols[a + t] - j0;
    return cnt;
  }
  void slab_operator(int64_t j0, int64_t cnt, bool with_scaling) {
    bsn_bed *img = slab_image(op->bed);
    if (!sop) sop.reset(new bsn_op());
    sop->bed = img;
    sop->n = n;
    sop->m = cnt;
    sop->rows_identity = true;
    sop->cols_contig = true;
    sop->col0 = 0;
    if (!sel_local.empty()) {   // a selection inside the slab: a range of it, or a gather list (padded like fill_op's)
      bool contig = true;
      for (int64_t t = 1; t < cnt && contig; t++) contig = sel_local[(size_t)t] == sel_local[0] + t;
      sop->cols_contig = contig;
      sop->col0 = contig ? sel_local[0] : 0;
      if (!contig) {
        const int64_t m_pad = round_up(cnt, 64);
        std::vector<int32_t> c((size_t)m_pad, (int32_t)sel_local[0]);
        for (int64_t t = 0; t < cnt; t++) c[(size_t)t] = (int32_t)sel_local[(size_t)t];
        copy_h2d(op->bed, sop->d_cols.ensure((size_t)m_pad), c.data(), (size_t)m_pad * 4);
        BSN_HIP(hipStreamSynchronize(st));   // (`c` is released on return)
      }
    }
    sop->no_na = false;
    sop->slices = op->slices;
    sop->profile = op->profile;
    sop->prof_kind_override = op->prof_kind_override;
    sop->preq_X = nullptr;
    sop->d_center.ensure((size_t)op->bed->slab_cols);
    sop->d_scale.ensure((size_t)op->bed->slab_cols);
    if (with_scaling) {
      BSN_HIP(hipMemcpyAsync(sop->d_center.p, op->d_center.p + j0, (size_t)cnt * 8, hipMemcpyDeviceToDevice, st));
      BSN_HIP(hipMemcpyAsync(sop->d_scale.p, op->d_scale.p + j0, (size_t)cnt * 8, hipMemcpyDeviceToDevice, st));
    }
  }
  void At_Qblock_ooc(int p0, int cb) {
    const int64_t nslab = slab_count(op->bed);
    const bool stats = op->stats_pending;
    if (stats) {
      ooc_na_total = ooc_n_bad = 0;
      op->d_na.ensure((size_t)op->m);
    }
    for (int64_t sl = 0; sl < nslab; sl++) {
      int64_t j0 = 0;
      const int64_t cnt = slab_selection(sl, &j0);
      if (cnt <= 0) continue;
      slab_operator(j0, cnt, !stats);
      sop->stats_pending = stats;
      sop->na_poll = false;
      op_cprod(sop.get(), newest_block(p0), n, cb, Z.p + (int64_t)p0 * m_local + j0, m_local);
      if (stats) {   // the slab's scaling and missing-value counts join the whole matrix's
        BSN_HIP(hipMemcpyAsync(op->d_center.p + j0, sop->d_center.p, (size_t)cnt * 8, hipMemcpyDeviceToDevice, st));
        BSN_HIP(hipMemcpyAsync(op->d_scale.p + j0, sop->d_scale.p, (size_t)cnt * 8, hipMemcpyDeviceToDevice, st));
        BSN_HIP(hipMemcpyAsync(op->d_na.p + j0, sop->d_na.p, (size_t)cnt * 4, hipMemcpyDeviceToDevice, st));
        sync_stream();
        if (sop->h_na_total && sop->h_na_total[0] >= 0) {
          ooc_na_total += sop->h_na_total[0];
          ooc_n_bad += sop->h_na_total[1];
        }
      } else {
        sync_stream();   // the slab image is overwritten by the next upload
      }
    }
    if (stats) {
      op->stats_pending = false;
      if (!op->h_na_total) BSN_HIP(hipHostMalloc((void **)&op->h_na_total, 2 * sizeof(long long), hipHostMallocDefault));
      op->h_na_total[0] = ooc_na_total;
      op->h_na_total[1] = ooc_n_bad;
    }
    op->passes++;
  }
  void A_Zblock_ooc(int p0, int cb) {
    const int64_t nslab = slab_count(op->bed);
    bool first = true;
    for (int64_t sl = 0; sl < nslab; sl++) {
      int64_t j0 = 0;
      const int64_t cnt = slab_selection(sl, &j0);
      if (cnt <= 0) continue;
      slab_operator(j0, cnt, true);
      op_prod_acc(sop.get(), Z.p + (int64_t)p0 * m_local + j0, m_local, cb, Wc, n, first ? 0.0 : 1.0);
      first = false;
      sync_stream();
    }
    op->passes++;
  }
  void At_Qblock(int p0, int cb) override {
    Tick tk(this, 1);
    if (progress) progress();
    guess_live = false;   // (the solve goes on)
    if (ooc) return At_Qblock_ooc(p0, cb);
    op_cprod(op, newest_block(p0), n, cb, Z.p + (int64_t)p0 * m_local, m_local);
  }
  // The product pass of a sharded solve in up to four SEGMENTS of sample blocks (every rank's sample block cut at the
  // same workgroup-block boundaries): as soon as a segment's partial sums are finalised into the blocked layout its
  // reduce-scatter is queued on a second stream behind an event, and runs while the next segment's k_prodT computes;
  // the stream of the solve waits for the last arrival.  BSN_NO_OVERLAP=1: the same segments with every collective on
  // the solve's own stream (A/B: identical results).  Needs the sample-major copy (k_prodT) and sample blocks of whole
  // 512-sample workgroup blocks; otherwise — and through the host hook — the pass runs whole, followed by ONE
  // reduce-scatter.  The sums over the ranks are the same per element either way.
  bool product_in_segments(int p0, int cb) {
    if (!comm || nr % 512 != 0 || nr < 4096 || getenv("BSN_NO_SEGMENTS")) return false;
    const int B = (int)(nr / 512), nseg = B >= 16 ? 4 : 2;
    if (ws.seg_n != n || ws.seg_nr != nr || ws.seg_world != world) {   // the segments' sample lists, piece by piece
      std::vector<int32_t> rows((size_t)world * nr);
      size_t at = 0;
      for (int sgi = 0; sgi < nseg; sgi++) {
        const int b0 = (int)((int64_t)B * sgi / nseg), b1 = (int)((int64_t)B * (sgi + 1) / nseg);
        for (int r = 0; r < world; r++)
          for (int64_t t = (int64_t)b0 * 512; t < (int64_t)b1 * 512; t++) {
            const int64_t gi = (int64_t)r * nr + t;
            rows[at++] = gi < n ? (int32_t)gi : -1;
          }
      }
      copy_h2d(op->bed, ws.seg_rows.ensure(rows.size()), rows.data(), rows.size() * 4);
      BSN_HIP(hipStreamSynchronize(st));
      ws.seg_n = n; ws.seg_nr = nr; ws.seg_world = world;
    }
    const bool overlap = !getenv("BSN_NO_OVERLAP");
    if (overlap && !ws.st_comm) BSN_HIP(hipStreamCreateWithFlags(&ws.st_comm, hipStreamNonBlocking));
    for (int i = 0; i < nseg; i++)
      if (!ws.ev_seg[i]) BSN_HIP(hipEventCreateWithFlags(&ws.ev_seg[i], hipEventDisableTiming));
    if (!ws.ev_arrived) BSN_HIP(hipEventCreateWithFlags(&ws.ev_arrived, hipEventDisableTiming));
    ws.Wrecv.ensure((size_t)nr * kMaxB);
    ProdSegment segs[4];
    for (int sgi = 0; sgi < nseg; sgi++) {
      const int b0 = (int)((int64_t)B * sgi / nseg), b1 = (int)((int64_t)B * (sgi + 1) / nseg);
      segs[sgi].bs = b1 - b0;
      segs[sgi].off = b0;
      segs[sgi].d_rows = ws.seg_rows.p + (size_t)world * 512 * b0;
      segs[sgi].d_out = Wblk.p + (size_t)world * cb * 512 * b0;
    }
    hipStream_t sc = overlap ? ws.st_comm : st;
    const std::function<void(int)> after = [&](int sgi) {
      const int64_t rows_s = (int64_t)segs[sgi].bs * 512, r0 = (int64_t)segs[sgi].off * 512;
      if (overlap) {
        BSN_HIP(hipEventRecord(ws.ev_seg[sgi], st));
        BSN_HIP(hipStreamWaitEvent(sc, ws.ev_seg[sgi], 0));
      }
      double *recv = ws.Wrecv.p + (size_t)cb * r0;
      comm_reduce_scatter_sum(comm, segs[sgi].d_out, recv, rows_s * cb, sc);
      panel_place_rows(sc, recv, rows_s, cb, r0, nr, Wc);
      BSN_HIP(hipGetLastError());
    };
    if (overlap) {   // the second stream must not run ahead of what produced Wc / Wblk's previous contents
      BSN_HIP(hipEventRecord(ws.ev_arrived, st));
      BSN_HIP(hipStreamWaitEvent(sc, ws.ev_arrived, 0));
    }
    if (!op_prod_segments(op, Z.p + (int64_t)p0 * m_local, m_local, cb, world, B, nseg, segs, after)) return false;
    if (overlap) {
      BSN_HIP(hipEventRecord(ws.ev_arrived, sc));
      hipEvent_t t0 = comm_time_begin(comm, st);   // what the solve's stream waits here is the exposed part of the exchange
      BSN_HIP(hipStreamWaitEvent(st, ws.ev_arrived, 0));
      comm_time_end(comm, t0, 3, st);
    }
    n_seg_passes++;
    exchange_mode = std::max(exchange_mode, overlap ? 3 : 2);
    return true;
  }
  // precision schedule of the driver: the digits of the following product pass, of the rounding of the block it
  // produces and of the crossproduct pass that reads that block (everything reads op->slices when it is queued)
  int min_slices = 8;
  bool hold_round = false;
  void hold_rounding(bool hold) override { hold_round = hold; }
  void set_precision(int S) override {
    if (S < 1) S = 1;
    if (S > 7) S = 7;
    op->slices = S;
    if (sop) sop->slices = S;
    if (S < min_slices) min_slices = S;
  }
  std::function<void()> progress;   // called once per pass (the exchange watchdog's deadline moves with it)
  int n_seg_passes = 0;   // product passes that ran in segments (diagnostics / tests)
  int exchange_mode = 0;  // bsn_svd_info::exchange_mode
  int n_compact_gathers = 0;   // basis blocks all-gathered as 16-bit integers
  void A_Zblock(int p0, int cb) override {
    Tick tk(this, 2);
    mx_valid = false;
    if (ooc) return A_Zblock_ooc(p0, cb);
    if (dist && product_in_segments(p0, cb)) return;
    op_prod(op, Z.p + (int64_t)p0 * m_local, m_local, cb, dist ? Wfull.p : Wc, n);
    if (dist) {
      reduce_scatter_W(cb);
      exchange_mode = std::max(exchange_mode, 1);
    }
  }
  // dC (p x cb, leading dimension ldc) = A[:, :p]' B[:, :cb] for operands with `rows` rows (leading
  // dimension = rows); local rows only
  void gemm_tn_any(const double *A, const double *B, int64_t rows, int p, int cb, double *dC, int ldc = 0) {
    panel_gemm_tn(st, A, rows, p, B, rows, cb, rows, dC, ldc > 0 ? ldc : p, partial.p);
  }
  void gemm_tn(const double *A, int p, int cb, double *C_host) {
    gemm_tn_any(A, Wc, nr, p, cb, dsmall.p);
    BSN_HIP(hipGetLastError());
    ar_small(dsmall.p, (int64_t)p * cb);
    double *hp = ws.pinned((size_t)(cap + kMaxB + 4) * kMaxB * 4 + 1024);
    BSN_HIP(hipMemcpyAsync(hp, dsmall.p, (size_t)p * cb * 8, hipMemcpyDeviceToHost, st));
    sync_stream();
    std::memcpy(C_host, hp, (size_t)p * cb * 8);
  }
  void round_cols(double *X, int64_t rows, int cb, bool have_mx) {
    unsigned long long *mx = (unsigned long long *)dorth.p;
    if (!have_mx) {
      BSN_HIP(hipMemsetAsync(mx, 0, (size_t)cb * 8, st));
      panel_col_absmax(st, X, rows, rows, cb, mx, true);
    }
    panel_round_cols(st, X, rows, rows, cb, mx, op->slices);
    BSN_HIP(hipGetLastError());
  }
  void round_W(int cb) override {
    if (cb <= 0) return;
    if (spec_rounded) {   // already queued behind the orthonormalisation (column by column: a clipped block is fine)
      spec_rounded = false;
      return;
    }
    Tick tk(this, 5);
    if (!dist) {
      round_cols(Wc, n, cb, mx_valid);
      mx_valid = false;
      return;
    }
    if (comm && op->slices <= 4 && nr % 4 == 0 && !getenv("BSN_NO_COMPACT_GATHER")) {
      // The block is rounded to 8 * slices <= 32 bits anyway: with the column maxima over ALL rows known first (an
      // all-gather of cb numbers), every rank rounds its own rows and the all-gather ships the integers — int16 up to
      // 16 bits (a quarter of the fp64 volume), int32 up to 32 (half) —, the same rounded values bit for bit (a zero
      // column keeps an unscaled zero: as in k_round_cols).  The integers travel as doubles: an all-gather only moves bytes.
      unsigned long long *mx = (unsigned long long *)dorth.p;
      BSN_HIP(hipMemsetAsync(mx, 0, (size_t)cb * 8, st));
      panel_col_absmax(st, Wc, nr, nr, cb, mx, false);
      // (the segments' receive buffer is free here; it also has to hold world * cb maxima when the sample blocks are short)
      double *gmax = ws.Wrecv.ensure(std::max((size_t)nr * kMaxB, (size_t)world * kMaxB));
      comm_all_gather(comm, (const double *)mx, gmax, cb, st);
      panel_max_over_ranks(st, (const unsigned long long *)gmax, world, cb, mx);
      // (the integers of a rank: Wfull as the send buffer, Wblk for all ranks'; 4 int16 or 2 int32 per double)
      panel_pack_int(st, Wc, nr, cb, mx, op->slices, Wfull.p);
      BSN_HIP(hipGetLastError());
      comm_all_gather(comm, Wfull.p, Wblk.p, nr * cb / (op->slices <= 2 ? 4 : 2), st);
      panel_unpack_int(st, Wblk.p, n, cb, nr, mx, op->slices, Qfull.p);
      BSN_HIP(hipGetLastError());
      n_compact_gathers++;
      return;
    }
    // every rank rounds the same gathered block (column maxima over all n rows), then keeps its rows
    all_gather_rows(Wc, cb, Qfull.p);
    round_cols(Qfull.p, n, cb, false);
    panel_take_rows(st, Qfull.p, n, cb, nr, row0, Wc);
    BSN_HIP(hipGetLastError());
  }
  void gram_to_host(const double *A, const double *B, int64_t rows, int p, int cb, double *out) {
    Tick tk(this, 3);
    gemm_tn_any(A, B, rows, p, cb, dsmall.p);
    BSN_HIP(hipGetLastError());
    ar_small(dsmall.p, (int64_t)p * cb);
    double *hp = ws.pinned((size_t)(cap + kMaxB + 4) * kMaxB * 4 + 1024);
    BSN_HIP(hipMemcpyAsync(hp, dsmall.p, (size_t)p * cb * 8, hipMemcpyDeviceToHost, st));
    sync_stream();
    std::memcpy(out, hp, (size_t)p * cb * 8);
    op_poll_stats(op);
  }
  void ZtZ(int p, int p0, int cb, double *G) override {
    gram_to_host(Z.p, Z.p + (int64_t)p0 * m_local, m_local, p, cb, G);
  }
  void QtQ(int p, int p0, int cb, double *M) override {
    gram_to_host(Q.p, Q.p + (int64_t)p0 * nr, nr, p, cb, M);
  }

  // ---- the fused block step (orth_small.hpp) -----------------------------------------------------
  // arena (doubles): [mx 16] [flag 1 | Rout B2 | ZtZ p cb | X = (Q'Qb over W'Qb | HG1) (p+cb) 2cb] [HG2 (p+cb) cb]
  // [C p cb] [Ct p cb] [Ri B2]; [flag .. left half of X] is downloaded in one piece, [ZtZ .. X] is one sum over
  // the ranks
  static constexpr int B2 = kMaxB * kMaxB;
  void update_W(int p, int cb, const double *C, const double *Ri, unsigned long long *mx) {
    panel_update(st, Q.p, nr, p, C, Ri, cb, Wc, nr, nr, mx);
  }
  // Gram blocks of the newest basis block + orthonormalisation of W against Q[:, :p] and itself, queued
  // without returning to the host; ONE synchronisation.  with_grams = false: orthonormalisation only
  // (start block, p == 0).  Returns cb, -1 (not supported: the caller takes the step-by-step path
  // for everything) or -2 (Gram blocks delivered, W restored: the panel needs the careful path).
  int fused(int p, int p0, int cb, bool with_grams, double *blkZ, double *blkQ, std::vector<double> &Rout) {
    if (cb <= 0 || cb > kMaxB || p + cb > kOrthMaxP || p + cb > cap + kMaxB || no_fused) return -1;
    if (p > 0 && Wc != Q.p + (int64_t)p * nr) return -1;
    if (p > 0 && !with_grams) return -1;   // the device copy of Q'Q is only kept by the full step
    const double *A0 = p > 0 ? Q.p : Wc;    // [Q W] (p + cb contiguous columns); the panel alone for p == 0
    Tick tk(this, 4);
    hipEvent_t tev0 = nullptr, tev1 = nullptr;
    if (timing) {
      BSN_HIP(hipEventCreate(&tev0));
      BSN_HIP(hipEventCreate(&tev1));
      BSN_HIP(hipEventRecord(tev0, st));
    }
    unsigned long long *mx = (unsigned long long *)dorth.p;
    // X = [Q W]' [Qb W] ((p + cb) x 2 cb, leading dimension p + cb; Qb = the newest basis block, columns
    // p0 .. p-1 of Q, and W right behind it: contiguous columns): its left half holds the Gram block Q'Qb the
    // Rayleigh-Ritz step needs, its right half [H; G] of pass 0 — ONE pass over Q for both
    const size_t pc = (size_t)p * cb, hg = (size_t)(p + cb) * cb;
    double *flag = dorth.p + 16, *dRout = flag + 1, *dZtZ = dRout + B2, *X = dZtZ + pc, *HG1 = X + (p > 0 ? hg : 0),
           *HG2 = HG1 + hg, *C = HG2 + hg, *Ct = C + pc, *Ri = Ct + pc;
    // (early_grams has put Z'Zb into dZtZ and Q'Qb into the first p rows of the left half of X: same kernels, same
    // operands, and an entry of gemm_tn_any depends on its two columns and the row tiling only — same numbers)
    const bool have_grams = grams_early && with_grams && p == eg_p && cb == eg_cb;
    grams_early = false;
    BSN_HIP(hipMemsetAsync(flag, 0, (size_t)(1 + B2) * 8, st));
    if (p > 0 && !have_grams) gemm_tn_any(Z.p, Z.p + (int64_t)p0 * m_local, m_local, p, cb, dZtZ);
    BSN_HIP(hipMemcpyAsync(Wsave.p, Wc, (size_t)nr * cb * 8, hipMemcpyDeviceToDevice, st));
    OrthSmall a;
    a.p = p;
    a.cb = cb;
    a.p0 = p0;
    a.QtQ = p > 0 ? X : nullptr;
    a.ldq = p + cb;
    a.M = ws.dM.p;
    a.ldm = kOrthMaxP;
    a.C = C;
    a.Ct = Ct;
    a.Ri = Ri;
    a.Rout = dRout;
    a.flag = flag;
    a.iters = std::min(min_slices, op->slices) >= 2 ? 2 : 4;   // |Q'Q - I| ~ 2^-8S (coarsest block): its cube (fifth power) is below rounding
    a.Cs = a.Gs = a.Rs = a.Ris = a.Ro = a.Dv = a.tmp = nullptr;
    for (int pass = 0; pass < 2; pass++) {
      double *HG = pass == 0 ? HG1 : HG2;
      if (pass == 0 && p > 0 && !have_grams) {
        gemm_tn_any(Q.p, Q.p + (int64_t)p0 * nr, nr, p + cb, 2 * cb, X, p + cb);
        ar_small(dZtZ, (int64_t)(pc + 2 * hg));
      } else {
        gemm_tn_any(A0, Wc, nr, p + cb, cb, HG, p + cb);   // [Q W]' W: W is columns p .. p+cb-1 of Q
        ar_small(HG, (int64_t)hg);
      }
      a.pass = pass;
      a.HG = HG;
      // the column maxima of the finished panel feed the rounding; with sample blocks they would have to be
      // combined over the ranks, so the distributed solve takes them from the gathered block instead
      unsigned long long *mxp = (pass == 1 && !dist) ? mx : nullptr;
      panel_orth2(st, a, mxp);
      update_W(p, cb, C, Ri, mxp);
    }
    BSN_HIP(hipGetLastError());
    const size_t nsmall = 1 + B2 + pc + (p > 0 ? hg : 0);
    double *hp = ws.pinned((size_t)(cap + kMaxB + 4) * kMaxB * 4 + 1024);
    BSN_HIP(hipMemcpyAsync(hp, flag, nsmall * 8, hipMemcpyDeviceToHost, st));
    if (timing) BSN_HIP(hipEventRecord(tev1, st));
    if (with_grams && speculate && !hold_round) {
      // The host now waits for the small matrices and then runs the Rayleigh-Ritz step; the device would idle
      // through both.  What the NEXT step starts with — rounding the new block and quantising it for the
      // crossproduct pass — depends on neither (unless the solve ends here or the panel turns out rank
      // deficient: then the two small kernels ran for nothing), so it is queued behind the copy and the host
      // waits for the copy alone.
      if (!ws.ev_small) BSN_HIP(hipEventCreateWithFlags(&ws.ev_small, hipEventDisableTiming));
      BSN_HIP(hipEventRecord(ws.ev_small, st));
      mx_valid = !dist;
      spec_rounded = false;
      round_W(cb);
      if (!ooc) op_cprod_prequant(op, dist ? Qfull.p : Wc, n, cb);
      spec_rounded = true;
      BSN_HIP(hipEventSynchronize(ws.ev_small));
      n_sync++;
    } else {
      sync_stream();
    }
    if (timing) {
      float ms = 0;
      BSN_HIP(hipEventElapsedTime(&ms, tev0, tev1));
      t_phase[7] += ms;
      (void)hipEventDestroy(tev0);
      (void)hipEventDestroy(tev1);
    }
    op_poll_stats(op);
    if (blkZ) std::memcpy(blkZ, hp + 1 + B2, pc * 8);
    if (blkQ)   // the first p rows of the left half of X (leading dimension p + cb)
      for (int j = 0; j < cb; j++) std::memcpy(blkQ + (size_t)j * p, hp + 1 + B2 + pc + (size_t)j * (p + cb), (size_t)p * 8);
    if (hp[0] != 0.0) {  // rank deficient or ill conditioned: undo, the driver takes the careful path
      BSN_HIP(hipMemcpyAsync(Wc, Wsave.p, (size_t)nr * cb * 8, hipMemcpyDeviceToDevice, st));
      mx_valid = false;
      spec_rounded = false;
      op->preq_X = nullptr;
      return -2;
    }
    Rout.assign((size_t)cb * cb, 0.0);
    for (int t = 0; t < cb * cb; t++) Rout[(size_t)t] = hp[1 + (size_t)t];
    mx_valid = spec_rounded ? false : !dist;
    return cb;
  }
  int step_fused(int p, int p0, int cb, double *blkZ, double *blkQ, std::vector<double> &Rout) override {
    return fused(p, p0, cb, true, blkZ, blkQ, Rout);
  }
  int orth_fused(int p, int cb, std::vector<double> &Cacc, std::vector<double> &Rout) override {
    if (p != 0) return -1;
    Cacc.clear();
    const int r = fused(0, 0, cb, false, nullptr, nullptr, Rout);
    return r < 0 ? -1 : r;
  }
  void QtW(int p, int cb, double *C) override { gemm_tn(Q.p, p, cb, C); }
  void WtW(int cb, double *G) override { gemm_tn(Wc, cb, cb, G); }
  void W_minus_QC(int p, int cb, const double *C) override {
    mx_valid = false;
    copy_h2d(op->bed, dsmall.p, C, (size_t)p * cb * 8);
    panel_gemm_nn(st, Q.p, nr, p, dsmall.p, cb, Wc, nr, 1.0, -1.0, Wc, nr, nr);
    BSN_HIP(hipGetLastError());
    sync_stream();  // C is a host vector that may be reused
  }
  void W_times(int cb, int r, const double *M) override {
    mx_valid = false;
    copy_h2d(op->bed, dsmall.p, M, (size_t)cb * r * 8);
    panel_right_mult(st, Wc, nr, nr, cb, r, dsmall.p);
    BSN_HIP(hipGetLastError());
    sync_stream();
  }
  void W_to_Q(int p0, int r) override {
    double *dst = Q.p + (int64_t)p0 * nr;
    if (dst != Wc)
      BSN_HIP(hipMemcpyAsync(dst, Wc, (size_t)nr * r * 8, hipMemcpyDeviceToDevice, st));
    wcol = p0 + r;
    Wc = Q.p + (int64_t)wcol * nr;   // the next panel goes behind the block just stored
  }
  // ---- early Rayleigh-Ritz: the hooks of svd_driver.hpp ------------------------------------------------
  // where the early Gram blocks land in the pinned staging buffer: behind everything fused() downloads
  double *early_host(size_t *cnt = nullptr) {
    const size_t half = (size_t)(cap + kMaxB + 4) * kMaxB * 2 + 512;
    if (cnt) *cnt = half;
    return ws.pinned(2 * half) + half;
  }
  bool early_grams(int p, int p0, int cb, double *blkZ, double *blkQ) override {
    grams_early = false;
    // (exactly where fused() serves the step: it then finds its Gram blocks done)
    if (!early_on || p <= 0 || cb <= 0 || cb > kMaxB || p + cb > kOrthMaxP || p + cb > cap + kMaxB) return false;
    if (Wc != Q.p + (int64_t)p * nr || p0 + cb != p) return false;
    Tick tk(this, 3);
    const size_t pc = (size_t)p * cb, hg = (size_t)(p + cb) * cb;
    size_t room = 0;
    double *hp = early_host(&room);
    if (pc + hg > room) return false;
    double *dZtZ = dorth.p + 16 + 1 + B2, *X = dZtZ + pc;   // fused()'s arena
    gemm_tn_any(Z.p, Z.p + (int64_t)p0 * m_local, m_local, p, cb, dZtZ);
    gemm_tn_any(Q.p, Q.p + (int64_t)p0 * nr, nr, p, cb, X, p + cb);
    BSN_HIP(hipGetLastError());
    BSN_HIP(hipMemcpyAsync(hp, dZtZ, (pc + hg) * 8, hipMemcpyDeviceToHost, st));
    if (!ws.ev_early) BSN_HIP(hipEventCreateWithFlags(&ws.ev_early, hipEventDisableTiming));
    BSN_HIP(hipEventRecord(ws.ev_early, st));
    eg_Z = blkZ;
    eg_Q = blkQ;
    eg_p = p;
    eg_cb = cb;
    grams_early = true;
    return true;
  }
  bool early_grams_wait() override {
    if (!grams_early) return false;
    Tick tk(this, 3);
    BSN_HIP(hipEventSynchronize(ws.ev_early));
    n_sync++;
    const double *hp = early_host();
    const size_t pc = (size_t)eg_p * eg_cb;
    std::memcpy(eg_Z, hp, pc * 8);
    for (int j = 0; j < eg_cb; j++)
      std::memcpy(eg_Q + (size_t)j * eg_p, hp + pc + (size_t)j * (eg_p + eg_cb), (size_t)eg_p * 8);
    return true;
  }
  // u = Q S and v = Z S diag(dinv) with finalize's kernels, operands and column chunks, on the handle's second stream
  // behind ev_early, and their download; returns without waiting.  Only into page-locked u / v: a pageable
  // destination would hold this thread in a staged copy while the product pass waits to be followed up.
  void prefinalize(int pp, int k, const double *S, const double *dinv, double *u, double *v) override {
    guess_live = false;
    if (!S || !early_on || !ws.ev_early || pp <= 0 || pp > cap + kMaxB || k <= 0 || (!u && !v)) return;
    if ((u && !host_is_pinned(u)) || (v && !host_is_pinned(v))) return;
    Tick tk(this, 6);
    hipStream_t up = upload_stream(op->bed);
    DevBuf<double> &dS = ws.dS, &dU = ws.dU, &dV = ws.dV;
    const size_t sk = (size_t)pp * k, need_S = (size_t)(cap + kMaxB) * k * 2 + 16;
    // one guess at a time writes dS / dU / dV / u / v: they follow each other on one stream, and a buffer grows only
    // with nothing in flight
    if (need_S > dS.n || (size_t)nr * k > dU.n || (size_t)m_local * k > dV.n) guess_wait();
    dS.ensure(need_S);
    dU.ensure((size_t)nr * k);
    dV.ensure((size_t)m_local * k);
    if (!ws.ev_guess_up) BSN_HIP(hipEventCreateWithFlags(&ws.ev_guess_up, hipEventDisableTiming));
    else BSN_HIP(hipEventSynchronize(ws.ev_guess_up));   // S of the previous guess has left the staging buffer
    if (2 * sk > ws.h_guess_n) {
      if (ws.h_guess) (void)hipHostFree(ws.h_guess);
      ws.h_guess = nullptr;
      ws.h_guess_n = 0;
      BSN_HIP(hipHostMalloc((void **)&ws.h_guess, need_S * sizeof(double), hipHostMallocDefault));
      ws.h_guess_n = need_S;
    }
    double *hs = ws.h_guess;
    std::memcpy(hs, S, sk * 8);
    for (int t = 0; t < k; t++)
      for (int i = 0; i < pp; i++) hs[sk + (size_t)i + (size_t)t * pp] = S[(size_t)i + (size_t)t * pp] * dinv[t];
    guess_inflight = true;
    BSN_HIP(hipMemcpyAsync(dS.p, hs, 2 * sk * 8, hipMemcpyHostToDevice, up));
    BSN_HIP(hipEventRecord(ws.ev_guess_up, up));
    BSN_HIP(hipStreamWaitEvent(up, ws.ev_early, 0));   // Z of this step and the stored Q are final
    for (int c0 = 0; c0 < k; c0 += kMaxB) {
      const int nc = k - c0 < kMaxB ? k - c0 : kMaxB;
      panel_gemm_nn(up, Q.p, nr, pp, dS.p + (size_t)c0 * pp, nc, nullptr, 0, 0.0, 1.0, dU.p + (int64_t)c0 * nr, nr, nr);
      panel_gemm_nn(up, Z.p, m_local, pp, dS.p + sk + (size_t)c0 * pp, nc, nullptr, 0, 0.0, 1.0, dV.p + (int64_t)c0 * m_local,
                    m_local, m_local);
    }
    BSN_HIP(hipGetLastError());
    if (u) BSN_HIP(hipMemcpyAsync(u, dU.p, (size_t)n * k * 8, hipMemcpyDeviceToHost, up));
    if (v) BSN_HIP(hipMemcpyAsync(v, dV.p, (size_t)m_local * k * 8, hipMemcpyDeviceToHost, up));
    guess_pp = pp;
    guess_k = k;
    guess_u = u;
    guess_v = v;
    guess_S.assign(S, S + sk);
    guess_dinv.assign(dinv, dinv + k);
    guess_live = true;
    n_guess++;
  }
  // thick restart: Q[:, :keep] = Q[:, :pp] S and Z[:, :keep] = Z[:, :pp] S (local rows of both), the waiting
  // panel moves behind column `keep`, the device copy of Q'Q becomes the identity on the kept part
  bool restart(int pp, int keep, const double *S, int rn, const double *Mk) override {
    if (keep + rn > pp || keep <= 0) return false;   // the panel moves to the left of where it is
    guess_live = false;   // Q and Z change under it, and its buffers are the scratch of this restart
    guess_wait();
    DevBuf<double> &dS = ws.dS, &tQ = ws.dU, &tZ = ws.dV;
    dS.ensure((size_t)pp * keep + 16);
    tQ.ensure((size_t)nr * keep);
    tZ.ensure((size_t)m_local * keep);
    copy_h2d(op->bed, dS.p, S, (size_t)pp * keep * 8);
    for (int c0 = 0; c0 < keep; c0 += kMaxB) {
      const int nc = keep - c0 < kMaxB ? keep - c0 : kMaxB;
      panel_gemm_nn(st, Q.p, nr, pp, dS.p + (size_t)c0 * pp, nc, nullptr, 0, 0.0, 1.0, tQ.p + (int64_t)c0 * nr, nr, nr);
      panel_gemm_nn(st, Z.p, m_local, pp, dS.p + (size_t)c0 * pp, nc, nullptr, 0, 0.0, 1.0, tZ.p + (int64_t)c0 * m_local,
                    m_local, m_local);
    }
    BSN_HIP(hipGetLastError());
    BSN_HIP(hipMemcpyAsync(Q.p, tQ.p, (size_t)nr * keep * 8, hipMemcpyDeviceToDevice, st));
    BSN_HIP(hipMemcpyAsync(Z.p, tZ.p, (size_t)m_local * keep * 8, hipMemcpyDeviceToDevice, st));
    double *dst = Q.p + (int64_t)keep * nr;
    BSN_HIP(hipMemcpyAsync(dst, Wc, (size_t)nr * rn * 8, hipMemcpyDeviceToDevice, st));
    Wc = dst;
    wcol = keep;
    // the device copy of Q'Q on the kept part: S'(Q'Q)S as the driver computed it (the identity up to rounding
    // unless the old basis was ill conditioned)
    copy_h2d(op->bed, dS.p, Mk, (size_t)keep * keep * 8);
    panel_put_block(st, ws.dM.p, kOrthMaxP, keep, dS.p);
    BSN_HIP(hipGetLastError());
    return true;
  }
  void finalize(int pp, int k, const double *S, const double *dinv, double *u, double *v) override {
    Tick tk(this, 6);
    guess_used = 0;
    if (guess_live && pp == guess_pp && k == guess_k && u == guess_u && v == guess_v &&
        std::memcmp(S, guess_S.data(), (size_t)pp * k * 8) == 0 && std::memcmp(dinv, guess_dinv.data(), (size_t)k * 8) == 0) {
      // the guess held: u and v are on their way (or there) — the same kernels on the same operands
      guess_live = false;
      guess_wait();
      guess_used = 1;
      sync_stream();
      return;
    }
    guess_live = false;
    guess_wait();
    std::vector<double> Sv((size_t)pp * k);
    for (int t = 0; t < k; t++)
      for (int i = 0; i < pp; i++) Sv[(size_t)i + (size_t)t * pp] = S[(size_t)i + (size_t)t * pp] * dinv[t];
    DevBuf<double> &dS = ws.dS, &dU = ws.dU, &dV = ws.dV, &dUfull = ws.dUfull;
    dS.ensure((size_t)pp * k * 2 + 16);
    dU.ensure((size_t)nr * k);
    dV.ensure((size_t)m_local * k);
    copy_h2d(op->bed, dS.p, S, (size_t)pp * k * 8);
    copy_h2d(op->bed, dS.p + (size_t)pp * k, Sv.data(), (size_t)pp * k * 8);
    for (int c0 = 0; c0 < k && pp > 0; c0 += kMaxB) {
      int nc = k - c0 < kMaxB ? k - c0 : kMaxB;
      panel_gemm_nn(st, Q.p, nr, pp, dS.p + (size_t)c0 * pp, nc, nullptr, 0, 0.0, 1.0, dU.p + (int64_t)c0 * nr, nr, nr);
      panel_gemm_nn(st, Z.p, m_local, pp, dS.p + (size_t)pp * k + (size_t)c0 * pp, nc, nullptr, 0, 0.0, 1.0,
                    dV.p + (int64_t)c0 * m_local, m_local, m_local);
    }
    BSN_HIP(hipGetLastError());
    if (pp == 0) {
      BSN_HIP(hipMemsetAsync(dU.p, 0, (size_t)nr * k * 8, st));
      BSN_HIP(hipMemsetAsync(dV.p, 0, (size_t)m_local * k * 8, st));
    }
    const double *ufull = dU.p;
    if (dist) {  // every rank returns all n rows of u
      dUfull.ensure((size_t)n * k);
      all_gather_rows(dU.p, k, dUfull.p);
      ufull = dUfull.p;
    }
    if (u) copy_d2h(op->bed, u, ufull, (size_t)n * k * 8);
    if (v) copy_d2h(op->bed, v, dV.p, (size_t)m_local * k * 8);
    sync_stream();
  }
};

}  // namespace bsn

using namespace bsn;

// Watchdog of a sharded solve (bsn_svd_options::exchange_timeout_ms): when the solve has not returned in time the
// communicator is aborted — the collectives in flight end, the next one fails, the call returns an error instead
// of hanging in a stream synchronisation for ever.  If even that does not bring the call back (a transport without
// ncclCommAbort, a wedged device) the process ends with status 86 after a grace period: a run that cannot finish
// must not outlive its driver's patience either.
struct ExchangeWatchdog {
  bsn_comm *c;
  int ms;
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  bool done = false;
  std::chrono::steady_clock::time_point deadline;
  std::atomic<int> fired{0};
  ExchangeWatchdog(bsn_comm *c_, int ms_) : c(c_), ms(ms_) {
    if (!c || ms <= 0) return;
    deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(ms);
    th = std::thread([this] {
      std::unique_lock<std::mutex> lk(mu);
      // the deadline moves with the solve's progress (kick): wait until it has really passed
      for (;;) {
        const auto dl = deadline;
        if (cv.wait_until(lk, dl, [this] { return done; })) return;
        if (std::chrono::steady_clock::now() >= deadline) break;
      }
      if (done) return;   // (checked under the lock: a solve that returned while the deadline passed keeps its communicator)
      fired.store(1);
      lk.unlock();
      const bool could = comm_abort(c);
      std::fprintf(stderr, "[bsn svd] rank %d: the sharded solve made no progress for %d ms: communicator %s\n", c->rank, ms,
                   could ? "aborted" : "cannot be aborted (no ncclCommAbort)");
      lk.lock();
      if (cv.wait_for(lk, std::chrono::seconds(20), [this] { return done; })) return;
      // Still blocked 20 s after the abort (a transport without ncclCommAbort, a wedged device).  Ending the host process
      // — R, Python — from inside a library is the caller's decision: BSN_WATCHDOG_EXIT=1 (bench.py sets it: a run that
      // cannot finish must not outlive its driver's patience) asks for exit status 86; otherwise the call stays blocked
      // and says so.
      const char *ex = getenv("BSN_WATCHDOG_EXIT");
      if (ex && atoi(ex) != 0) {
        std::fprintf(stderr, "[bsn svd] rank %d: still blocked 20 s after the abort: giving up (exit status 86, BSN_WATCHDOG_EXIT)\n", c->rank);
        std::fflush(stderr);
        _exit(86);
      }
      std::fprintf(stderr, "[bsn svd] rank %d: still blocked 20 s after the abort (BSN_WATCHDOG_EXIT=1 would end the process here)\n", c->rank);
    });
  }
  // progress of the solve (a block step's pass has been queued and the previous one synchronised): the deadline is per
  // step, not per solve — a legitimately long sharded solve is not aborted
  void kick() {
    if (!th.joinable()) return;
    std::lock_guard<std::mutex> lk(mu);
    deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(ms);
  }
  ~ExchangeWatchdog() {
    if (!th.joinable()) return;
    {
      std::lock_guard<std::mutex> lk(mu);
      done = true;
    }
    cv.notify_all();
    th.join();
  }
};

// bed_scaleBinom from host code counts (the path of row subsets, where the statistics cannot ride
// along a crossproduct pass over all samples): R/binom-scaling.R:133-142
static void binom_scale_host(const std::vector<int32_t> &cnt, int64_t n, int64_t m, std::vector<double> &center,
                             std::vector<double> &scale, int32_t *n_bad) {
  center.resize((size_t)m);
  scale.resize((size_t)m);
  int32_t bad = 0;
  for (int64_t j = 0; j < m; j++) {
    const int32_t *c = &cnt[(size_t)4 * j];
    const double sumX = (double)(c[1] + 2 * c[2]), nona = (double)(c[0] + c[1] + c[2]);
    const double af = sumX / (2.0 * nona);
    center[(size_t)j] = 2.0 * af;
    scale[(size_t)j] = std::sqrt(2.0 * af * (1.0 - af));
    if (2 * (int64_t)(c[0] + c[1] + c[2]) < n) bad++;
  }
  *n_bad = bad;
}

// What a counting pass leaves behind (matvec.hip, finish_fused_stats: k_binom_scale + k_stats_summary), for counts that
// come from the handle's cache instead (bsn_bed::stats_cache): centre / scale of bed_scaleBinom — the same operations in
// the same order, so the same bits — and out[0] = number of missing genotypes, out[1] = variants with > 50 % missing
// (integer atomics; cleared by the caller).  The per-variant missing counts are on the handle already (na_cnt).
#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void k_scale_from_counts(const int32_t *counts, int64_t m, int64_t n, double *center,
                                                           double *scale, unsigned long long *out) {
  long long s = 0, bad = 0;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < m; j += (int64_t)gridDim.x * 256) {
    const int4 c = *(const int4 *)(counts + 4 * j);
    const double sumX = (double)(c.y + 2 * c.z);
    const double nona = (double)(c.x + c.y + c.z);
    const double af = sumX / (2.0 * nona);
    center[j] = 2.0 * af;
    scale[j] = sqrt(2.0 * af * (1.0 - af));
    s += c.w;
    if (2 * ((int64_t)c.x + c.y + c.z) < n) bad++;
  }
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off);
    bad += __shfl_down(bad, off);
  }
  __shared__ long long sw[4], sb[4];
  if ((threadIdx.x & 63) == 0) {
    sw[threadIdx.x >> 6] = s;
    sb[threadIdx.x >> 6] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s = sw[0] + sw[1] + sw[2] + sw[3];
    bad = sb[0] + sb[1] + sb[2] + sb[3];
    if (s) atomicAdd(&out[0], (unsigned long long)s);
    if (bad) atomicAdd(&out[1], (unsigned long long)bad);
  }
}
#pragma clang fp contract(on)

// The scaling statistics of a solve whose variants all have their counts in the owner's cache: queued on the solve's
// stream before its first launch, so no pass has to count.  The two totals come back through the operator's pinned
// words like those of a counting pass and are read where the solve synchronises at its end.
static void stats_from_cache(bsn_op *op, bsn_bed *owner, const StatsCols &sel) {
  bsn_bed *b = op->bed;
  int32_t *cnt = op->d_counts.ensure((size_t)4 * op->m + 8);
  stats_cache_load(owner, sel, cnt, b->stream);
  if (!op->h_na_total) BSN_HIP(hipHostMalloc((void **)&op->h_na_total, 2 * sizeof(long long), hipHostMallocDefault));
  op->h_na_total[0] = -1;
  op->h_na_total[1] = -1;
  unsigned long long *d_tot = (unsigned long long *)(cnt + 4 * op->m);   // (the spare words behind the counts)
  BSN_HIP(hipMemsetAsync(d_tot, 0, 16, b->stream));
  int gx = (int)((op->m + 1023) / 1024);
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(k_scale_from_counts, dim3(gx), dim3(256), 0, b->stream, cnt, op->m, op->n, op->d_center.p,
                     op->d_scale.p, d_tot);
  BSN_HIP(hipGetLastError());
  BSN_HIP(hipMemcpyAsync(op->h_na_total, d_tot, 16, hipMemcpyDeviceToHost, b->stream));
}

// the variants of the compacted copy as indices of the owner, on the device (kept while the copy answers to the same list)
static const int32_t *owner_cols_device(bsn_bed *owner, bsn_bed *sub, const int64_t *cols, int64_t m) {
  auto &sc = owner->stats_cache;
  if (sc.cols_key == 0 || sc.cols_key != owner->sub_key || (int64_t)sc.d_cols.n < m) {
    std::vector<int32_t> c32((size_t)m);
    for (int64_t j = 0; j < m; j++) {
      if (cols[j] < 0 || cols[j] >= owner->m) fail("internal: variant %lld of %lld in a compacted solve", (long long)cols[j], (long long)owner->m);
      c32[(size_t)j] = (int32_t)cols[j];
    }
    copy_h2d(sub, sc.d_cols.ensure((size_t)m), c32.data(), (size_t)m * 4);
    sc.cols_key = owner->sub_key;
  }
  return sc.d_cols.p;
}

// A solve over a list of variants that is not a contiguous range runs on a compacted copy of the selection
// (bsn_bed::sub, bsn_internal.hpp).  Returns the copy, or nullptr when the solve should go through the gather lists:
// contiguous columns, a small selection (BSN_COMPACT_MIN_BYTES, default 256 MB of 2-bit payload: below that a solve
// is milliseconds either way), no room for the copy and its sample-major twin, BSN_NO_COMPACT=1, a byte / look-up image.
static bsn_bed *compacted_view(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m) {
  if (!ind_col || m < 2 || bed->bits != 2 || bed->generic || bed->streamed() || getenv("BSN_NO_COMPACT")) return nullptr;
  bool contig = true;
  for (int64_t j = 1; j < m && contig; j++) contig = ind_col[j] == ind_col[0] + j;
  if (contig) return nullptr;
  const int64_t pitch = round_up((n + 3) / 4, 256);
  const double bytes = (double)(m + 64) * (double)pitch;
  double min_bytes = 256e6;
  if (const char *e = getenv("BSN_COMPACT_MIN_BYTES")) min_bytes = atof(e);
  if (bytes < min_bytes) return nullptr;
  // FNV-1a over the lists: the same selection again (repeated solves, bench.py) reuses the copy as it is
  uint64_t key = 1469598103934665603ull;
  auto mix = [&](const int64_t *p, size_t count) {   // (one multiply per index: a list of a million variants in a millisecond)
    for (size_t i = 0; i < count; i++) {
      key = (key ^ (uint64_t)p[i]) * 1099511628211ull;
      key ^= key >> 29;
    }
  };
  mix(&n, 1);
  mix(&m, 1);
  mix(ind_col, (size_t)m);
  bool rows_ident = n == bed->n;
  if (ind_row)
    for (int64_t i = 0; rows_ident && i < n; i++) rows_ident = ind_row[i] == i;
  if (!rows_ident && ind_row) mix(ind_row, (size_t)n);
  if (key == 0) key = 1;
  // the same selection again: the key AND the lists themselves (8 m bytes kept on the handle; a hash can collide)
  const bool keep_rows = !rows_ident && ind_row;
  if (bed->sub && bed->sub_key == key && bed->sub->n == n && bed->sub->m == m && (int64_t)bed->sub_cols.size() == m &&
      std::memcmp(bed->sub_cols.data(), ind_col, (size_t)m * 8) == 0 &&
      (keep_rows ? ((int64_t)bed->sub_rows.size() == n && std::memcmp(bed->sub_rows.data(), ind_row, (size_t)n * 8) == 0)
                 : bed->sub_rows.empty()))
    return bed->sub;
  BSN_HIP(hipSetDevice(bed->device));
  const bool in_place = bed->sub && bed->sub->n == n && bed->sub->cap_m >= m;
  if (!in_place) {
    if (bed->sub) {   // another shape: its memory goes back first
      bed_free(bed->sub);
      bed->sub = nullptr;
      bed->sub_key = 0;
      bed->sub_cols.clear();
      bed->sub_rows.clear();
    }
    size_t free_b = 0, total_b = 0;
    BSN_HIP(hipMemGetInfo(&free_b, &total_b));
    // the copy, its sample-major twin, the workspace of a solve (basis and panels: ~ 3 KB per sample + per variant)
    if ((double)(free_b + dev_cache_held()) < 2.0 * bytes + 3000.0 * (double)(n + m) + 2e9) return nullptr;
  }
  bsn_bed *fresh = nullptr;
  try {
    fresh = image_gather(bed, rows_ident ? nullptr : ind_row, n, ind_col, m, in_place ? bed->sub : nullptr);
  } catch (const std::exception &) {
    if (in_place) {   // the old copy is half overwritten: it answers to no list any more
      bed->sub_key = 0;
      bed->sub_cols.clear();
      bed->sub_rows.clear();
      throw;
    }
    (void)hipGetLastError();
    return nullptr;   // (no room after all)
  }
  bed->sub = fresh;
  bed->sub_key = key;
  bed->stats_cache.cols_key = 0;   // (the device copy of the previous list)
  bed->sub_cols.assign(ind_col, ind_col + m);
  if (keep_rows) bed->sub_rows.assign(ind_row, ind_row + n);
  else bed->sub_rows.clear();
  return fresh;
}

// ---- bsn_bed_randomsvd, step by step ------------------------------------------------------------------------------------
namespace {

// what one call carries from step to step
struct SolveCall {
  const bsn_svd_options *o;
  // what the solve runs on: the caller's handle and lists, or (compacted) the copy of the selection, without lists
  bsn_bed *bed;
  const int64_t *ind_row, *ind_col;
  int64_t n, m;
  // the handle's device-resident code counts (bsn_bed::stats_cache) serve, and are fed by, a solve over all samples of
  // a resident 2-bit image; on the compacted copy too, through the caller's handle and the caller's variant list
  bsn_bed *owner = nullptr;
  const int64_t *owner_cols = nullptr;
  bool ooc = false;               // (round 5) an out-of-core handle: the passes of the solve walk the file in slabs
  bool all_rows = false;          // all samples in file order
  bool compacted = false;
  bool fused = false;             // bed_scaleBinom evaluated on the device ...
  bool served = false;            // ... from the counts on the handle, before the first launch
  bool use_stats_cache = false;
  StatsCols sel{nullptr, nullptr, 0, 0};
  int32_t n_bad = 0;
  std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
  double t_compact = 0.0, t_create = 0.0;
  float gpu_ms = 0;
  double since() const {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
};

// an out-of-core handle (HipSvdBackend, "out-of-core handle") covers all samples, and its variants in file order
void check_selection(SolveCall &c) {
  c.all_rows = c.n == c.bed->n;
  for (int64_t i = 0; c.all_rows && c.ind_row && i < c.n; i++) c.all_rows = c.ind_row[i] == i;
  if (!c.ooc) return;
  if (c.o->comm || c.o->allreduce) fail("an out-of-core handle cannot be one shard of a sharded solve: shard the file instead");
  const int64_t *ind_col = c.ind_col;
  bool all_cols = c.m == c.bed->m, in_order = true;
  for (int64_t j = 0; ind_col && j < c.m; j++) {
    if (ind_col[j] != j) all_cols = false;
    if (ind_col[j] < 0 || ind_col[j] >= c.bed->m) fail("Tested %lld < %lld. Subscript out of bounds (ind.col).", (long long)ind_col[j], (long long)c.bed->m);
    if (j > 0 && ind_col[j] <= ind_col[j - 1]) in_order = false;
  }
  // (round 6) a LIST of variants in file order is served too — what bed_autoSVD solves over (ind.keep, sorted)
  if (!c.all_rows || !in_order)
    fail("bed_randomSVD on an out-of-core handle (the file's image does not fit the device: it streams its file) "
         "covers all samples, and its variants in increasing file order; a subset small enough for the device is served "
         "by a handle of its own (snp_subset / bsn_bed_subset_payload)");
  c.ind_row = nullptr;
  if (all_cols) c.ind_col = nullptr;
}

// (round 5) a list of variants that is not a contiguous range: the solve runs on a compacted copy of the selection
void enter_compacted_view(SolveCall &c) {
  c.bed->last_solve_on_sub = false;
  c.owner = c.bed;
  c.owner_cols = c.ind_col;
  c.use_stats_cache = c.o->binom_scaling && !c.ooc && c.all_rows && stats_cache_enabled(c.owner);
  if (bsn_bed *sub = compacted_view(c.bed, c.ind_row, c.n, c.ind_col, c.m)) {
    c.bed->last_solve_on_sub = true;
    if (c.ind_row == nullptr && c.n != c.bed->n) fail("internal: row count of a compacted solve");
    c.bed = sub;
    c.ind_row = nullptr;
    c.ind_col = nullptr;
    c.compacted = true;
    c.t_compact = c.since();
  }
}

// operator and workspace of the previous solve on this handle are reused (grow-only buffers)
struct OpLend {
  bsn_bed *bed;
  std::unique_ptr<bsn_op> op;
  explicit OpLend(bsn_bed *b) : bed(b), op(std::move(b->svd_op)) {
    if (!op) op.reset(new bsn_op());
    op->passes = 0;
    op->prof_kind_override = -1;
    for (const void *&pk : op->prof_kernel) pk = nullptr;   // (bsn_bed_streaming_kernels names the launches of THIS solve)
    op->stats_pending = false;
    op->na_poll = false;
    op->no_na = false;
  }
  ~OpLend() { bed->svd_op = std::move(op); }
};

// the operator with its scaling: the caller's centre / scale, or bed_scaleBinom from counts that are on the handle
// already, that ride along the first crossproduct pass, or that the host takes (a subset of the samples)
void setup_scaling(SolveCall &c, bsn_op *op, const double *center, const double *scale) {
  const bsn_svd_options *o = c.o;
  bsn_bed *bed = c.bed;
  const int64_t n = c.n, m = c.m;
  c.sel = StatsCols{nullptr, nullptr, 0, m};
  if (!o->binom_scaling) {
    fill_op(op, bed, c.ind_row, n, c.ind_col, m, center, scale, false, c.ooc);
    return;
  }
  fill_op(op, bed, c.ind_row, n, c.ind_col, m, nullptr, nullptr, true, c.ooc);
  if (c.use_stats_cache) {
    if (c.compacted) c.sel = StatsCols{c.owner_cols, owner_cols_device(c.owner, bed, c.owner_cols, m), 0, m};
    else if (!op->cols_contig) c.sel = StatsCols{c.ind_col, op->d_cols.p, 0, m};
    else c.sel.col0 = op->col0;
    c.served = op->rows_identity && stats_cache_known(c.owner, c.sel);
  }
  if (c.served) {
    // every variant's counts are on the handle: centre / scale before the first launch, no pass counts, and whether
    // the missing-value plane is needed is known from the start
    c.fused = true;
    stats_from_cache(op, c.owner, c.sel);
    if (c.compacted && !getenv("BSN_FORCE_NA_PLANE")) {   // (fill_op looked at the copy's record; the owner's is the one that is known)
      bool all0 = (int64_t)c.owner->na_cnt.size() == c.owner->m;
      for (int64_t j = 0; all0 && j < m; j++) all0 = c.owner->na_cnt[(size_t)c.owner_cols[j]] == 0;
      op->no_na = all0;
    }
  } else if (op->rows_identity) {
    // the counts ride along the first crossproduct pass; until they are known the general kernels run
    op->stats_pending = true;
    op->no_na = false;
    c.fused = true;
  } else {
    std::vector<int32_t> cnt((size_t)4 * m);
    counts_host(bed, c.ind_row, n, c.ind_col, m, cnt.data());
    std::vector<double> ce, sc;
    binom_scale_host(cnt, n, m, ce, sc, &c.n_bad);
    copy_h2d(bed, op->d_center.p, ce.data(), (size_t)m * 8);
    copy_h2d(bed, op->d_scale.p, sc.data(), (size_t)m * 8);
    if (o->center_out) std::copy(ce.begin(), ce.end(), o->center_out);
    if (o->scale_out) std::copy(sc.begin(), sc.end(), o->scale_out);
  }
}

void configure_backend(HipSvdBackend &bk, const SolveCall &c, bsn_op *op) {
  const bsn_svd_options *o = c.o;
  bk.op = op;
  bk.ooc = c.ooc;
  bk.ooc_cols = c.ooc ? c.ind_col : nullptr;
  bk.st = c.bed->stream;
  bk.n = c.n;
  bk.m_local = c.m;
  bk.m_total = o->m_total > 0 ? o->m_total : c.m;
  bk.hook = o->comm ? nullptr : o->allreduce;
  bk.ctx = o->allreduce_ctx;
  bk.comm = o->comm;
  bk.rank = o->hook_rank;
  bk.world = o->hook_world > 0 ? o->hook_world : 1;
  bk.kmax = o->k;
  if (bk.comm && bk.comm->device != c.bed->device) fail("the communicator was created on another device");
  if (bk.hook && (bk.rank < 0 || bk.rank >= bk.world)) fail("hook_rank %d of %d", bk.rank, bk.world);
  bk.setup_ranks();
  bk.timing = getenv("BSN_TIMING") != nullptr;
  bk.speculate = getenv("BSN_NO_SPECULATION") == nullptr;
  bk.no_fused = getenv("BSN_NO_FUSED_STEP") != nullptr;
  bk.early_on = !bk.dist && !c.ooc && !bk.no_fused && getenv("BSN_NO_EARLY_RITZ") == nullptr;
  bk.fused_stats = c.fused && !c.served;
  bk.warm_den = warm_den_of(o->warm_denominator);
  const int64_t dim = bk.n < bk.m_total ? bk.n : bk.m_total;
  if (o->k > dim) fail("'k' is larger than the dimensions of the matrix.");
}

// what plan_solve (svd_plan.hpp) reads: the options, the operator and the switches
SolveFacts solve_facts(const SolveCall &c, const bsn_op *op, const HipSvdBackend &bk) {
  const bsn_svd_options *o = c.o;
  SolveFacts f;
  f.k = o->k, f.tol = o->tol, f.slices = o->slices, f.block = o->block, f.vec_floor = o->vec_floor;
  f.warm_start = o->warm_start, f.warm_denominator = o->warm_denominator;
  f.max_basis = o->max_basis, f.max_restarts = o->max_restarts, f.seed = o->seed, f.verbose = o->verbose;
  f.m = c.m, f.m_total = bk.m_total, f.n = c.n, f.cols_contig = op->cols_contig, f.col0 = op->col0;
  f.fused = c.fused;
  if (const char *e = getenv("BSN_VEC_FLOOR")) f.vec_floor_set = true, f.vec_floor_env = atof(e);   // (A/B and the accuracy sweeps of the tests)
  if (const char *e = abl_getenv("BSN_START_SLICES")) f.start_slices_set = true, f.start_slices_env = atoi(e);
  f.zq_split = abl_getenv("BSN_ZQ_SPLIT") != nullptr;
  return f;
}

// The second copy of the image this solve reads (which one it wants: svd_plan.hpp).  Returns true when the sample-major
// copy is to be started behind the call.
// (round 6) on one GPU the FIRST such solve of a handle runs without the copy — its product passes take k_prod<2>, the
// same sums, 55 ms more at 400K x 1M — and the copy is made BEHIND it (image_smaj_start at the end of the call: a helper
// thread allocates 100 GB and queues the transposition on a stream of its own while the caller looks at its result);
// later solves find it.  Inside the call the copy cost 90 ms (40 of allocation on an idle device, 51 of transposition)
// to save 55; allocated BESIDE the running solve the same hipMalloc took 1 - 2.5 s and held up every allocation of the
// solve (profiles/r06_cold.txt).  A caller that solves once never pays for it.  A sharded solve builds it up front:
// every rank must take the same exchange pattern, and which passes find the copy would differ between ranks.
bool choose_second_copy(bsn_bed *bed, const HipSvdBackend &bk, const SolvePlan &plan) {
  bool have_smaj = false, smaj_after = false;
  if (plan.wants_smaj) {
    if (bk.dist || getenv("BSN_SMAJ_SYNC")) have_smaj = image_smaj(bed);
    else if (bed->d_smaj || bed->smaj_job) have_smaj = image_smaj_poll(bed) || bed->smaj_job != nullptr;
    else have_smaj = smaj_after = !bed->smaj_tried && bed->bits == 2 && !getenv("BSN_NO_SMAJ");
  }
  if (!have_smaj && plan.tile_ok) image_tile(bed);
  return smaj_after;
}

// the exchange of a sharded solve by name (bsn_svd_info::exchange_mode); 0, no product pass has recorded one yet: the
// one the switches will make it take
const char *exchange_name(int mode) {
  if (mode == 0) mode = getenv("BSN_NO_SEGMENTS") ? 1 : getenv("BSN_NO_OVERLAP") ? 2 : 3;
  return mode == 3 ? "segments, reduce-scatters on a second stream" : mode == 2 ? "segments, one stream" : "whole pass";
}

// The solve, and its repeat on 56-bit products when the first one asks for it (needs_resolve, svd_plan.hpp); `plan` is
// the one of the last attempt afterwards.  Between the two events on the handle's stream: c.gpu_ms.
SvdResult solve_and_repeat(SolveCall &c, HipSvdBackend &bk, bsn_op *op, const SolveFacts &facts, SolvePlan &plan, double *d,
                           double *u, double *v) {
  const bsn_svd_options *o = c.o;
  bsn_bed *bed = c.bed;
  BSN_HIP(hipEventRecord(bed->ev0, bed->stream));
  int wd_ms = o->exchange_timeout_ms;
  if (wd_ms == 0)
    if (const char *e = getenv("BSN_EXCHANGE_TIMEOUT_MS")) wd_ms = atoi(e);
  ExchangeWatchdog watchdog(bk.comm, wd_ms);
  if (bk.comm && wd_ms > 0) bk.progress = [&watchdog] { watchdog.kick(); };
  if (bk.comm) {
    double junk_ms[kCommClasses];
    int junk_n[kCommClasses];
    bk.comm->timing = o->exchange_timing != 0;
    comm_time_collect(bk.comm, junk_ms, junk_n);   // (leftovers of a solve that failed)
  }
  struct TimingOff {
    bsn_comm *c;
    ~TimingOff() { if (c) c->timing = false; }
  } timing_off{bk.comm};
  SvdResult r;
  try {
    r = block_lanczos_svd(bk, plan.so, d, u, v);
  } catch (const std::exception &ex) {
    {   // the timing events of the launches that did run are of no use to anybody
      double pms[kProfKinds];
      int pc[kProfKinds];
      prof_collect(op, pms, pc);
    }
    if (watchdog.fired.load())
      fail("the exchange of the sharded solve did not finish within %d ms (exchange: %s) and the communicator was aborted; "
           "what the solve saw: %s", wd_ms, exchange_name(bk.exchange_mode), ex.what());
    throw;
  }
  // the precision schedule moves bsn_op::slices step by step (set_precision): the repeat and the verdict go by the digits
  // the solve ENDED on, as they always have
  plan.op_slices = op->slices;
  if (needs_resolve(r, facts, plan)) {
    // a Krylov space exhausted on rounded products (svd_driver.hpp): only matrices whose rank fits the basis get
    // here, so the second solve — 56-bit digits, at most four vectors per pass — is cheap, and it is run whenever
    // the coupling block is not negligible, met tolerance or not: a matrix this small deserves its exact values
    if (o->verbose)
      std::fprintf(stderr, "[bsn svd] %s on %d-bit products (relative residual %.3g, %d requested triplets below their resolution): "
                           "again with 56-bit products\n", r.exhausted ? "Krylov space exhausted" : "triplets below the products' resolution",
                   8 * op->slices, r.max_rel_resid, r.below_resolution);
    plan = plan_resolve(plan);
    op->slices = plan.op_slices;
    const SvdResult r1 = r;
    r = block_lanczos_svd(bk, plan.so, d, u, v);
    r.niter += r1.niter;
    r.nops += r1.nops;
    r.restarts += r1.restarts;
    plan.op_slices = op->slices;
  }
  bk.progress = nullptr;   // (the watchdog ends with this scope)
  const double t_solve = c.since() - c.t_create;
  if (o->verbose > 1 || bk.timing)
    std::fprintf(stderr,
                 "[bsn svd] host wall ms: op_create %.2f, solve %.2f = alloc %.2f + A'Q %.2f + AZ %.2f + grams %.2f + "
                 "orth %.2f (GPU events %.2f) + round %.2f + finalize %.2f + host algebra %.2f\n",
                 c.t_create, t_solve, bk.t_phase[0], bk.t_phase[1], bk.t_phase[2], bk.t_phase[3], bk.t_phase[4],
                 bk.t_phase[7], bk.t_phase[5], bk.t_phase[6],
                 t_solve - (bk.t_phase[0] + bk.t_phase[1] + bk.t_phase[2] + bk.t_phase[3] + bk.t_phase[4] +
                            bk.t_phase[5] + bk.t_phase[6]));
  BSN_HIP(hipEventRecord(bed->ev1, bed->stream));
  BSN_HIP(hipEventSynchronize(bed->ev1));
  BSN_HIP(hipEventElapsedTime(&c.gpu_ms, bed->ev0, bed->ev1));
  return r;
}

// What the scaling inside the solve leaves behind: the per-variant completeness of the handle, the counts for the
// handle's cache, the > 50 % missing count of bed_colstats (src/bed-fun.cpp:40-41) and the centre / scale actually used.
void harvest_scaling(SolveCall &c, bsn_op *op) {
  const bsn_svd_options *o = c.o;
  bsn_bed *bed = c.bed, *owner = c.owner;
  const int64_t m = c.m;
  if (c.fused && !c.served) {
    // by-products of the counting pass.  They come back through the workspace's pinned staging buffer: blocking copies
    // into pageable memory were measured to leave the runtime with ~4 ms wake-up latencies on every later stream
    // synchronisation of the process (tools/gpu/r02_h.sh).
    SvdWorkspace &ws = *bed->svd_ws;
    const int64_t chunk = 1 << 21;  // int32 per staged piece (8 MB)
    int32_t *hp = (int32_t *)ws.pinned((size_t)chunk / 2);
    if ((int64_t)bed->na_cnt.size() != bed->m) bed->na_cnt.assign((size_t)bed->m, -1);
    // ... and the counts themselves, into the handle's cache for the next solve (the downloads below synchronise)
    const bool feed = c.use_stats_cache && !op->stats_pending && op->m == m && (int64_t)op->d_counts.n >= 4 * m;
    if (feed) stats_cache_store(owner, c.sel, op->d_counts.p, bed->stream);
    if (feed && c.compacted && (int64_t)owner->na_cnt.size() != owner->m) owner->na_cnt.assign((size_t)owner->m, -1);
    for (int64_t j0 = 0; j0 < m; j0 += chunk) {
      const int64_t cnt = std::min<int64_t>(chunk, m - j0);
      BSN_HIP(hipMemcpyAsync(hp, op->d_na.p + j0, (size_t)cnt * 4, hipMemcpyDeviceToHost, bed->stream));
      BSN_HIP(hipStreamSynchronize(bed->stream));
      if (c.ind_col) {
        for (int64_t j = 0; j < cnt; j++) bed->na_cnt[(size_t)c.ind_col[j0 + j]] = hp[j];
      } else {
        std::memcpy(&bed->na_cnt[(size_t)j0], hp, (size_t)cnt * 4);
      }
      if (feed && c.compacted)
        for (int64_t j = 0; j < cnt; j++) owner->na_cnt[(size_t)c.owner_cols[j0 + j]] = hp[j];
    }
  }
  if (c.fused) {
    if (op->h_na_total && op->h_na_total[1] >= 0) c.n_bad += (int32_t)op->h_na_total[1];
    if (o->center_out) copy_d2h(bed, o->center_out, op->d_center.p, (size_t)m * 8);
    if (o->scale_out) copy_d2h(bed, o->scale_out, op->d_scale.p, (size_t)m * 8);
  }
}

// true, with the reason as the call's error text, when the triplets are not vouched for (return code 2)
bool unconverged_verdict(SvdResult &r, const SolvePlan &plan) {
  const SvdOptions &so = plan.so;
  if (r.converged && r.below_resolution > 0) {
    // (the digits were fixed by the caller: no second solve) the triplets the test left out are not vouched for
    r.converged = 0;
    char buf[320];
    std::snprintf(buf, sizeof(buf),
                  "%d of the %d requested singular triplets lie below what %d-bit products resolve (sigma below %.1e sigma_1): "
                  "their values are not converged; ask for more digits (slices) or fewer triplets",
                  r.below_resolution, so.k, 8 * plan.op_slices, std::sqrt(64.0) * so.resid_floor);
    set_error(buf);
    return true;
  }
  if (!r.converged) {
    char buf[256];
    std::snprintf(buf, sizeof(buf),
                  "the Krylov basis is full (%d vectors) but only a relative residual of %.3g (tol %.3g) was "
                  "reached for the %d requested singular triplets; increase max_basis or tol",
                  r.basis, r.max_rel_resid, so.tol, so.k);
    set_error(buf);
    return true;
  }
  return false;
}

void fill_info(bsn_svd_info *info, const SolveCall &c, const HipSvdBackend &bk, bsn_op *op, const SvdResult &r,
               const SolveFacts &facts, const SolvePlan &plan) {
  const SvdOptions &so = plan.so;
  const bsn_bed *bed = c.bed;
  info->n_bad = c.n_bad;
  info->fused_stats = c.fused ? 1 : 0;
  info->niter = r.niter;
  info->nops = (int32_t)op->passes;
  info->basis = r.basis;
  info->converged = r.converged;
  info->max_rel_resid = r.max_rel_resid;
  info->gpu_ms = c.gpu_ms;
  double pms[kProfKinds];
  int pc[kProfKinds];
  prof_collect(op, pms, pc);
  if (bk.sop) {   // out-of-core: the launches ran on the slab operator, one per slab
    double p2[kProfKinds];
    int c2[kProfKinds];
    prof_collect(bk.sop.get(), p2, c2);
    for (int t = 0; t < kProfKinds; t++) {
      pms[t] += p2[t];
      pc[t] += c2[t];
      if (bk.sop->prof_kernel[t]) op->prof_kernel[t] = bk.sop->prof_kernel[t];
    }
  }
  info->wide_cprod_ms = pms[4];
  info->wide_prod_ms = pms[5];
  info->n_wide_cprod = pc[4];
  info->n_wide_prod = pc[5];
  info->slices_max = r.slices_used_max > 0 ? r.slices_used_max : so.slices_base;
  info->wide_steps = r.wide_steps;
  info->lead_rel_resid = r.lead_rel_resid;
  info->cprod_ms = pms[0];
  info->prod_ms = pms[1];
  info->n_cprod = pc[0];
  info->n_prod = pc[1];
  info->cprod_stats_ms = pms[2];
  info->n_cprod_stats = pc[2];
  info->warm_ms = pms[3];
  info->warm_launches = bk.warm_launches;
  info->warm_fraction = bk.m_sub > 0 && bk.m_op_full > 0 ? (double)bk.m_sub / (double)bk.m_op_full : 0.0;
  info->block = so.block;
  info->slices = so.slices_base;
  info->tiled = (bed->d_tiled != nullptr && op->cols_contig && (op->col0 & 63) == 0) ? 1 : 0;
  if (bed->d_smaj != nullptr && on_prodT(so, facts)) info->tiled = 2;   // (one launch of two column blocks per product pass: k_prodT)
  info->segmented_passes = bk.n_seg_passes;
  info->compact_gathers = bk.n_compact_gathers;
  info->out_of_core = c.ooc ? 1 : 0;
  info->na_free_steps[0] = op->bed->na_free[0];
  info->na_free_steps[1] = op->bed->na_free[1];
  info->na_skip = (op->na_skip_c ? 1 : 0) | (op->na_skip_p ? 2 : 0);
  info->compacted = c.compacted ? 1 : 0;
  info->compact_ms = c.t_compact;
  info->exchange_mode = bk.exchange_mode;
  info->early_ritz[0] = bk.n_guess;
  info->early_ritz[1] = bk.guess_used;
  for (int t = 0; t < 4; t++) info->exchange_ms[t] = 0, info->n_exchange[t] = 0;
  if (bk.comm && c.o->exchange_timing) {
    double ems[kCommClasses];
    int en[kCommClasses];
    comm_time_collect(bk.comm, ems, en);
    for (int t = 0; t < 4 && t < kCommClasses; t++) info->exchange_ms[t] = ems[t], info->n_exchange[t] = en[t];
  }
}

}  // namespace

extern "C" int bsn_bed_randomsvd(bsn_bed *bed, const int64_t *ind_row, int64_t n,
                                 const int64_t *ind_col, int64_t m, const double *center,
                                 const double *scale, const bsn_svd_options *o, double *d, double *u,
                                 double *v, bsn_svd_info *info) {
  bool unconverged = false;
  int rc = guarded([&] {
    if (!o) fail("options must not be NULL");
    if (o->k < 1) fail("'k' must be at least 1.");
    RoctxRange whole("bsn_bed_randomsvd");
    SolveCall c{o, bed, ind_row, ind_col, n, m};
    c.ooc = bed->streamed();
    check_selection(c);
    enter_compacted_view(c);
    OpLend lend(c.bed);
    bsn_op *op = lend.op.get();
    if (!c.bed->svd_ws) c.bed->svd_ws = std::make_shared<SvdWorkspace>();
    setup_scaling(c, op, center, scale);
    c.t_create = c.since();
    op->profile = true;
    if (o->slices > 7) fail("slices must be in 1..7");
    HipSvdBackend bk(*c.bed->svd_ws);
    configure_backend(bk, c, op);
    const SolveFacts facts = solve_facts(c, op, bk);
    SolvePlan plan = plan_solve(facts);
    op->slices = plan.op_slices;
    const bool smaj_after = choose_second_copy(c.bed, bk, plan);
    SvdResult r = solve_and_repeat(c, bk, op, facts, plan, d, u, v);
    harvest_scaling(c, op);
    unconverged = unconverged_verdict(r, plan);
    if (info) fill_info(info, c, bk, op, r, facts, plan);
    // the sample-major copy for the NEXT solve, made beside the caller's own work — started last: on a box whose free
    // memory has to be scrubbed the allocation of 100 GB takes seconds and holds up every other call into the runtime
    if (smaj_after && !c.bed->d_smaj && !c.bed->smaj_job) (void)image_smaj_start(c.bed);
  });
  return rc != 0 ? rc : (unconverged ? 2 : 0);
}
