// handle.hip — a bsn_bed as an object: what it owns and how it goes, the slab image and the slab walk of an out-of-core
// handle, and the entries that make, describe, trim and close a handle.
#include <cxxabi.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>

#include "bsn_internal.hpp"

namespace bsn {

static void free_bed(bsn_bed *b) { bed_free(b); }
void bed_free(bsn_bed *b) {
  if (!b) return;
  for (int i = 0; i < 2; i++) {
    if (b->h_stage[i]) (void)hipHostFree(b->h_stage[i]);
    if (b->ev_stage[i]) (void)hipEventDestroy(b->ev_stage[i]);
  }
  if (b->smaj_job) {   // a background build of the sample-major copy reads d_img: let it end before the image goes
    try { image_smaj_wait(b); } catch (...) {}
  }
  if (b->d_img) (void)hipFree(b->d_img);
  if (b->map_base) (void)munmap(b->map_base, b->map_len);
  if (b->fd_file >= 0) (void)close(b->fd_file);
  if (b->slab_stage) delete (bsn::FileStage *)b->slab_stage;
  if (b->slab_img) bed_free(b->slab_img);
  if (b->sub) bed_free(b->sub);
  if (b->d_tiled) (void)hipFree(b->d_tiled);
  if (b->d_smaj) (void)hipFree(b->d_smaj);
  if (b->d_lut) (void)hipFree(b->d_lut);
  if (b->h_na_blocks) (void)hipHostFree(b->h_na_blocks);
  if (b->d_na_blocks) (void)hipFree(b->d_na_blocks);
  if (b->ev0) (void)hipEventDestroy(b->ev0);
  if (b->ev1) (void)hipEventDestroy(b->ev1);
  if (b->ev_up) (void)hipEventDestroy(b->ev_up);
  if (b->stream_up) (void)hipStreamDestroy(b->stream_up);
  if (b->stream && !b->stream_borrowed) (void)hipStreamDestroy(b->stream);
  delete b;
}

void require_resident(const bsn_bed *b, const char *what) {
  if (b->streamed())
    fail("%s needs the genotype image resident on the device: this handle streams its file (%.1f GB do not fit the device "
         "memory that was free when it was opened); bed_prodVec, bed_cprodVec, counts / colstats / MAF / scaleBinom and the "
         "`[` accessor are served out of core",
         what, (double)b->m * (double)b->pitch / 1e9);
}

// ---- out-of-core handles: the resident slab image --------------------------------------------------------------------
// One image of slab_cols variants lives on the handle (with its page-locked staging buffers) and is filled with one
// slab of the file at a time.  It works on the HANDLE's stream: whatever the caller queues there — the kernels of a
// one-shot entry point, the passes of a solve (svd.hip) — is ordered with the uploads without further ado.
bsn_bed *slab_image(bsn_bed *b) {
  BSN_HIP(hipSetDevice(b->device));
  if (!b->slab_img) {
    std::unique_ptr<bsn_bed, void (*)(bsn_bed *)> im(new bsn_bed(), bed_free);
    image_alloc(im.get(), b->n, b->slab_cols);
    (void)hipStreamDestroy(im->stream);
    im->stream = b->stream;
    im->stream_borrowed = true;
    b->slab_img = im.release();
  }
  if (!b->slab_stage) b->slab_stage = new FileStage();
  return b->slab_img;
}
int64_t slab_count(const bsn_bed *b) { return (b->m + b->slab_cols - 1) / b->slab_cols; }
// slab sl of the file into the slab image (pread into pinned buffers, double-buffered against the DMA, recode, zero
// pad rows); returns its number of variants, *j0 = its first variant
void slab_upload_range(bsn_bed *b, int64_t j0, int64_t cnt) {
  bsn_bed *img = slab_image(b);
  if (j0 < 0 || cnt <= 0 || j0 + cnt > b->m || cnt > b->slab_cols)
    fail("internal: variants %lld .. %lld into a slab image of %lld", (long long)j0, (long long)(j0 + cnt), (long long)b->slab_cols);
  img->m = cnt;
  img->na_cnt.clear();
  img->forget_counts();
  image_from_file(img, b->fd_file, 3 + j0 * b->n_byte, b->n_byte, (FileStage *)b->slab_stage);
}
int64_t slab_upload(bsn_bed *b, int64_t sl, int64_t *j0_out) {
  const int64_t j0 = sl * b->slab_cols, cnt = std::min(b->slab_cols, b->m - j0);
  if (cnt <= 0) fail("internal: slab %lld of %lld", (long long)sl, (long long)slab_count(b));
  slab_upload_range(b, j0, cnt);
  if (j0_out) *j0_out = j0;
  return cnt;
}

// ---- out-of-core handles: the one-shot entry points over slabs of variants --------------------------------------
// The selected variants are grouped by slab (order inside a slab = order in ind_col); `f(SlabPart)` runs per non-empty
// slab on a resident image of that slab, in ascending slab order.
void slab_walk(bsn_bed *bed, const int64_t *ind_col, int64_t m, const std::function<void(const SlabPart &)> &f) {
  bsn_bed *img = slab_image(bed);   // kept on the handle between calls, like its staging buffers
  const int64_t nslab = (bed->m + bed->slab_cols - 1) / bed->slab_cols;
  std::vector<std::vector<int64_t>> pos((size_t)nslab);
  for (int64_t p = 0; p < m; p++) {
    const int64_t c = ind_col ? ind_col[p] : p;
    if (c < 0 || c >= bed->m) fail("Tested %lld < %lld. Subscript out of bounds (ind.col).", (long long)c, (long long)bed->m);
    pos[(size_t)(c / bed->slab_cols)].push_back(p);
  }
  std::vector<int64_t> local;
  for (int64_t sl = 0; sl < nslab; sl++) {
    const std::vector<int64_t> &P = pos[(size_t)sl];
    if (P.empty()) continue;
    const int64_t j0 = sl * bed->slab_cols;
    slab_upload(bed, sl);
    local.resize(P.size());
    for (size_t k = 0; k < P.size(); k++) local[k] = (ind_col ? ind_col[P[k]] : P[k]) - j0;
    f(SlabPart{img, P, local});
  }
}

const double *SlabPart::gather(const double *src, std::vector<double> &buf) const {
  if (!src) return nullptr;
  buf.resize(P.size());
  for (size_t k = 0; k < P.size(); k++) buf[k] = src[P[k]];
  return buf.data();
}

void SlabPart::place(void *out, const void *part, size_t col_bytes) const {
  for (size_t k = 0; k < P.size(); k++)
    std::memcpy((uint8_t *)out + (size_t)P[k] * col_bytes, (const uint8_t *)part + k * col_bytes, col_bytes);
}

}  // namespace bsn

using namespace bsn;

extern "C" {

int bsn_bed_from_host(const uint8_t *payload, int64_t n, int64_t m, int64_t n_byte, bsn_bed **out) {
  return guarded([&] {
    require_gpu();
    if (n_byte < (n + 3) / 4) fail("n or p does not match the dimensions of the file.");
    std::unique_ptr<bsn_bed, void (*)(bsn_bed *)> b(new bsn_bed(), free_bed);
    image_alloc(b.get(), n, m);
    image_from_host(b.get(), payload, n_byte);
    *out = b.release();
  });
}

int bsn_bed_open(const char *path, int64_t n, int64_t m, bsn_bed **out) {
  return guarded([&] {
    // validation order and messages of src/bed-acc-xptr.cpp:14-35 (the reference maps the file;
    // here it is read once into the device image, so the header is checked with a 3-byte read)
    int fd = open(path, O_RDONLY);
    if (fd < 0) fail("Error when mapping file:\n  %s.\n", strerror(errno));
    struct Close {
      int fd;
      ~Close() { close(fd); }
    } closer{fd};
    struct stat st;
    if (fstat(fd, &st) != 0) fail("Error when mapping file:\n  %s.\n", strerror(errno));
    const size_t size = (size_t)st.st_size;
    uint8_t f[3] = {0, 0, 0};
    if (size == 0) fail("Error when mapping file:\n  %s.\n", strerror(EINVAL));  // mmap of an empty file
    const ssize_t got = pread(fd, f, 3, 0);
    if (got < 0) fail("Error when mapping file:\n  %s.\n", strerror(errno));
    if (size < 3 || !(f[0] == 0x6C && f[1] == 0x1B)) fail("File is not a binary PED file.");
    if (f[2] != 0x01) fail("Variant-major is the only mode supported.");
    int64_t n_byte = (n + 3) / 4;
    if (n <= 0 || m <= 0 || (size_t)(3 + n_byte * m) != size)
      fail("n or p does not match the dimensions of the file.");
    require_gpu();
    std::unique_ptr<bsn_bed, void (*)(bsn_bed *)> b(new bsn_bed(), free_bed);
    // does the image fit?  free device memory less 2 GB of working room, or BSN_IMAGE_BUDGET (bytes)
    const int64_t pitch = round_up(n_byte, 256);
    const double image_bytes = (double)(m + 64) * (double)pitch;
    size_t free_b = 0, total_b = 0;
    BSN_HIP(hipMemGetInfo(&free_b, &total_b));
    double budget = (double)(free_b + dev_cache_held()) - 2e9;
    const char *forced = getenv("BSN_IMAGE_BUDGET");
    if (forced) budget = atof(forced);
    // The resident image is tried first whenever it could fit at all: a device that other handles have filled to
    // within the 2 GB of working room must not turn a small file into a streamed handle, which most entry points
    // refuse.  Only an allocation that really fails — or a file beyond the budget — goes out of core.
    bool resident = image_bytes <= budget;
    if (!resident && !forced && image_bytes <= (double)(free_b + dev_cache_held())) resident = true;
    if (resident) {
      bool ok = true;
      try {
        image_alloc(b.get(), n, m);
      } catch (const std::exception &) {
        if (forced || image_bytes <= budget - 8e9) throw;   // (not a matter of room)
        (void)hipGetLastError();
        ok = false;
        b.reset(new bsn_bed());
      }
      if (ok) {
        image_from_file(b.get(), fd, 3, n_byte);
        *out = b.release();
        return;
      }
    }
    // out-of-core: keep the file mapped, walk it in slabs (bsn_internal.hpp)
    void *map = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (map == MAP_FAILED) fail("Error when mapping file:\n  %s.\n", strerror(errno));
    image_alloc(b.get(), n, 1);   // stream, events, geometry; no variants resident
    (void)hipFree(b->d_img);
    b->d_img = nullptr;
    b->m = m;
    b->map_base = map;
    b->map_len = size;
    b->h_map = (const uint8_t *)map + 3;
    b->fd_file = dup(fd);
    if (b->fd_file < 0) fail("Error when mapping file:\n  %s.\n", strerror(errno));
    // one resident slab image, kept on the handle between calls (bsn_bed_release_workspace frees it): a slab of at most
    // 16 GB — PCIe paces the walk, a larger slab buys nothing and would pin the device memory other handles need
    b->slab_cols = std::max<int64_t>(64, (int64_t)(std::min(std::max(budget, 0.0), 16e9) / (double)pitch) / 64 * 64 - 64);
    if (b->slab_cols > m) b->slab_cols = round_up(m, 64);
    if (getenv("BSN_VERBOSE"))
      std::fprintf(stderr, "[bsn] %s: image of %.1f GB does not fit (%.1f GB available): out-of-core handle, slabs of %lld variants\n",
                   path, image_bytes / 1e9, budget / 1e9, (long long)b->slab_cols);
    *out = b.release();
  });
}

int bsn_bed_is_streamed(const bsn_bed *bed) { return bed->streamed() ? 1 : 0; }

// FBM.code256 -> device image.  The 256 decoded values decide the image kind:
//   all of them in {0, 1, 2, NA}          -> 2-bit image (CODE_012, CODE_IMPUTE_PRED, ...): every entry point
//   on a grid v_off + v_step k, |k| <= 127 -> byte image (CODE_DOSAGE: 0.00 .. 2.00 by 0.01): colstats and
//                                             the products (and what is built on them: PRS, SVD)
//   anything else                          -> refused (there is no exact integer image of it)
static void fbm_open(const uint8_t *bytes, int64_t n, int64_t m, int64_t ld, const double *code256, bsn_bed **out) {
  require_gpu();
  if (ld < n) fail("Incompatibility between dimensions.");
  bool calls = true;
  double vmin = 0, vmax = 0;
  int nval = 0;
  for (int c = 0; c < 256; c++) {
    const double v = code256[c];
    if (std::isnan(v)) continue;
    if (!(v == 0.0 || v == 1.0 || v == 2.0)) calls = false;
    if (nval == 0 || v < vmin) vmin = v;
    if (nval == 0 || v > vmax) vmax = v;
    nval++;
  }
  if (nval == 0) fail("'code256' holds no value");
  uint8_t lut[256];
  std::unique_ptr<bsn_bed, void (*)(bsn_bed *)> b(new bsn_bed(), free_bed);
  if (calls) {
    for (int c = 0; c < 256; c++) lut[c] = std::isnan(code256[c]) ? 3 : (uint8_t)code256[c];
    image_alloc(b.get(), n, m, 2);
    image_from_fbm(b.get(), bytes, ld, lut);
    // FBMs of imputed data have no missing value: one count pass settles it for every later operator
    std::vector<int32_t> cnt((size_t)4 * m);
    counts_host(b.get(), nullptr, n, nullptr, m, cnt.data());
  } else {
    // smallest positive difference between two values as the step, mid-range as the offset; the grid is then
    // SNAPPED to the range (step = range / number of steps): the raw difference of two rounded decimals, e.g.
    // 0.00999999999999979 for CODE_DOSAGE, would bias every decoded value by up to 4e-14
    double step = 0;
    for (int a = 0; a < 256; a++)
      for (int c = 0; c < 256; c++) {
        const double d = code256[a] - code256[c];
        if (d > 1e-12 * (std::fabs(vmax) + std::fabs(vmin) + 1) && (step == 0 || d < step)) step = d;
      }
    double off = vmin;
    bool ok = step > 0 && (vmax - vmin) / step <= 254.5;
    if (ok) {
      const double nsteps = std::round((vmax - vmin) / step);
      step = (vmax - vmin) / nsteps;
      off = vmin + std::round(nsteps / 2.0) * step;
    }
    for (int c = 0; c < 256 && ok; c++) {
      if (std::isnan(code256[c])) {
        lut[c] = 0x80;
        continue;
      }
      // values like 0.07 are not exactly k * 0.01 in binary: the decoded value must reproduce the table entry to
      // a few units in the last place of the table's range
      const double kr = std::round((code256[c] - off) / step);
      // 16 units in the last place of the table's range: off + step * kr carries three roundings and the table was
      // written by other arithmetic (i * 0.01, seq(0, 2, by = 0.01), a decimal parser ...) — one ulp of slack (round 3)
      // sent such tables to the slow generic image for nothing; an entry really off the grid misses by ~step
      if (kr < -127 || kr > 127 ||
          std::fabs(off + step * kr - code256[c]) > 16 * 2.220446049250313e-16 * (std::fabs(vmax) + std::fabs(vmin) + step))
        ok = false;
      lut[c] = (uint8_t)(int8_t)kr;
    }
    if (!ok) {
      // any other table: the FBM's own bytes + the table, served by the fp64 look-up kernels only
      if (getenv("BSN_VERBOSE"))
        std::fprintf(stderr, "[bsn] code256 is neither calls nor a regular grid of <= 255 steps: generic look-up image "
                             "(colstats / prodVec / cprodVec only)\n");
      for (int c = 0; c < 256; c++) lut[c] = (uint8_t)c;
      image_alloc(b.get(), n, m, 8);
      b->generic = true;
      BSN_HIP(hipMalloc((void **)&b->d_lut, 256 * sizeof(double)));
      BSN_HIP(hipMemcpy(b->d_lut, code256, 256 * sizeof(double), hipMemcpyHostToDevice));
      image_from_fbm(b.get(), bytes, ld, lut);
      // missing values: which codes are NaN, counted per variant on the host from the caller's bytes would
      // cost a pass; the look-up kernels propagate NaN on their own, so only "some / none" is recorded
      bool any_nan = false;
      for (int c = 0; c < 256; c++) any_nan = any_nan || std::isnan(code256[c]);
      if (!any_nan) b->na_cnt.assign((size_t)m, 0);
      *out = b.release();
      return;
    }
    image_alloc(b.get(), n, m, 8);
    b->v_off = off;
    b->v_step = step;
    image_from_fbm(b.get(), bytes, ld, lut);
    // which variants are complete (no missing value): the products then skip the missing-value plane
    DevBuf<long long> d_st;
    stats8(b.get(), nullptr, n, nullptr, 0, m, d_st.ensure((size_t)3 * m));
    std::vector<long long> st((size_t)3 * m);
    copy_d2h(b.get(), st.data(), d_st.p, st.size() * 8);
    b->na_cnt.resize((size_t)m);
    for (int64_t j = 0; j < m; j++) b->na_cnt[(size_t)j] = (int32_t)st[(size_t)(3 * j + 2)];
  }
  *out = b.release();
}

int bsn_bed_from_fbm(const uint8_t *bytes, int64_t n, int64_t m, int64_t ld, bsn_bed **out) {
  return guarded([&] {
    double code[256];
    for (int c = 0; c < 256; c++) code[c] = c < 3 ? (double)c : std::numeric_limits<double>::quiet_NaN();
    fbm_open(bytes, n, m, ld, code, out);  // CODE_012, R/bigSNP-class.R:7
  });
}

int bsn_fbm_open(const uint8_t *bytes, int64_t n, int64_t m, int64_t ld, const double *code256, bsn_bed **out) {
  return guarded([&] { fbm_open(bytes, n, m, ld, code256, out); });
}

int bsn_bed_bits(const bsn_bed *bed) { return bed->bits; }

int64_t bsn_bed_na_known(const bsn_bed *bed) {
  if ((int64_t)bed->na_cnt.size() != bed->m) return -1;
  int64_t tot = 0;
  for (int32_t c : bed->na_cnt) {
    if (c < 0) return -1;
    tot += c;
  }
  return tot;
}

int bsn_bed_synthetic(int64_t n, int64_t m, uint32_t seed, uint32_t npop, uint32_t na16,
                      int64_t j_begin, bsn_bed **out) {
  return guarded([&] {
    require_gpu();
    std::unique_ptr<bsn_bed, void (*)(bsn_bed *)> b(new bsn_bed(), free_bed);
    image_alloc(b.get(), n, m);
    image_generate(b.get(), seed, npop ? npop : 1, na16, j_begin);
    if (na16 == 0) b->na_cnt.assign((size_t)m, 0);  // the generator draws no missing value then
    *out = b.release();
  });
}

int bsn_bed_close(bsn_bed *bed) {
  return guarded([&] {
    if (bed) {
      (void)hipSetDevice(bed->device);
      free_bed(bed);
    }
  });
}

int bsn_bed_tile(bsn_bed *bed, int *built) {
  return guarded([&] {
    BSN_HIP(hipSetDevice(bed->device));
    const bool ok = image_tile(bed);
    if (built) *built = ok ? 1 : 0;
  });
}

// Names (demangled, without the argument list: rocprofv3's Kernel_Name up to the parenthesis) of the streaming
// kernels the LAST profiled solve on this handle launched, one "kind=name" per line for the kinds cprod / prod /
// cprod_stats / warm.  Lets a measurement record be tied to the kernels of the running build.
int bsn_bed_streaming_kernels(bsn_bed *bed, char *buf, int64_t len) {
  return guarded([&] {
    if (!buf || len < 1) fail("bsn_bed_streaming_kernels: no buffer");
    buf[0] = 0;
    if (bed->last_solve_on_sub && bed->sub) bed = bed->sub;   // the last solve ran on the compacted copy: its operator lives there
    if (!bed->svd_op) return;
    static const char *kinds[kProfKinds] = {"cprod", "prod", "cprod_stats", "warm", "cprod_wide", "prod_wide"};
    std::string out;
    for (int k = 0; k < kProfKinds; k++) {
      const void *fn = bed->svd_op->prof_kernel[k];
      if (!fn) continue;
      const char *mangled = hipKernelNameRefByPtr(fn, bed->stream);
      if (!mangled) continue;
      int status = 1;
      char *dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
      std::string name = (status == 0 && dem) ? dem : mangled;
      free(dem);
      const size_t par = name.find('(');
      if (par != std::string::npos) name.resize(par);
      out += std::string(kinds[k]) + "=" + name + "\n";
    }
    snprintf(buf, (size_t)len, "%s", out.c_str());
  });
}

int bsn_bed_sample_major(bsn_bed *bed, int *built) {
  return guarded([&] {
    BSN_HIP(hipSetDevice(bed->device));
    const bool ok = image_smaj(bed);
    if (built) *built = ok ? 1 : 0;
  });
}

int bsn_bed_release_workspace(bsn_bed *bed) {
  return guarded([&] {
    BSN_HIP(hipSetDevice(bed->device));
    BSN_HIP(hipStreamSynchronize(bed->stream));
    bed->svd_op.reset();
    bed->svd_ws.reset();
    if (bed->d_tiled) {  // the streaming-layout copy is rebuilt by the next solve if there is room again
      BSN_HIP(hipFree(bed->d_tiled));
      bed->d_tiled = nullptr;
    }
    bed->tiled_tried = false;
    image_smaj_wait(bed);   // (a build in flight is adopted first, then freed with the rest)
    if (bed->d_smaj) {  // likewise the sample-major copy
      BSN_HIP(hipFree(bed->d_smaj));
      bed->d_smaj = nullptr;
    }
    bed->smaj_tried = false;
    bed->smaj_cap = 0;
    if (bed->sub) {     // the compacted sub-image of the last solve over a column list (and everything IT holds)
      bed_free(bed->sub);
      bed->sub = nullptr;
      bed->sub_key = 0;
      bed->sub_cols.clear();
      bed->sub_rows.clear();
      bed->last_solve_on_sub = false;
    }
    bed->stats_cache.release();   // the code counts over all samples (16 B per variant): counted again when next needed
    if (bed->slab_img) {   // out-of-core handle: the resident slab image and its page-locked staging buffers
      bed_free(bed->slab_img);
      bed->slab_img = nullptr;
    }
    if (bed->slab_stage) {
      delete (bsn::FileStage *)bed->slab_stage;
      bed->slab_stage = nullptr;
    }
    dev_cache_flush();
  });
}

int64_t bsn_bed_nrow(const bsn_bed *bed) { return bed->n; }
int64_t bsn_bed_ncol(const bsn_bed *bed) { return bed->m; }
int64_t bsn_bed_bytes(const bsn_bed *bed) { return bed->pitch * bed->m; }

int bsn_bed_download(bsn_bed *bed, uint8_t *payload_out) {
  return guarded([&] {
    BSN_HIP(hipSetDevice(bed->device));
    if (bed->streamed()) {   // the payload is the mapped file itself
      std::memcpy(payload_out, bed->h_map, (size_t)bed->n_byte * (size_t)bed->m);
      return;
    }
    image_download(bed, payload_out);
  });
}

int bsn_timer_start(bsn_bed *bed) {
  return guarded([&] { BSN_HIP(hipEventRecord(bed->ev0, bed->stream)); });
}
int bsn_timer_stop(bsn_bed *bed, double *ms) {
  return guarded([&] {
    BSN_HIP(hipEventRecord(bed->ev1, bed->stream));
    BSN_HIP(hipEventSynchronize(bed->ev1));
    float t = 0;
    BSN_HIP(hipEventElapsedTime(&t, bed->ev0, bed->ev1));
    *ms = t;
  });
}

}  // extern "C"
