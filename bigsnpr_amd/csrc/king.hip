// king.hip — bed_king / bed_kingQC: the KING-robust kinship table of every pair of samples, on the device (bsn_bed_king,
// bsn_king_fetch, bsn_king_free, bsn_king_last_ms).
//
// Replaces the PLINK 2 run of snp_plinkKINGQC (R/external-software.R:520-590 of the reference: --make-king-table /
// --king-cutoff in a child process).  The statistic of a pair is five counts over the variants where both samples are
// called (king_step.hpp); they follow from seven plane products over the VARIANTS — the sums of the windowed-LD kernels
// (ld.hip) with samples and variants swapped, plus H.H — which are exact integer GEMMs on the int8 MFMA pipe over the
// sample-major copy of the image (bsn_internal.hpp, image_smaj): 16 bytes of it are 64 variants of one sample, one K-step.
//
//     k_king_pairs    64 x 64 sample pairs per workgroup -> the dense statistics of the tile pair (a stash that lives for
//                     one batch of tile pairs)
//     k_king_count    rows of the table per (sample i, column tile b): the segments of the result in the order (i, j)
//     k_king_scan     exclusive scan of those counts, one workgroup, fixed order
//     k_king_write    every segment writes its rows behind its offset
// No float atomics, no order that depends on the schedule: two calls return the same bytes.  DESIGN.md 3.5n.
// The walk over the batches of tile pairs (kingwalk::pairs_walk, king_walk.hpp) is shared with bed_ibd (ibd.hip), whose
// table is another reading of the same stash: what a row is and which pairs pass is the caller's PairSink.
#include <algorithm>
#include <memory>
#include <vector>

#include "bsn_internal.hpp"
#include "king_step.hpp"
#include "king_walk.hpp"
#include "plane_decode.hpp"

struct bsn_king {
  bsn_bed *bed = nullptr;   // the handle whose staging buffers serve the download
  int64_t count = 0, cap = 0;
  std::unique_ptr<bsn::DevBuf<int32_t>> d_i1, d_i2, d_cnt;   // count, count, 5 x count (row k at 5 k)
  std::unique_ptr<bsn::DevBuf<double>> d_kin;
};

namespace bsn {
namespace {

using namespace kingwalk;   // KT, kBatchTiles, the stash, Batch, PairSink

// device milliseconds of the last call of this process (bsn_king_last_ms): the operand (gathered selection, sample-major
// copy, row list), the per-sample totals of the complete-data path (0 on the general path), the pair kernel, the compaction
double g_last_ms[4] = {0.0, 0.0, 0.0, 0.0};

// The operand as the kernels read it: position p of the (padded) sample list is row rows[p] (NULL: p) of the sample-major
// copy, whose 128 bytes "variants 512 ch .. 512 ch + 511 of row r" sit at (ch * rows_smaj + r) * 128.
struct Operand {
  const uint8_t *smaj;
  int64_t rows_smaj;
  const int32_t *rows;
  int nit;            // K-iterations of 64 bytes (256 variants) per sample: two per chunk
  int32_t m, pad;     // selected variants; variants of the last chunk past m (code 0: called, homozygous)
  const int32_t *tot; // complete data: sum x, sum x^2 of position p at 2 p, 2 p + 1
};

__device__ __forceinline__ const uint8_t *row_ptr(const Operand &op, int64_t p) {
  const int64_t r = op.rows ? (int64_t)op.rows[p] : p;
  return op.smaj + r * 128;
}

// sum x and sum x^2 of every operand position over the selected variants (the codes of the pad variants are 0): what
// x.P and x^2.P of a pair are when no call is missing.  One workgroup per position, integer adds only.
__global__ __launch_bounds__(256) void k_king_totals(Operand op, int32_t *__restrict__ tot) {
  __shared__ int32_t s[2];
  const int tid = threadIdx.x;
  if (tid < 2) s[tid] = 0;
  __syncthreads();
  const uint8_t *base = row_ptr(op, blockIdx.x);
  const int64_t cs = op.rows_smaj * 128;
  const int nw = (op.nit >> 1) * 32;   // 32-bit words of the position
  int32_t sx = 0, sx2 = 0;
  for (int w = tid; w < nw; w += 256) {
    const uint32_t v = *(const uint32_t *)(base + (int64_t)(w >> 5) * cs + (w & 31) * 4);
    const uint32_t lo = v & 0x55555555u, hi = (v >> 1) & 0x55555555u;
    const int one = __popc(lo & ~hi), two = __popc(hi & ~lo);
    sx += one + 2 * two;
    sx2 += one + 4 * two;
  }
  atomicAdd(&s[0], sx);
  atomicAdd(&s[1], sx2);
  __syncthreads();
  if (tid < 2) tot[2 * (int64_t)blockIdx.x + tid] = s[tid];
}

// One tile pair (a, b) = tiles[block]: rows are the 64 samples of tile a, columns those of tile b.  Wave w owns the rows
// 16 w .. 16 w + 15 (decoded privately) and multiplies them with all 64 columns, whose planes are decoded once per
// workgroup — wave w decodes column sub-tile w — and shared through LDS (the shape of k_pair_stats_b).  NA: the seven
// products of the general path; otherwise x.x and H.H alone, the other sums being the per-sample totals.
// stash: counts [tile pair][5][row][col], kinship [tile pair][row][col]; every entry is written, pad samples and the lower
// triangle included (the compaction does not read them).
template <bool NA>
__global__ __launch_bounds__(256, 2) void k_king_pairs(Operand op, const int2 *__restrict__ tiles, int32_t *__restrict__ st_cnt,
                                                       double *__restrict__ st_kin) {
  constexpr int NP = NA ? 4 : 2;   // planes of an operand: x, H (, x^2, P)
  constexpr int NQ = NA ? 7 : 2;   // products
  __shared__ uint4 sB[4][4][NP][64];   // [K-step][column sub-tile][plane][lane]: 64 KB / 32 KB
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, g = lane >> 4;
  const int2 t = tiles[blockIdx.x];
  const uint8_t *pa = row_ptr(op, (int64_t)t.x * KT + wave * 16 + r16) + g * 16;
  const uint8_t *pb = row_ptr(op, (int64_t)t.y * KT + wave * 16 + r16) + g * 16;
  const int64_t cs = op.rows_smaj * 128;
  v4i acc[4][NQ];
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int q = 0; q < NQ; q++) acc[j][q] = v4i{0, 0, 0, 0};
  auto as_u4 = [](const v4i &v) { return uint4{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]}; };
  auto as_v4 = [](const uint4 &v) { return v4i{(int)v.x, (int)v.y, (int)v.z, (int)v.w}; };
  uint4 a = *(const uint4 *)pa, b = *(const uint4 *)pb;
  for (int it = 0; it < op.nit; it++) {
    // the next iteration's words (past the end the last one again: no branch around loads)
    const int itn = it + 1 < op.nit ? it + 1 : it;
    const int64_t off = (int64_t)(itn >> 1) * cs + (itn & 1) * 64;
    const uint4 an = *(const uint4 *)(pa + off), bn = *(const uint4 *)(pb + off);
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const Fields f = fields(d == 0 ? b.x : d == 1 ? b.y : d == 2 ? b.z : b.w);
      sB[d][wave][0][lane] = as_u4(plane(kLX, f));
      sB[d][wave][1][lane] = as_u4(plane(kLH, f));
      if constexpr (NA) {
        sB[d][wave][2][lane] = as_u4(plane(kLX2, f));
        sB[d][wave][3][lane] = as_u4(plane(kLM, f));
      }
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const Fields f = fields(d == 0 ? a.x : d == 1 ? a.y : d == 2 ? a.z : a.w);
      const v4i Ax = plane(kLX, f), Ah = plane(kLH, f);
      v4i Ax2 = Ax, Am = Ax;
      if constexpr (NA) {
        Ax2 = plane(kLX2, f);
        Am = plane(kLM, f);
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const v4i Bx = as_v4(sB[d][j][0][lane]), Bh = as_v4(sB[d][j][1][lane]);
        acc[j][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Ax, Bx, acc[j][0], 0, 0, 0);
        acc[j][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Ah, Bh, acc[j][1], 0, 0, 0);
        if constexpr (NA) {
          const v4i Bx2 = as_v4(sB[d][j][2][lane]), Bm = as_v4(sB[d][j][3][lane]);
          acc[j][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Ax, Bm, acc[j][2], 0, 0, 0);
          acc[j][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Ax2, Bm, acc[j][3], 0, 0, 0);
          acc[j][4] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Am, Bx, acc[j][4], 0, 0, 0);
          acc[j][5] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Am, Bx2, acc[j][5], 0, 0, 0);
          acc[j][6] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Am, Bm, acc[j][6], 0, 0, 0);
        }
      }
    }
    __syncthreads();   // every wave has read the planes before the next iteration overwrites them
    a = an;
    b = bn;
  }
  int32_t *oc = st_cnt + (size_t)blockIdx.x * kStashCnt;
  double *ok = st_kin + (size_t)blockIdx.x * kStashKin;
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = wave * 16 + 4 * g + r, col = j * 16 + r16;
      king::Sums s;
      s.xx = acc[j][0][r];
      s.hh = acc[j][1][r];
      if constexpr (NA) {
        s.xP = acc[j][2][r];
        s.x2P = acc[j][3][r];
        s.Px = acc[j][4][r];
        s.Px2 = acc[j][5][r];
        s.PP = acc[j][6][r] - op.pad;
      } else {
        const int64_t pi = (int64_t)t.x * KT + row, pj = (int64_t)t.y * KT + col;
        s.xP = op.tot[2 * pi];
        s.x2P = op.tot[2 * pi + 1];
        s.Px = op.tot[2 * pj];
        s.Px2 = op.tot[2 * pj + 1];
        s.PP = op.m;
      }
      const king::Pair p = king::pair_from_sums(s);
      const int e = row * KT + col;
      oc[0 * KT * KT + e] = p.nsnp;
      oc[1 * KT * KT + e] = p.hethet;
      oc[2 * KT * KT + e] = p.ibs0;
      oc[3 * KT * KT + e] = p.het1hom2;
      oc[4 * KT * KT + e] = p.het2hom1;
      ok[e] = p.kinship;
    }
}

// is the lane's pair of the segment (king_walk.hpp) a row of the table?
__device__ __forceinline__ bool seg_row(const Batch &B, const double *__restrict__ st_kin, int64_t seg, int lane, int64_t &i, int64_t &j,
                                        size_t &slot, int &e) {
  if (!seg_pair(B, seg, lane, i, j, slot, e)) return false;
  return !B.filter || king::passes(st_kin[slot * kStashKin + e], B.thr);
}

__global__ __launch_bounds__(256) void k_king_count(Batch B, const double *__restrict__ st_kin, int64_t nseg, int32_t *__restrict__ cnt) {
  const int64_t seg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const int lane = threadIdx.x & 63;
  int64_t i, j;
  size_t slot;
  int e;
  const bool keep = seg_row(B, st_kin, seg, lane, i, j, slot, e);
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) cnt[seg] = __popcll(bal);
}

// off[s] = cnt[0] + ... + cnt[s - 1], *total = the sum of all; one workgroup, thread t sums the t-th run of segments
__global__ __launch_bounds__(1024) void k_king_scan(const int32_t *__restrict__ cnt, int64_t nseg, int64_t *__restrict__ off,
                                                    int64_t *__restrict__ total) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t per = (nseg + 1023) / 1024, s0 = t * per < nseg ? t * per : nseg, s1 = s0 + per < nseg ? s0 + per : nseg;
  int64_t sum = 0;
  for (int64_t s = s0; s < s1; s++) sum += cnt[s];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int64_t v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int64_t at = part[t] - sum;
  for (int64_t s = s0; s < s1; s++) {
    off[s] = at;
    at += cnt[s];
  }
  if (t == 1023) *total = part[1023];
}

__global__ __launch_bounds__(256) void k_king_write(Batch B, const int32_t *__restrict__ st_cnt, const double *__restrict__ st_kin,
                                                    int64_t nseg, const int64_t *__restrict__ off, int64_t base, int32_t *__restrict__ i1,
                                                    int32_t *__restrict__ i2, int32_t *__restrict__ counts, double *__restrict__ kin) {
  const int64_t seg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const int lane = threadIdx.x & 63;
  int64_t i, j;
  size_t slot = 0;
  int e = 0;
  const bool keep = seg_row(B, st_kin, seg, lane, i, j, slot, e);
  const unsigned long long bal = __ballot(keep);
  if (!keep) return;
  const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
  const int64_t k = base + off[seg] + rank;
  i1[k] = (int32_t)i;
  i2[k] = (int32_t)j;
#pragma unroll
  for (int q = 0; q < 5; q++) counts[5 * k + q] = st_cnt[slot * kStashCnt + (size_t)q * KT * KT + e];
  kin[k] = st_kin[slot * kStashKin + e];
}

// the table's buffers hold at least `need` rows (the first `keep` rows survive a move); refuses by name without the room
void table_reserve(bsn_king *K, int64_t need, int64_t keep, hipStream_t st) {
  if (need <= K->cap) return;
  const int64_t cap = std::max<int64_t>(std::max<int64_t>(need, 2 * K->cap), 1 << 16);
  const double bytes = 36.0 * (double)cap;
  size_t free_b = 0, total_b = 0;
  BSN_HIP(hipMemGetInfo(&free_b, &total_b));
  if ((double)(free_b + dev_cache_held()) < bytes + 256e6)
    fail("bed_king: a table of %lld rows does not fit in device memory (%.1f GB for it, %.1f GB free); raise the kinship "
         "threshold or select fewer samples",
         (long long)need, bytes / 1e9, (double)free_b / 1e9);
  auto n_i1 = std::make_unique<DevBuf<int32_t>>(), n_i2 = std::make_unique<DevBuf<int32_t>>(), n_cnt = std::make_unique<DevBuf<int32_t>>();
  auto n_kin = std::make_unique<DevBuf<double>>();
  n_i1->ensure((size_t)cap);
  n_i2->ensure((size_t)cap);
  n_cnt->ensure((size_t)5 * cap);
  n_kin->ensure((size_t)cap);
  if (keep > 0) {
    BSN_HIP(hipMemcpyAsync(n_i1->p, K->d_i1->p, (size_t)keep * 4, hipMemcpyDeviceToDevice, st));
    BSN_HIP(hipMemcpyAsync(n_i2->p, K->d_i2->p, (size_t)keep * 4, hipMemcpyDeviceToDevice, st));
    BSN_HIP(hipMemcpyAsync(n_cnt->p, K->d_cnt->p, (size_t)keep * 20, hipMemcpyDeviceToDevice, st));
    BSN_HIP(hipMemcpyAsync(n_kin->p, K->d_kin->p, (size_t)keep * 8, hipMemcpyDeviceToDevice, st));
    BSN_HIP(hipStreamSynchronize(st));
  }
  K->d_i1 = std::move(n_i1);
  K->d_i2 = std::move(n_i2);
  K->d_cnt = std::move(n_cnt);
  K->d_kin = std::move(n_kin);
  K->cap = cap;
}

// the rows of bed_king's table: the stash's own columns, filtered by the kinship
struct KingSink final : PairSink {
  bsn_king *K;
  explicit KingSink(bsn_king *k) : K(k) {}
  void reserve(int64_t need, int64_t keep, hipStream_t st) override { table_reserve(K, need, keep, st); }
  void count(const Batch &B, const int32_t *, const double *st_kin, int64_t nseg, int32_t *cnt, hipStream_t st) override {
    hipLaunchKernelGGL(k_king_count, dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, st, B, st_kin, nseg, cnt);
    BSN_HIP(hipGetLastError());
  }
  void write(const Batch &B, const int32_t *st_cnt, const double *st_kin, int64_t nseg, const int64_t *off, int64_t base,
             hipStream_t st) override {
    hipLaunchKernelGGL(k_king_write, dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, st, B, st_cnt, st_kin, nseg, off, base, K->d_i1->p,
                       K->d_i2->p, K->d_cnt->p, K->d_kin->p);
    BSN_HIP(hipGetLastError());
  }
};

}  // namespace

namespace kingwalk {

void pairs_check(bsn_bed *bed, int64_t n, int64_t m, const char *what) {
  require_gpu();
  if (!bed) fail("%s: null argument", what);
  refuse_generic(bed, what);
  require_bits(bed, 2, what);
  require_resident(bed, what);
  if (n < 2) fail("%s: at least 2 samples are needed to form a pair ('ind.row' holds %lld)", what, (long long)n);
  if (m < 1) fail("%s: at least 1 variant is needed ('ind.col' holds %lld)", what, (long long)m);
  if (m > king::kMaxVariants)
    fail("%s: %lld variants: the int32 plane sums are exact for fewer than 2^29 variants only", what, (long long)m);
}

int64_t pairs_walk(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, double thr, int filter,
                   const char *what, PairSink &sink, double ms[4]) {
  pairs_check(bed, n, m, what);
  BSN_HIP(hipSetDevice(bed->device));
  // (no list: the first n samples, whose positions are their rows)
  bool rows_ident = true, cols_all = m == bed->m;
  if (!ind_row && n > bed->n) fail("Tested %lld < %lld. Subscript out of bounds (ind.row).", (long long)(n - 1), (long long)bed->n);
  for (int64_t i = 0; ind_row && i < n; i++) {
    const int64_t r = ind_row[i];
    if (r < 0 || r >= bed->n) fail("Tested %lld < %lld. Subscript out of bounds (ind.row).", (long long)r, (long long)bed->n);
    rows_ident = rows_ident && r == i;
  }
  bool complete = (int64_t)bed->na_cnt.size() == bed->m && !getenv("BSN_KING_GENERAL");
  for (int64_t j = 0; j < m; j++) {
    const int64_t c = ind_col ? ind_col[j] : j;
    if (c < 0 || c >= bed->m) fail("Tested %lld < %lld. Subscript out of bounds (ind.col).", (long long)c, (long long)bed->m);
    cols_all = cols_all && c == j;
    complete = complete && bed->na_cnt[(size_t)c] == 0;
  }

  // ---- the operand: the handle's own sample-major copy (all variants in file order; a row list selects its rows), or
  // the copy of a gathered image of the selection
  EventMarks<2> evo;
  evo.mark(0, bed->stream);
  std::unique_ptr<bsn_bed, void (*)(bsn_bed *)> sub(nullptr, bed_free);
  bsn_bed *src = bed;
  if (!cols_all) {
    sub.reset(image_gather(bed, ind_row, n, ind_col, m));
    src = sub.get();
    rows_ident = true;
  }
  hipStream_t st = src->stream;
  const int T = (int)((n + KT - 1) / KT);
  const int64_t npad = (int64_t)T * KT;
  DevBuf<int32_t> d_rows;
  if (!rows_ident) {
    std::vector<int32_t> rows((size_t)npad, (int32_t)ind_row[0]);   // pad positions repeat a valid row: never a table row
    for (int64_t i = 0; i < n; i++) rows[(size_t)i] = (int32_t)ind_row[i];
    copy_h2d(src, d_rows.ensure((size_t)npad), rows.data(), (size_t)npad * 4);
  }
  if (!image_smaj(src))
    fail("%s: no room for the sample-major operand of the selection (%.1f GB beside the image; BSN_NO_SMAJ forbids it too)", what,
         (double)round_up(src->n, 256) * (double)round_up((src->m + 3) / 4 + 128, 256) / 1e9);
  evo.mark(1, st);
  const int64_t nch = (m + 511) / 512;
  Operand op;
  op.smaj = src->d_smaj;
  op.rows_smaj = src->rows_smaj;
  op.rows = rows_ident ? nullptr : d_rows.p;
  op.nit = (int)(2 * nch);
  op.m = (int32_t)m;
  op.pad = (int32_t)(nch * 512 - m);
  op.tot = nullptr;
  if (nch * 128 > src->pitch_smaj || npad > src->rows_smaj) fail("internal: sample-major copy smaller than the selection");

  EventMarks<5> ev;
  DevBuf<int32_t> d_tot;
  if (complete) {
    ev.mark(0, st);
    hipLaunchKernelGGL(k_king_totals, dim3((unsigned)npad), dim3(256), 0, st, op, d_tot.ensure((size_t)2 * npad));
    BSN_HIP(hipGetLastError());
    ev.mark(1, st);
    op.tot = d_tot.p;
  }

  // ---- batches of whole tile rows
  std::vector<int> cut{0};
  int max_tiles = 0, max_rows = 0;
  for (int a = 0; a < T;) {
    int tiles = 0, a1 = a;
    do {
      tiles += T - a1;
      a1++;
    } while (a1 < T && tiles + (T - a1) <= kBatchTiles);
    max_tiles = std::max(max_tiles, tiles);
    max_rows = std::max(max_rows, a1 - a);
    cut.push_back(a1);
    a = a1;
  }
  const int64_t max_seg = (int64_t)max_rows * KT * T;
  DevBuf<int2> d_tiles;
  DevBuf<int32_t> d_stc, d_segcnt;
  DevBuf<double> d_stk;
  DevBuf<int64_t> d_off;   // [max_seg] offsets, then the batch total
  d_tiles.ensure((size_t)max_tiles);
  d_stc.ensure((size_t)max_tiles * kStashCnt);
  d_stk.ensure((size_t)max_tiles * kStashKin);
  d_segcnt.ensure((size_t)max_seg);
  d_off.ensure((size_t)max_seg + 1);

  int64_t count = 0;
  if (!filter) sink.reserve(n * (n - 1) / 2, 0, st);
  BSN_HIP(hipStreamSynchronize(st));
  ms[0] += evo.ms(0, 1);
  if (complete) ms[1] += ev.ms(0, 1);

  std::vector<int2> tiles;
  for (size_t c = 0; c + 1 < cut.size(); c++) {
    const int a0 = cut[c], a1 = cut[c + 1];
    tiles.clear();
    for (int a = a0; a < a1; a++)
      for (int b = a; b < T; b++) tiles.push_back(int2{a, b});
    copy_h2d(src, d_tiles.p, tiles.data(), tiles.size() * sizeof(int2));
    Batch B;
    B.a0 = a0;
    B.T = T;
    B.i0 = (int64_t)a0 * KT;
    B.i1 = std::min<int64_t>((int64_t)a1 * KT, n);
    B.n = n;
    B.thr = thr;
    B.filter = filter ? 1 : 0;
    const int64_t nseg = (B.i1 - B.i0) * T;
    ev.mark(0, st);
    if (complete)
      hipLaunchKernelGGL(k_king_pairs<false>, dim3((unsigned)tiles.size()), dim3(256), 0, st, op, d_tiles.p, d_stc.p, d_stk.p);
    else
      hipLaunchKernelGGL(k_king_pairs<true>, dim3((unsigned)tiles.size()), dim3(256), 0, st, op, d_tiles.p, d_stc.p, d_stk.p);
    BSN_HIP(hipGetLastError());
    ev.mark(1, st);
    sink.count(B, d_stc.p, d_stk.p, nseg, d_segcnt.p, st);
    hipLaunchKernelGGL(k_king_scan, dim3(1), dim3(1024), 0, st, d_segcnt.p, nseg, d_off.p, d_off.p + max_seg);
    BSN_HIP(hipGetLastError());
    ev.mark(2, st);
    int64_t rows_batch = 0;
    copy_d2h(src, &rows_batch, d_off.p + max_seg, 8);
    BSN_HIP(hipStreamSynchronize(st));
    sink.reserve(count + rows_batch, count, st);
    ev.mark(3, st);
    if (rows_batch > 0) sink.write(B, d_stc.p, d_stk.p, nseg, d_off.p, count, st);
    ev.mark(4, st);
    BSN_HIP(hipStreamSynchronize(st));
    ms[2] += ev.ms(0, 1);
    ms[3] += ev.ms(1, 2) + ev.ms(3, 4);
    count += rows_batch;
  }
  return count;
}

}  // namespace kingwalk

namespace {

void bed_king(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, double thr, int filter,
              int64_t *count_out, bsn_king **out) {
  if (!bed || !count_out || !out) fail("bed_king: null argument");
  std::unique_ptr<bsn_king> K(new bsn_king());
  K->bed = bed;
  K->d_i1 = std::make_unique<DevBuf<int32_t>>();
  K->d_i2 = std::make_unique<DevBuf<int32_t>>();
  K->d_cnt = std::make_unique<DevBuf<int32_t>>();
  K->d_kin = std::make_unique<DevBuf<double>>();
  KingSink sink(K.get());
  double ms[4] = {0.0, 0.0, 0.0, 0.0};
  K->count = pairs_walk(bed, ind_row, n, ind_col, m, thr, filter, "bed_king", sink, ms);
  for (int q = 0; q < 4; q++) g_last_ms[q] = ms[q];
  *count_out = K->count;
  *out = K.release();
}

}  // namespace
}  // namespace bsn

extern "C" {

int bsn_bed_king(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, double thr, int filter,
                 int64_t *count, bsn_king **out) {
  return bsn::guarded([&] { bsn::bed_king(bed, ind_row, n, ind_col, m, thr, filter, count, out); });
}

int bsn_king_fetch(bsn_king *k, int32_t *i1, int32_t *i2, int32_t *counts, double *kinship) {
  return bsn::guarded([&] {
    if (k->count <= 0) return;
    BSN_HIP(hipSetDevice(k->bed->device));
    bsn::copy_d2h(k->bed, i1, k->d_i1->p, (size_t)k->count * 4);
    bsn::copy_d2h(k->bed, i2, k->d_i2->p, (size_t)k->count * 4);
    bsn::copy_d2h(k->bed, counts, k->d_cnt->p, (size_t)k->count * 20);
    bsn::copy_d2h(k->bed, kinship, k->d_kin->p, (size_t)k->count * 8);
  });
}

int bsn_king_free(bsn_king *k) {
  return bsn::guarded([&] { delete k; });
}

int bsn_king_last_ms(double *ms_out) {
  return bsn::guarded([&] {
    for (int q = 0; q < 4; q++) ms_out[q] = bsn::g_last_ms[q];
  });
}

}  // extern "C"
