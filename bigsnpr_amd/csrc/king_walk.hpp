// king_walk.hpp — the walk over all pairs of samples that bed_king (king.hip) and bed_ibd (ibd.hip) share: the sample-major
// operand of the selection, the batches of whole tile rows, k_king_pairs over every batch into the stash, and the
// compaction of the stash into a table (count per segment, k_king_scan, write behind the offsets).  What a row of the table
// is, and which pairs pass, is the caller's: a PairSink.  The walk itself lives in king.hip.
#pragma once
#include "bsn_internal.hpp"

namespace bsn {
namespace kingwalk {

constexpr int KT = 64;                   // samples per tile edge
constexpr int kBatchTiles = 2048;        // tile pairs whose dense statistics are held at once (28 B x 4096 each: 235 MB)
// the stash of one tile pair: counts [5][row][col] (NSNP, HETHET, IBS0, HET1HOM2, HET2HOM1), kinship [row][col]
constexpr size_t kStashCnt = (size_t)5 * KT * KT, kStashKin = (size_t)KT * KT;

// A batch holds the tile rows a0 .. a1 - 1, tile row a with its T - a tile pairs (a, a), (a, a + 1), ... in that order.
struct Batch {
  int a0, T;
  int64_t i0, i1, n;   // the samples (positions of ind_row) i0 <= i < i1 of the batch; n: all samples
  double thr;
  int filter;
};
__device__ __forceinline__ int64_t tile_slot(const Batch &B, int a, int b) {
  const int64_t k = a - B.a0;
  return k * B.T - k * (2 * (int64_t)B.a0 + k - 1) / 2 + (b - a);
}
// segment = (sample i of the batch, column tile b), one wave each: the lane's pair is (i, 64 b + lane).  False where that
// is no pair i < j < n of the upper tile triangle; otherwise its tile pair's slot in the stash and its entry there.
__device__ __forceinline__ bool seg_pair(const Batch &B, int64_t seg, int lane, int64_t &i, int64_t &j, size_t &slot, int &e) {
  i = B.i0 + seg / B.T;
  const int b = (int)(seg % B.T), a = (int)(i / KT);
  j = (int64_t)b * KT + lane;
  if (b < a || j <= i || j >= B.n) return false;
  slot = (size_t)tile_slot(B, a, b);
  e = (int)(i - (int64_t)a * KT) * KT + lane;
  return true;
}

// The table a walk fills.  Segments are numbered as seg_pair reads them, four to a workgroup of 256.
struct PairSink {
  virtual ~PairSink() = default;
  // room for `need` rows, the first `keep` of which survive a move; refuses by name without it
  virtual void reserve(int64_t need, int64_t keep, hipStream_t st) = 0;
  // cnt[seg] = the rows of segment seg
  virtual void count(const Batch &B, const int32_t *st_cnt, const double *st_kin, int64_t nseg, int32_t *cnt, hipStream_t st) = 0;
  // every segment writes its rows at base + off[seg], ascending in j
  virtual void write(const Batch &B, const int32_t *st_cnt, const double *st_kin, int64_t nseg, const int64_t *off, int64_t base,
                     hipStream_t st) = 0;
};

// the argument checks of a walk, refusing by name as `what` (a caller with work of its own before the walk runs them first)
void pairs_check(bsn_bed *bed, int64_t n, int64_t m, const char *what);
// Walks every pair i < j of the positions of ind_row over the variants ind_col and returns the rows of the table.
// thr / filter reach the sink through Batch.  ms[4] += operand, per-sample totals, pair kernel, compaction (device ms).
int64_t pairs_walk(bsn_bed *bed, const int64_t *ind_row, int64_t n, const int64_t *ind_col, int64_t m, double thr, int filter,
                   const char *what, PairSink &sink, double ms[4]);

}  // namespace kingwalk
}  // namespace bsn
