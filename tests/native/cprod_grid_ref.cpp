// Host build of k_cprod's one-dimensional grid (bigsnpr_amd/csrc/prod_plan.hpp: plan_cprod, cprod_slab — the text the kernel
// compiles — cprod_workgroups, cprod_partial_words) for tests/test_cprod_grid_cpu.py.
#include <cstdint>
#include <vector>

#include "prod_plan.hpp"

using namespace bsn;

static CprodGridFacts facts(const int64_t *f) {
  CprodGridFacts p;
  p.m = f[0], p.per_wg = (int)f[1], p.nchunks = (int)f[2], p.pitch = f[3], p.NB = (int)f[4], p.nplane = (int)f[5];
  p.ncu = (int)f[6], p.resident = (int)f[7], p.one_split = f[8] != 0, p.slabs = (int)f[9];
  return p;
}

extern "C" {
// facts: m, per_wg, nchunks, pitch, NB, nplane, ncu, resident, one_split, slabs (0: the rule)
// out: blocks, blocks_whole, slabs, cps, nchunks, m_rem, workgroups of the grid, int32 words of the partial region
void cg_plan(const int64_t *f, int64_t *out) {
  const CprodGridFacts p = facts(f);
  const CprodGrid g = plan_cprod(p);
  out[0] = g.blocks, out[1] = g.blocks_whole, out[2] = g.slabs, out[3] = g.cps, out[4] = g.nchunks, out[5] = g.m_rem;
  out[6] = cprod_workgroups(g), out[7] = cprod_partial_words(g, p.nplane, p.NB);
}

// the workgroup wg of the plan's grid; out: block, slab, first chunk, end chunk
void cg_slab(const int64_t *f, int64_t wg, int64_t *out) {
  const CprodSlab s = cprod_slab(plan_cprod(facts(f)), (uint32_t)wg);
  out[0] = s.block, out[1] = s.slab, out[2] = s.ch_begin, out[3] = s.ch_end;
}

// Walks every workgroup of the plan's grid, writing where k_cprod writes.  0: every (block, chunk) pair is covered exactly
// once; the slabs of a remainder block are non-empty, contiguous and in slab order; whole-round blocks come first, each over
// all chunks, and are a whole number of rounds of ncu x resident; every word of the partial region
// [slab][plane][variant - first remainder variant][16 NB] is written exactly once and none beyond the size the planner
// reports; the old geometry stays where the issue of a split does not arise (whole rounds, one chunk, the switch).
// Otherwise the number of the rule broken.
int cg_check(const int64_t *f) {
  const CprodGridFacts p = facts(f);
  const CprodGrid g = plan_cprod(p);
  const int64_t blocks = (p.m + p.per_wg - 1) / p.per_wg, slots = (int64_t)p.ncu * p.resident;
  if (g.blocks != blocks || g.nchunks != p.nchunks) return 1;
  const bool split = g.blocks_whole < g.blocks;
  if (!split && (g.slabs != 0 || g.cps != 0 || g.m_rem != 0 || g.blocks_whole != g.blocks)) return 2;
  if ((p.one_split || blocks % slots == 0 || p.nchunks <= 1 || p.slabs == 1) && split) return 3;
  if (split) {
    if (g.blocks_whole != blocks / slots * slots) return 4;
    if (g.slabs < 2 || g.slabs > (p.slabs > 0 ? p.nchunks : kCprodMaxSlabs) || g.cps < 1) return 5;
    if ((int64_t)(g.slabs - 1) * g.cps >= p.nchunks || (int64_t)g.slabs * g.cps < p.nchunks) return 6;   // the last slab is not empty
    if (g.m_rem != p.m - (int64_t)g.blocks_whole * p.per_wg || g.m_rem < 1) return 7;
  }
  const int64_t W = cprod_workgroups(g);
  if (W != g.blocks_whole + (int64_t)(g.blocks - g.blocks_whole) * g.slabs) return 8;
  const int ncol = 16 * p.NB;
  const int64_t words = cprod_partial_words(g, p.nplane, p.NB);
  if (words != (int64_t)g.slabs * p.nplane * g.m_rem * ncol) return 9;
  std::vector<uint8_t> seen((size_t)(blocks * p.nchunks), 0), part((size_t)words, 0);
  std::vector<int> next_chunk((size_t)blocks, 0), next_slab((size_t)blocks, 0);
  bool in_rest = false;
  for (int64_t wg = 0; wg < W; wg++) {
    const CprodSlab s = cprod_slab(g, (uint32_t)wg);
    if (s.block < 0 || s.block >= blocks) return 10;
    if (s.ch_begin >= s.ch_end || s.ch_begin < 0 || s.ch_end > p.nchunks) return 11;             // an empty slab
    const bool rest = s.block >= g.blocks_whole;
    if (in_rest && !rest) return 12;                                                           // whole rounds first
    in_rest = rest;
    if (!rest && (s.slab != 0 || s.ch_begin != 0 || s.ch_end != p.nchunks)) return 13;
    if (rest && (s.slab < 0 || s.slab >= g.slabs)) return 14;
    if (s.ch_begin != next_chunk[(size_t)s.block] || s.slab != next_slab[(size_t)s.block]) return 15;   // contiguous, in order
    next_chunk[(size_t)s.block] = s.ch_end, next_slab[(size_t)s.block]++;
    for (int ch = s.ch_begin; ch < s.ch_end; ch++)
      if (seen[(size_t)(s.block * (int64_t)p.nchunks + ch)]++) return 16;                        // covered twice
    if (rest) {
      // the stores of k_cprod: variants j of the block below m, every plane, every column
      const int64_t j0 = p.m - g.m_rem;
      for (int64_t j = (int64_t)s.block * p.per_wg; j < (int64_t)(s.block + 1) * p.per_wg && j < p.m; j++)
        for (int pl = 0; pl < p.nplane; pl++)
          for (int c = 0; c < ncol; c++) {
            const int64_t at = (((int64_t)s.slab * p.nplane + pl) * g.m_rem + (j - j0)) * ncol + c;
            if (j < j0 || at < 0 || at >= words) return 17;                                    // beyond the region
            if (part[(size_t)at]++) return 18;                                                 // written twice
          }
    }
  }
  for (uint8_t v : seen)
    if (v != 1) return 19;                                                                     // not covered
  for (uint8_t v : part)
    if (v != 1) return 20;                                                                     // a word nobody writes
  return 0;
}
}
