// Host build of k_prodT's one-dimensional grid (bigsnpr_amd/csrc/prod_plan.hpp: plan_prod's whole-round fields, prodt_grid,
// prodt_slab — the text the kernel compiles) for tests/test_prodt_grid_cpu.py.
#include <cstdint>
#include <vector>

#include "prod_plan.hpp"

using namespace bsn;

static ProdFacts facts(const int64_t *f) {
  ProdFacts p;
  p.bits = (int)f[0], p.n = f[1], p.m = f[2], p.pitch = f[3], p.col0 = f[4], p.cols_contig = f[5] != 0, p.have_smaj = f[6] != 0;
  p.mode = (int)f[7], p.raw_na = f[8] != 0, p.has_q = f[9] != 0, p.no_sparse = f[10] != 0, p.nvec = (int)f[11], p.S = (int)f[12];
  p.ncu = (int)f[13], p.segmented = f[14] != 0, p.ky = (int)f[15], p.ky_t = (int)f[16], p.ky_whole = (int)f[17];
  return p;
}

extern "C" {
// facts: bits, n, m, pitch, col0, cols_contig, have_smaj, mode, raw_na, has_q, no_sparse, nvec, S, ncu, segmented, ky, ky_t, ky_whole
// out: refuse, smaj, vmax, m_pad, wgx, ky, smaj_cps, mc, sparse_ok, wgx_whole, ky_whole, cps_whole, workgroups of the grid
void pg_plan(const int64_t *f, int64_t *out) {
  const ProdPlan r = plan_prod(facts(f));
  out[0] = (int64_t)r.refuse, out[1] = r.smaj, out[2] = r.vmax, out[3] = r.m_pad, out[4] = r.wgx, out[5] = r.ky, out[6] = r.smaj_cps;
  out[7] = r.mc, out[8] = r.sparse_ok, out[9] = r.wgx_whole, out[10] = r.ky_whole, out[11] = r.cps_whole;
  out[12] = r.smaj ? prodt_workgroups(prodt_grid(r)) : 0;
}

// the workgroup wg of the plan's grid; out: sample block, slab, first chunk, end chunk
void pg_slab(const int64_t *f, int64_t wg, int64_t *out) {
  const ProdTSlab s = prodt_slab(prodt_grid(plan_prod(facts(f))), (uint32_t)wg);
  out[0] = s.bx, out[1] = s.slab, out[2] = s.ch_begin, out[3] = s.ch_end;
}

// Walks every workgroup of the plan's grid.  0: every (sample block, chunk) pair is covered exactly once, no slab is empty or
// beyond 2 500 000 variants, the slab index stays inside the accumulator, whole-round blocks come first, and wgx_whole is a
// whole number of rounds (none when the pass is segmented or has fewer blocks than CUs).  Otherwise the number of the rule broken.
int pg_check(const int64_t *f) {
  const ProdFacts p = facts(f);
  const ProdPlan r = plan_prod(p);
  if (r.refuse != ProdRefusal::none || !r.smaj) return -1;
  const ProdTGrid g = prodt_grid(r);
  const int64_t nchunks = r.m_pad / 512;
  if (g.nchunks != nchunks || g.wgx != r.wgx) return 1;
  if (r.wgx_whole % p.ncu != 0 || r.wgx_whole > r.wgx || (r.wgx_whole > 0 && r.wgx - r.wgx_whole >= p.ncu)) return 2;
  if ((p.segmented || r.wgx < p.ncu) && r.wgx_whole != 0) return 3;
  if (!p.segmented && r.wgx >= p.ncu && r.wgx_whole != r.wgx / p.ncu * p.ncu) return 4;
  if (r.wgx_whole > 0 && (r.ky_whole < 1 || (int64_t)r.ky_whole * 2500000 < r.m_pad)) return 5;
  if (r.wgx_whole == 0 && (r.ky_whole != 0 || r.cps_whole != 0)) return 6;
  const int slabs_acc = r.ky > r.ky_whole ? r.ky : r.ky_whole;   // slabs the accumulator of prod_planes holds
  std::vector<uint8_t> seen((size_t)(r.wgx * nchunks), 0);
  const int64_t W = prodt_workgroups(g);
  if (W != r.wgx_whole * r.ky_whole + (r.wgx - r.wgx_whole) * r.ky) return 7;
  bool in_rest = false;
  for (int64_t wg = 0; wg < W; wg++) {
    const ProdTSlab s = prodt_slab(g, (uint32_t)wg);
    if (s.bx < 0 || s.bx >= r.wgx || s.slab < 0 || s.slab >= slabs_acc) return 8;
    if (s.ch_begin >= s.ch_end || s.ch_begin < 0 || s.ch_end > nchunks) return 9;                 // an empty slab
    if ((int64_t)(s.ch_end - s.ch_begin) * 512 > 2500000) return 10;
    const bool rest = s.bx >= r.wgx_whole;
    if (s.slab >= (rest ? r.ky : r.ky_whole)) return 11;
    if (in_rest && !rest) return 12;                                                               // whole rounds first
    in_rest = rest;
    for (int ch = s.ch_begin; ch < s.ch_end; ch++)
      if (seen[(size_t)(s.bx * nchunks + ch)]++) return 13;                                        // covered twice
  }
  for (uint8_t v : seen)
    if (v != 1) return 14;                                                                         // not covered
  return 0;
}
}
