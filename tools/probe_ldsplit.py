#!/usr/bin/env python3
"""snp_ldsplit at config C5 -> profiles/ldsplit_c5.json.

LD matrix: bed_cor of the C5 image (400K x 100K synthetic .bed), size = 3/1000 on cM positions with Exp(mean 1.5e-3 cM)
gaps, as tools/probe_lassosum2.py builds it.  One dynamic program with thr_r2 0.05, min_size 50,
max_size 3000, max_K 500, max_r2 0.3 and the default max_cost (m / 200, clamped) runs on the device; its time is recorded
for E (with the suffix sums), the levels and the epilogue.  The CPU statement (tests/native/ldsplit_ref.cpp, one thread)
runs the same program with --cpu-max-K levels (fewer than the device's unless asked otherwise: the record says how many);
every output is compared over the levels both have.

    python tools/probe_ldsplit.py [--n 400000] [--m 100000] [--cpu-max-K 40] [--out profiles/ldsplit_c5.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
import numpy as np  # noqa: E402

import bigsnpr_amd as ba  # noqa: E402
import ldsplit_ref as ref  # noqa: E402
from bigsnpr_amd.ldsplit import clamp_max_cost, ldsplit_one  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400000)
    ap.add_argument("--m", type=int, default=100000)
    ap.add_argument("--thr-r2", type=float, default=0.05)
    ap.add_argument("--min-size", type=int, default=50)
    ap.add_argument("--max-size", type=int, default=3000)
    ap.add_argument("--max-K", type=int, default=500)
    ap.add_argument("--max-r2", type=float, default=0.3)
    ap.add_argument("--cpu-max-K", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldsplit_c5.json"))
    a = ap.parse_args()
    rec = dict(config="C5", n=a.n, m=a.m, size_cM=3.0, thr_r2=a.thr_r2, min_size=a.min_size, max_size=a.max_size, max_K=a.max_K,
               max_r2=a.max_r2)
    rng = np.random.default_rng(20261016)
    gb = ba.bed.synthetic(a.n, a.m)
    pos = np.cumsum(rng.exponential(1.5e-3, a.m))
    t0 = time.perf_counter()
    corr = ba.bed_cor(gb, size=3 / 1000, infos_pos=pos)
    rec["bed_cor_s"] = time.perf_counter() - t0
    m = corr.Dim[1]
    t0 = time.perf_counter()
    sf = ba.as_SFBM(corr)
    rec["as_SFBM_s"] = time.perf_counter() - t0
    rec["nnz_full"], rec["bandwidth"] = int(sf.nnz), int(sf.bandwidth)
    mc = clamp_max_cost(None, m, sf.sumsq_lower)
    rec["max_cost"] = mc
    args = (a.thr_r2, a.min_size, a.max_size)

    runs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        dev = ldsplit_one(sf, *args, a.max_K, a.max_r2, mc)
        wall = time.perf_counter() - t0
        runs.append(dict(wall_s=wall, E_s=float(dev["seconds"][0]), levels_s=float(dev["seconds"][1]),
                         epilogue_s=float(dev["seconds"][2])))
    got = np.nonzero(dev["ok"])[0] + 1
    rec["device"] = dict(runs=runs, levels_run=int(dev["levels_run"]),
                         n_block_reported=dict(count=int(got.size), first=int(got[0]) if got.size else None,
                                               last=int(got[-1]) if got.size else None),
                         wall_includes="the download of C and best_ind (12 m max_K bytes) into pageable memory")
    W = a.max_size - a.min_size + 1
    rec["device"]["candidates_per_level"] = int(sum(max(0, min(W, m - r - a.min_size + 1)) for r in range(m)))
    print(json.dumps(rec["device"]["runs"]), flush=True)
    _write(a.out, rec)      # the device part stands on its own if the CPU statement is cut short

    Kc = min(a.cpu_max_K, a.max_K)
    from scipy import sparse
    low = sparse.csc_matrix(corr.tocsc().T)       # the lower triangle: the transposed upper one
    low.sort_indices()
    t0 = time.perf_counter()
    cpu = ref.split(low.indptr.astype(np.int64), low.indices, low.data, m, *args, Kc, a.max_r2, mc, counters=False)
    wall = time.perf_counter() - t0
    lv = min(Kc, int(dev["levels_run"]), int(cpu["levels_run"]))
    equal = {key: bool(np.array_equal(dev[key][..., :lv], cpu[key][..., :lv])) for key in ("C", "best_ind")}
    for key in ("cost", "cost2", "perc_kept", "ok"):
        equal[key] = bool(np.array_equal(dev[key][:lv], cpu[key][:lv]))
    equal["all_last"] = bool(np.array_equal(dev["all_last"][:lv, :lv], cpu["all_last"][:lv, :lv]))
    rec["cpu"] = dict(threads=1, max_K=Kc, wall_covers="suffix sums, E, max_K levels, epilogue",
                      fewer_levels_than_device=bool(Kc < a.max_K), wall_s=wall, levels_run=int(cpu["levels_run"]), levels_compared=lv,
                      equal=equal, all_equal=all(equal.values()))
    print(json.dumps(rec["cpu"]), flush=True)
    _write(a.out, rec)


def _write(path, rec):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
