#!/usr/bin/env python3
"""snp_lassosum2 at config C5 -> profiles/lassosum2_c5.json.

LD matrix: bed_cor of the C5 image (400K x 100K synthetic .bed), size = 3/1000 on cM positions with Exp(mean 1.5e-3 cM)
gaps.  Sumstats: beta_hat = corr . beta + N(0, 1/N), 1 % causal variants, N = 400 000 (beta_se = 1/sqrt(N),
n_eff = N).  The default grid (30 lambdas x 4 deltas = 120 points, maxiter 1000) runs on the device; the CPU statement
(tests/native/lassosum2_ref.c, OpenMP, 16 threads) runs a sample of the grid points, which are also checked bit for bit
against the device, and its 16-thread time for the whole grid is extrapolated from the sample.

    python tools/probe_lassosum2.py [--n 400000] [--m 100000] [--cpu-points 16] [--out profiles/lassosum2_c5.json]
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
import lassosum2_ref as ref  # noqa: E402
from bigsnpr_amd.lassosum2 import lassosum2_inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400000)
    ap.add_argument("--m", type=int, default=100000)
    ap.add_argument("--cpu-points", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lassosum2_c5.json"))
    a = ap.parse_args()
    rec = dict(config="C5", n=a.n, m=a.m, size_cM=3.0, N=400000, causal=0.01)
    rng = np.random.default_rng(20261016)
    gb = ba.bed.synthetic(a.n, a.m)
    pos = np.cumsum(rng.exponential(1.5e-3, a.m))
    t0 = time.perf_counter()
    corr = ba.bed_cor(gb, size=3 / 1000, infos_pos=pos)
    rec["bed_cor_s"] = time.perf_counter() - t0
    m2 = corr.Dim[1]
    rec["nnz_upper"] = int(corr.p[-1])
    from scipy import sparse
    U = corr.tocsc()
    N = 400000.0
    b = np.where(rng.random(m2) < 0.01, rng.normal(0, np.sqrt(0.5 / (0.01 * m2)), m2), 0.0)
    d = U.diagonal()
    beta = U @ b + U.T @ b - d * b + rng.normal(0, np.sqrt(1 / N), m2)
    df = {"beta": beta, "beta_se": np.full(m2, 1 / np.sqrt(N)), "n_eff": np.full(m2, N)}

    t0 = time.perf_counter()
    sf = ba.as_SFBM(corr)
    rec["as_SFBM_s"] = time.perf_counter() - t0
    rec["nnz_full"], rec["bandwidth"] = int(sf.nnz), int(sf.bandwidth)
    runs = []
    for _ in range(1):
        t0 = time.perf_counter()
        res = ba.snp_lassosum2(sf, df)
        runs.append(time.perf_counter() - t0)
    gp = res.grid_param
    rec["gpu_grid_s"] = runs
    rec["gpu_grid_points"] = int(res.shape[1])
    rec["gpu_point_device_s"] = [float(v) for v in gp["time"]]
    rec["num_iter"] = [int(v) for v in gp["num_iter"]]
    rec["sparsity"] = [None if np.isnan(v) else float(v) for v in gp["sparsity"]]
    rec["lambda"] = [float(v) for v in gp["lambda"]]
    rec["delta"] = [float(v) for v in gp["delta"]]
    print(json.dumps({k: rec[k] for k in ("bed_cor_s", "as_SFBM_s", "nnz_full", "bandwidth", "gpu_grid_s")}), flush=True)
    _write(a.out, rec)      # the device part stands on its own if the CPU sample is cut short

    # CPU statement: a sample of grid points, 16 threads, checked against the device
    G = res.shape[1]
    # evenly spaced over the grid, plus the grid point that took the device longest
    pick = np.unique(np.append(np.linspace(0, G - 1, min(a.cpu_points, G)).round().astype(int), np.argmax(gp["time"])))
    full = sparse.csc_matrix(U + sparse.triu(U, k=1).T)
    full.sort_indices()
    scale, bh, pf, lam, dl = lassosum2_inputs(df["beta"], df["beta_se"], df["n_eff"], (0.001, 0.01, 0.1, 1), 30, 0.01)
    t0 = time.perf_counter()
    cb, citer, cmoves, csecs = ref.grid(full.indptr.astype(np.int64), full.indices, full.data, m2, bh, pf, lam[pick],
                                        dl[pick], maxiter=1000, nthreads=a.threads)
    wall = time.perf_counter() - t0
    same = bool(np.array_equal(cb * scale[:, None], np.asarray(res)[:, pick], equal_nan=True)
                and np.array_equal(citer, gp["num_iter"][pick]))
    rec["cpu"] = dict(threads=a.threads, points=[int(v) for v in pick], wall_s=wall, point_s=[float(v) for v in csecs],
                      num_iter=[int(v) for v in citer], nonzero_shift_steps=[int(v) for v in cmoves],
                      bits_equal_device=same,
                      whole_grid_16_threads_est_s=float(max(np.max(csecs), np.sum(csecs) * G / pick.size / a.threads)),
                      estimate="max(slowest sampled point, sum of the sampled points' single-thread seconds x (G / sample) / "
                               "threads): perfect load balance over the threads, a lower bound on the full run's wall time")
    rec["speedup_est"] = rec["cpu"]["whole_grid_16_threads_est_s"] / min(runs)
    print(json.dumps({k: rec[k] for k in ("cpu", "speedup_est")}), flush=True)
    _write(a.out, rec)


def _write(path, rec):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
