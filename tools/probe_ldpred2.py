#!/usr/bin/env python3
"""snp_ldpred2_grid at config C5 -> profiles/ldpred2_c5.json.

LD matrix and sumstats: those of tools/probe_lassosum2.py (bed_cor of the 400K x 100K synthetic .bed, size = 3/1000 on cM
positions; beta_hat = corr . beta + N(0, 1/N), 1 % causal variants, h2 = 0.5, N = 400 000).  The grid has the reference's
shape (test-8-LDpred2.R:51-56 at full size): 21 values of p from 1e-5 to 1, one h2, sparse off and on = 42 chains,
burn_in 50, num_iter 100.  The same call runs on the LDS-window path and, under BSN_GIBBS_NO_WINDOW=1, on the general
path; the CPU statement (tests/native/ldpred2_ref.cpp, OpenMP, 16 threads) runs the whole grid, is compared bit for bit
with the device and gives the committed moves of each chain.

    python tools/probe_ldpred2.py [--n 400000] [--m 100000] [--burn-in 50] [--num-iter 100] [--skip-general] [--skip-cpu]
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
import ldpred2_ref as ref  # noqa: E402


def _write(path, rec):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400000)
    ap.add_argument("--m", type=int, default=100000)
    ap.add_argument("--burn-in", type=int, default=50)
    ap.add_argument("--num-iter", type=int, default=100)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=20261017)
    ap.add_argument("--skip-general", action="store_true")
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldpred2_c5.json"))
    a = ap.parse_args()
    rec = dict(config="C5", n=a.n, m=a.m, size_cM=3.0, N=400000, causal=0.01, h2=0.5, burn_in=a.burn_in, num_iter=a.num_iter,
               seed=a.seed)
    rng = np.random.default_rng(20261016)
    gb = ba.bed.synthetic(a.n, a.m)
    pos = np.cumsum(rng.exponential(1.5e-3, a.m))
    corr = ba.bed_cor(gb, size=3 / 1000, infos_pos=pos)
    m2 = corr.Dim[1]
    from scipy import sparse
    U = corr.tocsc()
    N = 400000.0
    b = np.where(rng.random(m2) < 0.01, rng.normal(0, np.sqrt(0.5 / (0.01 * m2)), m2), 0.0)
    beta = U @ b + U.T @ b - U.diagonal() * b + rng.normal(0, np.sqrt(1 / N), m2)
    df = {"beta": beta, "beta_se": np.full(m2, 1 / np.sqrt(N)), "n_eff": np.full(m2, N)}
    pp = ba.seq_log(1e-5, 1, 21)
    gp = {"p": np.tile(pp, 2), "h2": np.full(42, 0.5), "sparse": np.repeat([False, True], 21)}
    rec["p"] = [float(v) for v in gp["p"]]
    rec["sparse"] = [bool(v) for v in gp["sparse"]]
    i_p1, i_p3 = 20, int(np.argmin(np.abs(pp - 1e-3)))      # the non-sparse chains with p = 1 and p = 1e-3

    sf = ba.as_SFBM(corr)
    rec["nnz_full"], rec["bandwidth"] = int(sf.nnz), int(sf.bandwidth)
    full = sparse.csc_matrix(U + sparse.triu(U, k=1).T)
    full.sort_indices()
    fp, fi, fx = full.indptr.astype(np.int64), full.indices, full.data
    fits, rows = ref.envelope(fp, fi, m2)
    rec["window"] = dict(taken=bool(fits), rows=int(rows), budget_rows=int(ref.window_rows()), lds_bytes=int(-(-rows // 64) * 64 * 8))
    kw = dict(burn_in=a.burn_in, num_iter=a.num_iter, seed=a.seed)

    def device(tag):
        t0 = time.perf_counter()
        res = ba.snp_ldpred2_grid(sf, df, gp, **kw)
        rec[tag] = dict(call_s=time.perf_counter() - t0, chain_s=[float(v) for v in res.grid_param["time"]],
                        nan_columns=[int(v) for v in np.nonzero(np.isnan(np.asarray(res)).all(axis=0))[0]])
        print(json.dumps({tag: {"call_s": rec[tag]["call_s"], "slowest_chain_s": max(rec[tag]["chain_s"])}}), flush=True)
        _write(a.out, rec)
        return res

    ba.snp_ldpred2_grid(sf, df, {k: v[:2] for k, v in gp.items()}, burn_in=1, num_iter=1, seed=1)      # code objects loaded
    win = device("window_path")
    if not a.skip_general:
        os.environ["BSN_GIBBS_NO_WINDOW"] = "1"
        gen = device("general_path")
        del os.environ["BSN_GIBBS_NO_WINDOW"]
        rec["paths_bits_equal"] = bool(np.array_equal(np.asarray(win), np.asarray(gen), equal_nan=True))
        rec["window_over_general"] = rec["general_path"]["call_s"] / rec["window_path"]["call_s"]
        _write(a.out, rec)

    if not a.skip_cpu:
        scale = np.sqrt(df["n_eff"] * df["beta_se"] ** 2 + df["beta"] ** 2)
        t0 = time.perf_counter()
        cb, moves, csecs = ref.grid(fp, fi, fx, m2, df["beta"] / scale, df["n_eff"], gp["h2"], gp["p"], gp["sparse"],
                                    nthreads=a.threads, **kw)
        rec["cpu"] = dict(threads=a.threads, wall_s=time.perf_counter() - t0, chain_s=[float(v) for v in csecs],
                          committed_moves=[int(v) for v in moves],
                          bits_equal_device=bool(np.array_equal(cb * scale[:, None], np.asarray(win), equal_nan=True)))
        for tag in ("window_path", "general_path"):
            if tag in rec:
                rec[tag]["us_per_move_p1"] = 1e6 * rec[tag]["chain_s"][i_p1] / max(int(moves[i_p1]), 1)
                rec[tag]["us_per_move_p1e-3"] = 1e6 * rec[tag]["chain_s"][i_p3] / max(int(moves[i_p3]), 1)
        rec["cpu"]["us_per_move_p1"] = 1e6 * float(csecs[i_p1]) / max(int(moves[i_p1]), 1)
        rec["cpu"]["us_per_move_p1e-3"] = 1e6 * float(csecs[i_p3]) / max(int(moves[i_p3]), 1)
        rec["device_over_cpu"] = rec["window_path"]["call_s"] / rec["cpu"]["wall_s"]
        print(json.dumps({"cpu": {k: rec["cpu"][k] for k in ("wall_s", "bits_equal_device", "us_per_move_p1")}}), flush=True)
        _write(a.out, rec)
    sf.close()


if __name__ == "__main__":
    main()
