#!/usr/bin/env python3
"""snp_ldpred2_auto at config C5 -> profiles/ldpred2_auto_c5.json.

LD matrix and sumstats: those of tools/probe_ldpred2.py (bed_cor of the 400K x 100K synthetic .bed, size = 3/1000 on cM
positions; beta_hat = corr . beta + N(0, 1/N), 1 % causal variants, h2 = 0.5, N = 400 000).  The call has the usual shape:
vec_p_init = seq_log(1e-4, 0.2, 30), burn_in 500, num_iter 200, h2_init 0.3, everything else at its default.  It runs on
the LDS-window path and, under BSN_GIBBS_NO_WINDOW=1, on the general path; the CPU statement
(tests/native/ldpred2_auto_ref.cpp, OpenMP, 16 threads) runs the same chains, is compared bit for bit with the device and
gives the committed moves of each chain.

    python tools/probe_ldpred2_auto.py [--n 400000] [--m 100000] [--burn-in 500] [--num-iter 200] [--chains 30]
                                       [--skip-general] [--skip-cpu]
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
import ldpred2_auto_ref as ref  # noqa: E402

KEYS = ("beta_est", "postp_est", "corr_est", "sample_beta", "path_p_est", "path_h2_est", "path_alpha_est")


def _write(path, rec):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def _equal(a, b):
    return bool(all(np.array_equal(x[k], y[k], equal_nan=True) for x, y in zip(a, b) for k in KEYS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400000)
    ap.add_argument("--m", type=int, default=100000)
    ap.add_argument("--burn-in", type=int, default=500)
    ap.add_argument("--num-iter", type=int, default=200)
    ap.add_argument("--chains", type=int, default=30)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=20261017)
    ap.add_argument("--skip-general", action="store_true")
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldpred2_auto_c5.json"))
    a = ap.parse_args()
    rec = dict(config="C5", n=a.n, m=a.m, size_cM=3.0, N=400000, causal=0.01, h2=0.5, h2_init=0.3, burn_in=a.burn_in,
               num_iter=a.num_iter, seed=a.seed)
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
    pv = ba.seq_log(1e-4, 0.2, a.chains)
    rec["p_init"] = [float(v) for v in pv]

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
        res = ba.snp_ldpred2_auto(sf, df, 0.3, vec_p_init=pv, **kw)
        rec[tag] = dict(call_s=time.perf_counter() - t0, chain_s=[r["time"] for r in res],
                        h2_est=[r["h2_est"] for r in res], p_est=[r["p_est"] for r in res],
                        alpha_est=[r["alpha_est"] for r in res])
        rec[tag]["s_per_chain"] = rec[tag]["call_s"] / len(res)
        print(json.dumps({tag: {"call_s": rec[tag]["call_s"], "slowest_chain_s": max(rec[tag]["chain_s"])}}), flush=True)
        _write(a.out, rec)
        return res

    ba.snp_ldpred2_auto(sf, df, 0.3, vec_p_init=pv[:2], burn_in=1, num_iter=1, seed=1)      # code objects loaded
    win = device("window_path")
    if not a.skip_general:
        os.environ["BSN_GIBBS_NO_WINDOW"] = "1"
        gen = device("general_path")
        del os.environ["BSN_GIBBS_NO_WINDOW"]
        rec["paths_bits_equal"] = _equal(win, gen)
        rec["window_over_general"] = rec["general_path"]["call_s"] / rec["window_path"]["call_s"]
        _write(a.out, rec)

    if not a.skip_cpu:
        sd = 1 / np.sqrt(df["n_eff"] * df["beta_se"] ** 2 + df["beta"] ** 2)
        mean_ld = float(np.mean(ba.ld_scores_sfbm(sf)))
        t0 = time.perf_counter()
        raw = ref.auto(fp, fi, fx, m2, df["beta"] * sd, df["n_eff"], 2 * np.log(sd), pv, 0.3, mean_ld, nthreads=a.threads, **kw)
        wall = time.perf_counter() - t0
        cpu = [{"beta_est": raw["beta_est"][:, g] / sd, "postp_est": raw["postp_est"][:, g], "corr_est": raw["corr_est"][:, g],
                "sample_beta": raw["sample_beta"][:, :, g], "path_p_est": raw["path_p"][:, g], "path_h2_est": raw["path_h2"][:, g],
                "path_alpha_est": raw["path_alpha"][:, g]} for g in range(pv.size)]
        moves = raw["moves"]
        rec["cpu"] = dict(threads=a.threads, wall_s=wall, s_per_chain=wall / pv.size, chain_s=[float(v) for v in raw["secs"]],
                          committed_moves=[int(v) for v in moves], bits_equal_device=_equal(cpu, win),
                          us_per_move=1e6 * float(np.sum(raw["secs"])) / max(int(np.sum(moves)), 1))
        for tag in ("window_path", "general_path"):
            if tag in rec:
                rec[tag]["us_per_move"] = 1e6 * float(np.sum(rec[tag]["chain_s"])) / max(int(np.sum(moves)), 1)
        rec["device_over_cpu"] = rec["window_path"]["call_s"] / wall
        print(json.dumps({"cpu": {k: rec["cpu"][k] for k in ("wall_s", "bits_equal_device", "us_per_move")}}), flush=True)
        _write(a.out, rec)
    sf.close()


if __name__ == "__main__":
    main()
