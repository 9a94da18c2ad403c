#!/usr/bin/env python3
"""big_spLinReg / big_spLogReg at config C2 -> profiles/plr_c2.json.

50 000 x 200 000 synthetic 2-bit image without missing values, 10 standard normal covariates, K = 10 folds, three alphas
(30 chains), a phenotype simulated from 50 variants and two covariates.  Each family is timed as one call with host
vectors (host clock around the synchronous call, uploads and downloads included) after a warm-up call on 2 000 columns;
bsn_plr_last_stats splits its device time into sweeps and scans (events around the launches of every turn) and counts
the turns and the coordinate updates.  A scan reads the selected columns once per turn (matrix bytes) and, in every
column's workgroup, the whole n x C panel of the live chains (panel bytes, counted here with all C chains: an upper
bound once chains have ended): 12 MB per column at C2, which no L2 holds, so the panel is what is expected to bound the
scan.  Both rates are reported; the 6.0 - 6.3 TB/s streaming rate of profiles/sfbm_c5.json is the yardstick for the
matrix bytes, not a rate this untuned kernel is expected to reach.  The CPU statement (tests/native/plr_ref.cpp, OpenMP
over the chains) runs on a subset of the columns; it is a different problem (fewer columns), so its time is reported as
measured, with the device's time on the same subset beside it, and the two results are compared.

    python tools/probe_plr.py [--n 50000] [--m 200000] [--cpu-cols 2000] [--threads 16] [--nlambda 200]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
import numpy as np  # noqa: E402

import bigsnpr_amd as ba  # noqa: E402
import plr_ref as ref  # noqa: E402

STREAM_TBS = (6.0, 6.3)   # profiles/sfbm_c5.json


def last_stats():
    out = (C.c_double * 6)()
    ba.load().bsn_plr_last_stats(out)
    return dict(zip(("sweep_ms", "scan_ms", "turns", "coordinate_updates", "start_ms", "device_ms"), map(float, out)))


def _write(path, rec):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def call(fit, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.perf_counter()
        mod = fit(*a, **kw)
        return mod, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--q", type=int, default=10)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--nlambda", type=int, default=200)
    ap.add_argument("--cpu-cols", type=int, default=2000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plr_c2.json"))
    a = ap.parse_args()
    n, m, q, K = a.n, a.m, a.q, a.K
    alphas = [1, 0.01, 0.0001]
    rng = np.random.default_rng(20261019)
    gb = ba.bed.synthetic(n, m, na16=0)
    cov = rng.standard_normal((n, q))
    causal = np.sort(rng.choice(min(m, a.cpu_cols), 50, replace=False))      # inside the CPU subset as well
    g = np.asarray(gb[:, causal], dtype=np.float64)
    g = (g - g.mean(axis=0)) / np.maximum(g.std(axis=0), 1e-12)
    eta = g @ rng.normal(0, 0.15, 50) + 0.4 * cov[:, 0] - 0.2 * cov[:, 1]
    ys = dict(linear=eta + rng.standard_normal(n), logistic=(rng.random(n) < 1 / (1 + np.exp(-eta))).astype(np.float64))
    sets = ba.plr.draw_sets(n, K, seed=1)
    pitch = (n + 3) // 4
    rec = dict(config="C2", n=n, m=m, covariates=q, K=K, alphas=alphas, nlambda=a.nlambda,
               image="2-bit synthetic, no missing values", streaming_rate_tbs=STREAM_TBS)
    fits = dict(linear=ba.big_spLinReg, logistic=ba.big_spLogReg)
    kw = dict(covar_train=cov, ind_sets=sets, alphas=alphas, nlambda=a.nlambda)
    sub = np.arange(min(m, a.cpu_cols))
    for fam, fit in fits.items():
        call(fit, gb, ys[fam], ind_col=sub, **kw)                            # warm-up: code objects, work buffers
        sub_mod, t_sub = call(fit, gb, ys[fam], ind_col=sub, **kw)
        st_sub = last_stats()
        mod, t_call = call(fit, gb, ys[fam], **kw)
        st = last_stats()
        scan_bytes = st["turns"] * m * pitch
        panel_bytes = st["turns"] * m * n * K * len(alphas) * 8.0
        rec[fam] = dict(call_s=t_call, **st,
                        share_in_sweeps=st["sweep_ms"] / st["device_ms"], share_in_scans=st["scan_ms"] / st["device_ms"],
                        scan_bytes=scan_bytes, scan_tbs=scan_bytes / (st["scan_ms"] * 1e-3) / 1e12,
                        scan_panel_bytes_upper=panel_bytes, scan_panel_tbs_upper=panel_bytes / (st["scan_ms"] * 1e-3) / 1e12,
                        us_per_coordinate_update=1e3 * st["sweep_ms"] / max(st["coordinate_updates"], 1.0),
                        messages=sorted({mo["message"] for mods in mod for mo in mods}),
                        lambdas_done=[int(mo["iter"].size) for mods in mod for mo in mods],
                        nb_var=[r["nb_var"] for r in mod.summary()],
                        subset=dict(columns=int(sub.size), call_s=t_sub, **st_sub),
                        note="scan_ms holds the scan, its flag pass and the commit of every turn; scan_bytes counts the "
                             "selected columns once per turn; scan_panel_bytes_upper counts the n x C panel once per column and "
                             "turn with all chains live (it exceeds L2: the expected bound of the scan)")
        print(json.dumps({fam: {k: rec[fam][k] for k in ("call_s", "sweep_ms", "scan_ms", "turns", "scan_tbs",
                                                           "us_per_coordinate_update")}}), flush=True)
        _write(a.out, rec)
        # the CPU statement on the subset
        X = np.asfortranarray(np.asarray(gb[:, sub], dtype=np.float64))
        t0 = time.perf_counter()
        f = ref.fit(X, ys[fam], sets, K, alphas=alphas, covar=cov, family=fam, nlambda=a.nlambda, nthreads=a.threads)
        t_cpu = time.perf_counter() - t0
        beta = np.column_stack([mo["beta"] for mods in sub_mod for mo in mods])
        rec[fam]["cpu_statement"] = dict(
            threads=a.threads, columns=int(sub.size), seconds=t_cpu, device_over_cpu=t_cpu / t_sub,
            status_equal=bool(np.array_equal(f["status"], [ref.MESSAGES.index(mo["message"]) for mods in sub_mod for mo in mods])),
            n_done_equal=bool(np.array_equal(f["n_done"], [mo["iter"].size for mods in sub_mod for mo in mods])),
            max_d_beta_over_max_beta=float(np.abs(beta - f["beta"]).max() / np.abs(f["beta"]).max()))
        print(json.dumps(rec[fam]["cpu_statement"]), flush=True)
        _write(a.out, rec)


if __name__ == "__main__":
    main()
