#!/usr/bin/env python3
"""big_univLinReg and big_univLogReg at config C2 -> profiles/gwas_c2.json.

50 000 x 200 000 synthetic 2-bit image without missing values, 10 standard normal covariates, a binary phenotype
simulated from 20 variants and the first two covariates.  Both scans are timed as calls with host vectors (host clock
around the synchronous call: uploads, the null model and the downloads included), after a warm-up call, with the spread
of the repeats.  The CPU statement (tests/native/gwas_ref.cpp, OpenMP) runs on a subset of the columns and is scaled to
m; the device's results on those columns are compared with it.

    python tools/probe_gwas.py [--n 50000] [--m 200000] [--cpu-cols 512] [--threads 16] [--repeats 3]
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
import gwas_ref as ref  # noqa: E402

# MI355X at 2.4 GHz, 256 CUs x 4 SIMDs: the f64 MFMA and the f64 vector pipe both peak at 78.6 TFLOP/s (AMD's
# published figures; half the f32 vector rate)
PEAK_F64 = 78.6e12
MAXITER = 20


def timed(f, repeats):
    f()                                       # warm-up: code objects, work buffers
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return out, dict(median_s=float(np.median(ts)), min_s=float(min(ts)), max_s=float(max(ts)), repeats=repeats)


def _write(path, rec):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--q", type=int, default=10)
    ap.add_argument("--cpu-cols", type=int, default=512)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gwas_c2.json"))
    a = ap.parse_args()
    n, m, q = a.n, a.m, a.q
    rng = np.random.default_rng(20261018)
    gb = ba.bed.synthetic(n, m, na16=0)
    cov = rng.standard_normal((n, q))
    causal = np.sort(rng.choice(m, 20, replace=False))
    g = np.asarray(gb[:, causal], dtype=np.float64)
    g = (g - g.mean(axis=0)) / np.maximum(g.std(axis=0), 1e-12)
    eta = -0.3 + g @ rng.normal(0, 0.15, 20) + 0.4 * cov[:, 0] - 0.2 * cov[:, 1]
    y01 = (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(np.float64)
    ylin = eta + rng.standard_normal(n)
    rec = dict(config="C2", n=n, m=m, covariates=q, image="2-bit synthetic, no missing values", cases=int(y01.sum()),
               tol=1e-8, maxiter=MAXITER)

    log, rec["logistic_call"] = timed(lambda: ba.big_univLogReg(gb, y01, covar_train=cov, tol=1e-8, maxiter=MAXITER, verbose=False), a.repeats)
    it = log["niter"]
    vals, cnt = np.unique(it, return_counts=True)
    rec["niter_histogram"] = {str(int(v)): int(c) for v, c in zip(vals, cnt)}
    solves = int(np.where(it > 0, it, np.where(it < 0, MAXITER, 1)).sum())
    t_vi = rec["logistic_call"]["median_s"] / solves
    P = q + 2
    mfma_flop = 2048.0 * -(-n // 4)           # one 16x16x4 f64 MFMA per four samples (P + 1 <= 16)
    useful_flop = 2.0 * n * (P * (P + 1) / 2 + P)
    rec["logistic"] = dict(
        variant_iterations=solves, s_per_variant_iteration=t_vi, variants_per_s=m / rec["logistic_call"]["median_s"],
        mfma_flop_per_variant_iteration=mfma_flop, useful_flop_per_variant_iteration=useful_flop,
        mfma_rate_tflops=mfma_flop / t_vi / 1e12, share_of_f64_mfma_peak=mfma_flop / t_vi / PEAK_F64,
        note="whole-call rates (host clock), not kernel time; peak: 78.6 TFLOP/s on the f64 matrix pipe; the vector "
             "instructions of a step (eta, exp, the operand scaling) have not been counted from the ISA")
    print(json.dumps({"logistic": rec["logistic_call"], "niter": rec["niter_histogram"]}), flush=True)
    _write(a.out, rec)

    lin, rec["linear_call"] = timed(lambda: ba.big_univLinReg(gb, ylin, covar_train=cov), max(a.repeats, 5))
    yv = rng.standard_normal(n)
    _, rec["bed_cprodVec_call"] = timed(lambda: ba.bed_cprodVec(gb, yv), max(a.repeats, 5))
    rec["linear"] = dict(panel_vectors=q + 2, variants_per_s=m / rec["linear_call"]["median_s"],
                         ratio_to_one_cprodVec_call=rec["linear_call"]["median_s"] / rec["bed_cprodVec_call"]["median_s"],
                         note="the panel [y~, U] is q + 2 vectors at 7 slices: 4 vectors per launch of the streaming kernel")
    print(json.dumps({"linear": rec["linear_call"], "cprodVec": rec["bed_cprodVec_call"]}), flush=True)
    _write(a.out, rec)

    # the CPU statement on a subset of the columns, scaled to m
    cols = np.sort(rng.choice(m, a.cpu_cols, replace=False))
    X = np.asfortranarray(np.asarray(gb[:, cols], dtype=np.float64))
    t0 = time.perf_counter()
    cl = ref.logreg(X, y01, cov, tol=1e-8, maxiter=MAXITER, nthreads=a.threads)
    t_log = time.perf_counter() - t0
    t0 = time.perf_counter()
    cn = ref.linreg(X, ylin, cov, nthreads=a.threads)
    t_lin = time.perf_counter() - t0
    ok = cl["niter"] > 0
    rec["cpu_statement"] = dict(
        threads=a.threads, subset_columns=int(a.cpu_cols), logistic_subset_s=t_log, linear_subset_s=t_lin,
        logistic_scaled_s=t_log * m / a.cpu_cols, linear_scaled_s=t_lin * m / a.cpu_cols,
        niter_equal=bool(np.array_equal(cl["niter"], it[cols])),
        max_d_estim_over_se=float(np.max(np.abs(cl["estim"][ok] - log["estim"][cols][ok]) / cl["std_err"][ok])),
        max_rel_d_se=float(np.max(np.abs(log["std_err"][cols][ok] / cl["std_err"][ok] - 1))),
        linear_max_rel_d_estim=float(np.nanmax(np.abs(lin["estim"][cols] / cn["estim"] - 1))),
        linear_max_rel_d_se=float(np.nanmax(np.abs(lin["std_err"][cols] / cn["std_err"] - 1))))
    rec["device_over_cpu"] = dict(logistic=rec["cpu_statement"]["logistic_scaled_s"] / rec["logistic_call"]["median_s"],
                                  linear=rec["cpu_statement"]["linear_scaled_s"] / rec["linear_call"]["median_s"])
    _write(a.out, rec)
    print(json.dumps(rec["cpu_statement"]), flush=True)
    print(json.dumps(rec["device_over_cpu"]), flush=True)


if __name__ == "__main__":
    main()
