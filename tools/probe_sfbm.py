#!/usr/bin/env python3
"""sp_prodVec, ld_scores_sfbm and snp_ldpred2_inf at config C5 -> profiles/sfbm_c5.json.

LD matrix and summary statistics as tools/probe_lassosum2.py: bed_cor of the C5 image (400K x 100K synthetic .bed),
size = 3/1000 on cM positions with Exp(mean 1.5e-3 cM) gaps; beta_hat = corr . beta + N(0, 1/N), 1 % causal variants,
N = 400 000.  Times are host clocks around calls that end in a device synchronisation (with the host copies) and HIP events
inside the library (without: SFBM.last_ms).  Bytes moved by one product: 12 per stored entry (x and i), 8 per column
offset, 4 per entry of the column list, and the vectors (the gathered v read once, y written once: 16 per column).  The
roofline beside it is the streaming read rate measured on this device, 6.0 - 6.3 TB/s, not the 8 TB/s of the data sheet.

The comparator is tests/native/sfbm_ref.c: the same product with OpenMP over the columns on --threads CPU threads, and
scipy.sparse.linalg.minres running on that product (scipy stops on its own estimate ||r|| / (||A|| ||x||); the true
residual it reached is recorded).

    python tools/probe_sfbm.py [--n 400000] [--m 100000] [--threads 16] [--out profiles/sfbm_c5.json]
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
import sfbm_ref  # noqa: E402

STREAM_TBS = [6.0, 6.3]


def timed(f, reps, after=None):
    """wall seconds of each of `reps` calls (after one untimed warm-up), the last result, and after() of each call"""
    out = f()
    secs, extra = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        secs.append(time.perf_counter() - t0)
        if after:
            extra.append(after())
    return secs, out, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400000)
    ap.add_argument("--m", type=int, default=100000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--h2", type=float, default=0.3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sfbm_c5.json"))
    a = ap.parse_args()
    rec = dict(config="C5", n=a.n, m=a.m, size_cM=3.0, N=400000, causal=0.01, h2=a.h2, streaming_read_TBs=STREAM_TBS)
    rng = np.random.default_rng(20261016)
    gb = ba.bed.synthetic(a.n, a.m)
    pos = np.cumsum(rng.exponential(1.5e-3, a.m))
    t0 = time.perf_counter()
    corr = ba.bed_cor(gb, size=3 / 1000, infos_pos=pos)
    rec["bed_cor_s"] = time.perf_counter() - t0
    m2 = corr.Dim[1]
    t0 = time.perf_counter()
    sf = ba.as_SFBM(corr)
    rec["as_SFBM_s"] = time.perf_counter() - t0
    rec["nnz_full"], rec["bandwidth"] = int(sf.nnz), int(sf.bandwidth)
    N = 400000.0
    b = np.where(rng.random(m2) < 0.01, rng.normal(0, np.sqrt(0.5 / (0.01 * m2)), m2), 0.0)
    beta = ba.sp_prodVec(sf, b) + rng.normal(0, np.sqrt(1 / N), m2)
    df = {"beta": beta, "beta_se": np.full(m2, 1 / np.sqrt(N)), "n_eff": np.full(m2, N)}
    x = rng.normal(size=m2)

    # the product
    secs, y, dev = timed(lambda: ba.sp_prodVec(sf, x), a.reps, sf.last_ms)
    nbytes = 12 * sf.nnz + 8 * (m2 + 1) + 4 * m2 + 16 * m2
    rec["prodvec"] = dict(wall_ms=[1e3 * s for s in secs], device_ms=dev, bytes=int(nbytes),
                          TBs_device=nbytes / (min(dev) * 1e-3) / 1e12, TBs_device_median=nbytes / (np.median(dev) * 1e-3) / 1e12,
                          share_of_streaming_rate=[nbytes / (np.median(dev) * 1e-3) / 1e12 / r for r in STREAM_TBS[::-1]])
    # the same product on half of the columns (unsorted subset)
    sub = rng.permutation(m2)[:m2 // 2]
    secs, _, dev = timed(lambda: ba.sp_prodVec(sf, x[:sub.size], ind_corr=sub), 3, sf.last_ms)
    rec["prodvec_half_subset"] = dict(wall_ms=[1e3 * s for s in secs], device_ms=dev)
    # LD scores
    secs, ld, dev = timed(lambda: ba.ld_scores_sfbm(sf), a.reps, sf.last_ms)
    nb_ld = 12 * sf.nnz + 8 * (m2 + 1) + 4 * m2 + 8 * m2
    rec["ld_scores"] = dict(wall_ms=[1e3 * s for s in secs], device_ms=dev, bytes=int(nb_ld),
                            TBs_device_median=nb_ld / (np.median(dev) * 1e-3) / 1e12)
    # LDSC on those scores, then LDpred2-inf
    t0 = time.perf_counter()
    rec["snp_ldsc2"] = ba.snp_ldsc2(sf, df, blocks=200, intercept=None)
    rec["snp_ldsc2_s"] = time.perf_counter() - t0
    secs, beta_inf, _ = timed(lambda: ba.snp_ldpred2_inf(sf, df, a.h2), 3)
    scale = np.sqrt(N * df["beta_se"] ** 2 + df["beta"] ** 2)
    bh, d = df["beta"] / scale, m2 / (a.h2 * df["n_eff"])
    sol = ba.sp_solve_sym(sf, bh, add_to_diag=d)
    assert np.array_equal(np.asarray(sol) * scale, beta_inf)
    solve_ms = sf.last_ms()
    rec["snp_ldpred2_inf"] = dict(wall_s=secs, iterations=sol.iters, relres=sol.relres, tol=1e-10, solve_device_ms=solve_ms,
                                  device_ms_per_iteration=solve_ms / max(sol.iters, 1), add_to_diag=float(d[0]))
    print(json.dumps({k: rec[k] for k in ("bed_cor_s", "as_SFBM_s", "nnz_full", "prodvec", "ld_scores", "snp_ldpred2_inf")}),
          flush=True)
    _write(a.out, rec)      # the device part stands on its own if the CPU part is cut short
    if a.no_cpu:
        return

    # the comparator: OpenMP product over full columns, scipy's MINRES on it
    from scipy import sparse
    U = corr.tocsc()
    full = sparse.csc_matrix(U + sparse.triu(U, k=1).T)
    full.sort_indices()
    del U
    M = sfbm_ref.Matrix(full.indptr, full.indices, full.data, nthreads=a.threads)
    secs, y_cpu, _ = timed(lambda: M.prodvec(x), 5)
    mag = np.abs(y_cpu).max()
    cpu = dict(threads=a.threads, what="tests/native/sfbm_ref.c (OpenMP over columns) + scipy.sparse.linalg.minres",
               prodvec_ms=[1e3 * s for s in secs], prodvec_max_abs_diff_over_max=float(np.abs(y - y_cpu).max() / mag))
    secs, ld_cpu, _ = timed(M.colsumsq, 3)
    cpu["ld_scores_ms"] = [1e3 * s for s in secs]
    cpu["ld_scores_max_rel_diff"] = float(np.max(np.abs(ld - ld_cpu) / ld_cpu))
    t0 = time.perf_counter()
    x_cpu, products, relres = M.solve_sym(bh, d, tol=1e-10)
    cpu["solve_s"] = time.perf_counter() - t0
    cpu["solve_products"], cpu["solve_relres"] = products, relres
    cpu["solve_rel_diff_to_device"] = float(np.linalg.norm(np.asarray(sol) - x_cpu) / np.linalg.norm(x_cpu))
    rec["cpu"] = cpu
    rec["ratio_cpu_over_device"] = dict(prodvec_with_copies=min(cpu["prodvec_ms"]) / min(rec["prodvec"]["wall_ms"]),
                                        prodvec_device=min(cpu["prodvec_ms"]) / min(rec["prodvec"]["device_ms"]),
                                        ldpred2_inf=cpu["solve_s"] / min(rec["snp_ldpred2_inf"]["wall_s"]))
    print(json.dumps({k: rec[k] for k in ("cpu", "ratio_cpu_over_device")}), flush=True)
    _write(a.out, rec)


def _write(path, rec):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
