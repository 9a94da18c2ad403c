#!/usr/bin/env python3
"""The OADP projection on the device against pca_OADP_proj2 on the host -> profiles/project_pca.json.

For K = 10 and K = 20, n = 400 000 target samples with synthetic simple projections (normal, scaled by the singular
values; squared norms 1.05 to 4 times |l|^2):

* the OADP launch: device time between two events around the kernel (bsn_project_last_ms), median of the repeats;
* bsn_pca_oadp_proj as a call: host clock around the synchronous call (upload, launch, download), after a warm-up call;
* pca_OADP_proj2 (NumPy: one eigh and one svd per sample) on the first 20 000 samples in the same process, SCALED to n
  (marked as scaled: the function is linear in n), and the largest deviation of the device result from it on that slice;
* the fused call bsn_bed_project_pca on the C2 image (50 000 x 200 000 synthetic 2-bit image, 1 % missing, all rows, the
  variants with a positive scale, a random orthonormal V): host clock, and the device time of its product passes and of
  its OADP launch.

    python tools/probe_project.py [--n 400000] [--slice 20000] [--repeats 3] [--no-fused] [--out profiles/project_pca.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bigsnpr_amd as ba  # noqa: E402
from bigsnpr_amd.prs import project_last_ms  # noqa: E402

SEED = 20261019
KS = (10, 20)


def timed(f, repeats, dev=None):
    f()                                       # warm-up: code objects, work buffers
    ts, ds = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
        if dev:
            ds.append(dev())
    r = dict(median_s=float(np.median(ts)), min_s=float(min(ts)), max_s=float(max(ts)), repeats=repeats)
    if dev:
        r["device_ms_median"] = [float(x) for x in np.median(np.array(ds), axis=0)]
    return r


def _write(path, rec):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400000)
    ap.add_argument("--slice", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-fused", action="store_true")
    ap.add_argument("--c2-n", type=int, default=50000)
    ap.add_argument("--c2-m", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "project_pca.json"))
    a = ap.parse_args()
    n, ns = a.n, min(a.slice, a.n)
    rng = np.random.default_rng(SEED)
    rec = dict(n=n, host_slice=ns, seed=SEED,
               note="oadp_launch_ms: HIP events around the kernel; call: host clock around bsn_pca_oadp_proj; host_scaled_s: "
                    "pca_OADP_proj2 on host_slice samples times n / host_slice (SCALED, not measured at n)")
    for K in KS:
        d = np.sort(rng.uniform(20, 400, K))[::-1].copy()
        XV = np.asfortranarray(rng.normal(size=(n, K)) * d / np.sqrt(300.0))
        X_norm = (XV ** 2).sum(axis=1) * rng.uniform(1.05, 4.0, n)
        call = timed(lambda: ba.pca_OADP_proj_device(XV, X_norm, d), a.repeats, project_last_ms)
        dev = ba.pca_OADP_proj_device(XV[:ns], X_norm[:ns], d)
        t0 = time.perf_counter()
        host = ba.pca_OADP_proj2(XV[:ns], X_norm[:ns], d)
        host_s = time.perf_counter() - t0
        r = dict(call=call, oadp_launch_ms=call["device_ms_median"][1],
                 host_slice_s=host_s, host_us_per_sample=host_s / ns * 1e6, host_scaled_s=host_s * n / ns, host_is_scaled=True,
                 max_abs_diff_over_d1=float(np.abs(dev - host).max() / d[0]))
        r["ratio_host_scaled_over_call"] = r["host_scaled_s"] / call["median_s"]
        r["ratio_host_scaled_over_launch"] = r["host_scaled_s"] / (r["oadp_launch_ms"] * 1e-3)
        rec["K=%d" % K] = r
        print(json.dumps({"K": K, **r}), flush=True)
        _write(a.out, rec)

    if not a.no_fused:
        gb = ba.bed.synthetic(a.c2_n, a.c2_m, na16=655)
        sc = ba.bed_scaleBinom(gb)
        ic = np.nonzero(sc["scale"] > 0)[0]
        rec["fused_C2"] = dict(config="C2", n=a.c2_n, m=a.c2_m, columns=int(ic.size),
                               image="2-bit synthetic, 1 % missing (na16 = 655)",
                               note="device_ms_median = [product and row-norm passes, OADP launch]")
        for K in KS:
            V = np.linalg.qr(rng.normal(size=(ic.size, K)))[0]
            d = np.sqrt(a.c2_n) * np.linspace(3.0, 1.0, K)
            center, scale = sc["center"][ic], sc["scale"][ic]
            fused = timed(lambda: ba.project_pca(gb, None, ic, center, scale, V, d), a.repeats, project_last_ms)
            parts = timed(lambda: ba.prod_and_rowSumsSq(gb, None, ic, center, scale, V), a.repeats)
            rec["fused_C2"]["K=%d" % K] = dict(fused=fused, prod_and_rowSumsSq_alone=parts)
            print(json.dumps({"fused_C2_K": K, **rec["fused_C2"]["K=%d" % K]}), flush=True)
            _write(a.out, rec)
        gb.close()


if __name__ == "__main__":
    main()
