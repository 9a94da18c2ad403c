"""AUC / snp_grid_AUC / AUCBoot / big_prodMat at the shapes of the SCT vignette -> profiles/auc_c3.json.

What it records (device milliseconds are HIP events inside the library, bsn_auc_last_ms):

* AUC and snp_grid_AUC on 300 000 rows x 1 400 columns of synthetic scores, resident in fp64: the split into key pass,
  sort, and group + evaluation kernels, with the bytes each moves at least once over its time, beside the 6.0 - 6.3 TB/s
  streaming rate of profiles/sfbm_c5.json; the call on the float32 host matrix (upload included) as wall clock; the same
  call with the column batch forced (BSN_AUC_BATCH), results asserted equal — for the record, no decision is taken.
* AUCBoot, nboot 10 000, one column and eight columns, at n = 10 000, 100 000 and 1 000 000: draws per second of the
  bootstrap kernel (draws, atomics and evaluation are one kernel: there is no split to record) and the time of the sort
  path before it.  Where nboot x columns x n would take more than --boot-budget seconds at the rate just measured, nboot
  is cut and the record says so.
* the CPU statement (tests/native/auc_ref.cpp, OpenMP) on a subset: 64 columns of the AUC shape, 256 replicates of the
  n = 1 000 000 bootstrap, SCALED by count to the full shapes and labelled as scaled, not run.
* big_prodMat with K = 168 at C2 (50 000 x 200 000, synthetic image) against prod_and_rowSumsSq alone, same process.

No time here is a target.

    python tools/probe_auc.py [--n 300000] [--K 1400] [--nboot 10000] [--skip auc boot cpu prodmat] [--out profiles/auc_c3.json]
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

STREAM_LOW, STREAM_HIGH = 6.0e12, 6.3e12


def _write(path, rec):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def timed(f):
    t0 = time.perf_counter()
    res = f()
    return res, time.perf_counter() - t0


def split(ms, n, K, nsum):
    """the three parts of the sort path with the bytes each moves at least once"""
    cells = float(n) * K
    b = dict(key_pass=cells * (8.0 * nsum + 12.0),               # members in, key and row out
             sort=cells * 24.0,                                  # keys and rows in and out once: a lower bound, a radix sort makes several passes
             group_scan=cells * (12.0 + 1.0 + 4.0 + 4.0))   # key, row, class in; code out; one atomic
    out = {}
    for k, t in zip(("key_pass", "sort", "group_scan"), ms[:3]):
        out[k] = dict(ms=float(t), bytes_at_least=b[k], TBps=b[k] / (t * 1e-3) / 1e12 if t > 0 else None,
                      share_of_streaming_6p0_TBps=b[k] / (t * 1e-3) / STREAM_LOW if t > 0 else None)
    return out


def auc_part(a, rec):
    n, K = a.n, a.K
    rng = np.random.default_rng(1)
    X32, gen = timed(lambda: rng.standard_normal((K, n), dtype=np.float32).T)
    y = (rng.uniform(size=n) < 0.3).astype(np.uint8)
    y[:2] = 0, 1
    ba.AUC(X32[:4096, :8], y[:4096])                                          # first use of the library and of its buffers
    d = ba.DeviceArray.from_numpy(X32)
    ba.AUC(d, y)
    runs = []
    for _ in range(a.repeats):
        res, wall = timed(lambda: ba.AUC(d, y))
        runs.append(dict(wall_s=wall, **split(ba.auc_last_ms(), n, K, 1)))
    # the column batch forced, for the record (no decision is taken from it): one batch allocates its whole workspace at once
    sweep = []
    for cap in a.batches:
        if cap:
            os.environ["BSN_AUC_BATCH"] = str(cap)
        else:
            os.environ.pop("BSN_AUC_BATCH", None)
        ba.AUC(d, y)
        got, wall = timed(lambda: ba.AUC(d, y))
        assert np.array_equal(got, res)
        ms = ba.auc_last_ms()
        sweep.append(dict(BSN_AUC_BATCH=cap or None, batches=-(-K // cap) if cap else 1, wall_s=wall, key_pass_ms=float(ms[0]),
                          sort_ms=float(ms[1]), group_scan_ms=float(ms[2]), workspace_GB=48.0 * n * (cap or K) / 1e9))
    os.environ.pop("BSN_AUC_BATCH", None)
    host, wall_host = timed(lambda: ba.AUC(X32, y))
    assert np.array_equal(host, res)
    rec["auc"] = dict(n=n, K=K, generated_s=gen, resident_fp64_runs=runs, batch_sweep=sweep, host_float32_call_wall_s=wall_host,
                      best=float(res.max()), note="one batch when the free memory allows: 48 n bytes of workspace per column")
    print("auc", json.dumps(rec["auc"]), flush=True)
    _write(a.out, rec)
    n_chr = a.n_chr
    width = K // n_chr
    runs = []
    for _ in range(a.repeats):
        tab, wall = timed(lambda: ba.snp_grid_AUC(d, y, n_chr=n_chr))
        runs.append(dict(wall_s=wall, **split(ba.auc_last_ms(), n, width, n_chr)))
    rec["snp_grid_AUC"] = dict(n=n, columns=width * n_chr, n_chr=n_chr, sums=width, resident_fp64_runs=runs)
    print("snp_grid_AUC", json.dumps(rec["snp_grid_AUC"]), flush=True)
    _write(a.out, rec)
    d.free()
    if "cpu" not in a.skip:
        import auc_ref
        sub = np.asfortranarray(X32[:, :a.cpu_cols].astype(np.float64))
        tw, cpu_s = timed(lambda: auc_ref.auc(sub, y))
        assert np.array_equal(tw["auc"], res[:a.cpu_cols])
        rec["auc_cpu_twin"] = dict(columns=a.cpu_cols, threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or None, seconds=cpu_s,
                                   scaled_seconds_all_columns=cpu_s * K / a.cpu_cols,
                                   scaled_note="SCALED by the number of columns from the run on %d; not run on all" % a.cpu_cols,
                                   equal_to_device=True)
        print("auc_cpu_twin", json.dumps(rec["auc_cpu_twin"]), flush=True)
        _write(a.out, rec)


def boot_part(a, rec):
    rng = np.random.default_rng(2)
    rec["auc_boot"] = []
    ba.AUCBoot(rng.normal(size=1000), np.r_[0, 1, rng.integers(0, 2, 998)], nboot=64, seed=1)
    rate = None
    for n in a.boot_n:
        y = (rng.uniform(size=n) < 0.3).astype(np.uint8)
        y[:2] = 0, 1
        X = np.asfortranarray(rng.normal(size=(n, 8)))
        for K in (1, 8):
            nboot = a.nboot
            if rate:
                nboot = int(max(64, min(nboot, a.boot_budget * rate / (float(n) * K))))
            r, wall = timed(lambda: ba.AUCBoot(X[:, :K], y, nboot=nboot, seed=5))
            ms = r.ms
            draws = float(nboot) * n * K
            rate = draws / (ms[3] * 1e-3)
            row = dict(n=n, K=K, nboot=nboot, nboot_cut=nboot < a.nboot, wall_s=wall, sort_path_ms=float(ms[:3].sum()),
                       boot_kernel_ms=float(ms[3]), draws=draws, draws_per_s=rate, nan_replicates=int(np.isnan(r.replicates).sum()),
                       mean=float(np.asarray(r).reshape(-1, 4)[0, 0]), sd=float(np.asarray(r).reshape(-1, 4)[0, 3]),
                       note="draws, atomics and evaluation are ONE kernel: no split exists to record")
            rec["auc_boot"].append(row)
            print("auc_boot", json.dumps(row), flush=True)
            _write(a.out, rec)
        if "cpu" not in a.skip and n == a.boot_n[-1]:
            import auc_ref
            rep, cpu_s = timed(lambda: auc_ref.boot(X[:, 0], y, a.cpu_reps, 5))
            dev = ba.AUCBoot(X[:, 0], y, nboot=a.cpu_reps, seed=5).replicates
            assert np.array_equal(rep, dev)
            rec["auc_boot_cpu_twin"] = dict(n=n, replicates=a.cpu_reps, threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or None,
                                            seconds=cpu_s, scaled_seconds_nboot=cpu_s * a.nboot / a.cpu_reps,
                                            scaled_note="SCALED by the number of replicates from the run on %d, one column; not run "
                                            "on all" % a.cpu_reps, equal_to_device=True)
            print("auc_boot_cpu_twin", json.dumps(rec["auc_boot_cpu_twin"]), flush=True)
            _write(a.out, rec)


def prodmat_part(a, rec):
    n, m, K = a.c2_n, a.c2_m, 168
    gb = ba.bed.synthetic(n, m, seed=3)
    rng = np.random.default_rng(3)
    A = np.asfortranarray(rng.normal(0, 0.01, size=(m, K)))
    ir, ic = np.arange(n), np.arange(m)
    center, scale = np.zeros(m), np.ones(m)
    ba.big_prodMat(gb, A[:, :4], center=center, scale=scale)
    ba.prod_and_rowSumsSq(gb, ir, ic, center, scale, A[:, :4])
    rows = dict(big_prodMat=[], big_prodMat_on_device=[], prod_and_rowSumsSq=[])
    for _ in range(a.repeats):                                                # alternating
        XV, t = timed(lambda: ba.big_prodMat(gb, A, center=center, scale=scale))
        rows["big_prodMat"].append(t)
        d, t = timed(lambda: ba.big_prodMat(gb, A, center=center, scale=scale, on_device=True))
        rows["big_prodMat_on_device"].append(t)
        d.free()
        (XV2, _), t = timed(lambda: ba.prod_and_rowSumsSq(gb, ir, ic, center, scale, A))
        rows["prod_and_rowSumsSq"].append(t)
        assert np.array_equal(XV, XV2)
    rec["big_prodMat"] = dict(n=n, m=m, K=K, wall_s=rows, wall_s_median={k: float(np.median(v)) for k, v in rows.items()},
                              result_MB=n * K * 8 / 1e6, equal_to_prod_and_rowSumsSq=True,
                              note="wall clock of the whole call: upload of A, the product pass, download of the result (not for on_device)")
    print("big_prodMat", json.dumps(rec["big_prodMat"]), flush=True)
    _write(a.out, rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300000)
    ap.add_argument("--K", type=int, default=1400)
    ap.add_argument("--n-chr", type=int, default=7)
    ap.add_argument("--nboot", type=int, default=10000)
    ap.add_argument("--boot-n", type=int, nargs="+", default=[10000, 100000, 1000000])
    ap.add_argument("--boot-budget", type=float, default=40.0, help="seconds one AUCBoot call may take at the measured rate")
    ap.add_argument("--cpu-cols", type=int, default=64)
    ap.add_argument("--cpu-reps", type=int, default=256)
    ap.add_argument("--c2-n", type=int, default=50000)
    ap.add_argument("--c2-m", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="*", default=[0, 700, 350, 128, 32], help="BSN_AUC_BATCH values of the sweep (0: unset)")
    ap.add_argument("--skip", nargs="*", default=[], choices=["auc", "boot", "cpu", "prodmat"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auc_c3.json"))
    a = ap.parse_args()
    rec = dict(config="C3 scores", streaming_rate_Bps_of_sfbm_c5=[STREAM_LOW, STREAM_HIGH],
               note="nothing tuned: first shape of every kernel; device ms are HIP events inside the library")
    if "boot" not in a.skip:
        boot_part(a, rec)
    if "auc" not in a.skip:
        auc_part(a, rec)
    if "prodmat" not in a.skip:
        prodmat_part(a, rec)


if __name__ == "__main__":
    main()
