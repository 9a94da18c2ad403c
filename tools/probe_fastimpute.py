#!/usr/bin/env python3
"""snp_fastImpute at config C2's sample count -> profiles/fastimpute_c2.json.

A 50 000 x `--m` synthetic 2-bit image with 1 % missing calls (bsn_bed_synthetic, na16 = 655): the columns of C2
(50 000 x 200 000) are independent draws, so `--m` of them are a column subset of it in everything that matters here.
Every variant has missing calls and is a target; its list is what the mirror builds from snp_cor (the variants that pass
the test at `alpha`, or the window of `size` variants on either side: 2 x size = 400 predictors at most; mean and
largest count are recorded).  Recorded: the
call (host clock around snp_fastImpute), snp_cor alone with the arguments the mirror passes, the device time of the
boosting kernel, the image copy and the FBM-bytes kernels (bsn_fast_impute_last_ms), microseconds per target and per
target x round x predictor, the CPU statement (tests/native/fastimpute_ref.cpp, OpenMP) on the first targets with
equality asserted, and the boosting time SCALED to the reference's 15 000 x 300 000 ("a few hours").

    python tools/probe_fastimpute.py [--n 50000] [--m 1024] [--size 200] [--cpu-targets 32] [--threads 16]
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
from bigsnpr_amd import _lib  # noqa: E402
import fastimpute_ref as ref  # noqa: E402

SEED = 20261020
ROUNDS = 10


def last_ms():
    ms = (C.c_double * 3)()
    _lib.check(_lib.load().bsn_fast_impute_last_ms(ms))
    return list(ms)


def _write(path, rec):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--size", type=int, default=200)
    ap.add_argument("--cpu-targets", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastimpute_c2.json"))
    a = ap.parse_args()
    n, m = a.n, a.m
    warnings.simplefilter("ignore")
    gb = ba.bed.synthetic(n, m, na16=655)
    chrom = np.ones(m, dtype=np.int64)
    rec = dict(config="C2 (50 000 x 200 000, 1 % missing), a column subset", n=n, m=m, size=a.size, alpha=1e-4, p_train=0.8,
               seed=SEED, image="2-bit synthetic, 1 % missing (na16 = 655), independent columns",
               note="call = host clock around snp_fastImpute (snp_cor, the predictor lists on the host, the uploads, the "
                    "result image and its bytes); boost / copy / bytes = HIP events inside bsn_fast_impute.  No shape of "
                    "the kernel was decided from a timing: the per-sample state is in LDS when it fits and in global "
                    "scratch otherwise, lanes run over samples.  There is no A/B to record yet.")

    t0 = time.perf_counter()
    res = ba.snp_fastImpute(gb, chrom, size=a.size, seed=SEED, return_bytes=True)
    rec["first_call_s"] = time.perf_counter() - t0
    res._bed.close()
    t0 = time.perf_counter()
    res = ba.snp_fastImpute(gb, chrom, size=a.size, seed=SEED, return_bytes=True)
    call_s = time.perf_counter() - t0
    ms = last_ms()
    t0 = time.perf_counter()
    ba.snp_cor(gb, ind_row=np.arange(n, dtype=np.int64), ind_col=np.arange(m, dtype=np.int64), size=a.size, alpha=1e-4,
               fill_diag=False)
    cor_s = time.perf_counter() - t0
    lens = np.diff(res.pred_off)
    targets = int((res.infos[0] > 0).sum() - res.n_all_missing)
    pred_total = int(lens[(res.infos[0] > 0) & (res.infos[0] < 1)].sum())
    rec.update(call_s=call_s, snp_cor_s=cor_s, boost_ms=ms[0], copy_ms=ms[1], bytes_kernels_ms=ms[2], targets=targets,
               predictors_mean=float(lens.mean()), predictors_max=int(lens.max()),
               us_per_target=ms[0] * 1e3 / max(targets, 1),
               us_per_target_round_predictor=ms[0] * 1e3 / max(ROUNDS * pred_total, 1),
               mean_validation_error=float(np.nanmean(res.infos[1])))
    print(json.dumps(rec), flush=True)
    _write(a.out, rec)

    # the CPU statement on the first targets (their windows lie inside the first cpu_targets + size columns)
    k = min(a.cpu_targets, m)
    width = min(m, k + a.size)
    raw = np.asarray(gb[:, np.arange(width)])
    sub = np.asfortranarray(np.where(raw < 0, 3, raw).astype(np.uint8))
    preds = [res.pred_idx[res.pred_off[j]:res.pred_off[j + 1]] if j < k else np.zeros(0, dtype=np.int32) for j in range(width)]
    assert all(p.size == 0 or p.max() < width for p in preds)
    off, idx = ref.lists(preds)
    ref.fast_impute(sub[:64, :], off, idx, 0.8, SEED, nthreads=a.threads)    # builds and loads the statement
    empty_off = np.zeros(width + 1, dtype=np.int64)
    t0 = time.perf_counter()
    ref.fast_impute(sub, empty_off, idx[:0], 0.8, SEED, nthreads=a.threads)   # what the variants outside the slice cost
    t_empty = time.perf_counter() - t0
    t0 = time.perf_counter()
    want, want_infos, _ = ref.fast_impute(sub, off, idx, 0.8, SEED, nthreads=a.threads)
    t_cpu = time.perf_counter() - t0 - t_empty * (width - k) / width
    equal = bool(np.array_equal(res.bytes[:, :k], want[:, :k]) and
                 np.array_equal(res.infos[:, :k], want_infos[:, :k], equal_nan=True))
    rec["cpu_statement"] = dict(threads=a.threads, targets=k, s=t_cpu, us_per_target=t_cpu * 1e6 / k,
                                equal_to_device=equal, device_over_cpu=(t_cpu / k) / (ms[0] * 1e-3 / max(targets, 1)))
    assert equal, "device and CPU statement differ on the first %d targets" % k
    # scaled, not measured: boosting time ~ samples x targets x predictors
    rec["scaled_to_reference_15000_x_300000"] = dict(
        scaled=True, boost_s=ms[0] * 1e-3 * (15000 / n) * (300000 / max(targets, 1)),
        assumes="every variant a target with as many predictors as here; time proportional to samples x targets; at 15 000 "
                "samples the per-sample state still lies in global scratch",
        reference="'a few hours' (BASELINE.md, snp_fastImpute row)")
    print(json.dumps(rec["cpu_statement"]), json.dumps(rec["scaled_to_reference_15000_x_300000"]), flush=True)
    _write(a.out, rec)


if __name__ == "__main__":
    main()
