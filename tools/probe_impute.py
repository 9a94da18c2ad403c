#!/usr/bin/env python3
"""snp_fastImputeSimple at config C2 -> profiles/impute_c2.json.

50 000 x 200 000 synthetic 2-bit image with 1 % missing calls (bsn_bed_synthetic, na16 = 655).  For every method: the call
without bytes (host clock around the synchronous call, after a warm-up call, with the spread of the repeats), the
device time of its two phases (HIP events inside the library, bsn_impute_last_ms: counts + rule, rewrite) and the bytes
the rewrite reads and writes over its time, set against the 6.0 - 6.3 TB/s streaming rate of profiles/sfbm_c5.json.  For
`mode` also the call with the FBM bytes (10 GB to the host) and the CPU statement (tests/native/impute_ref.cpp, OpenMP)
on a subset of the columns, scaled to m; the device's bytes on those columns are compared with it.

    python tools/probe_impute.py [--n 50000] [--m 200000] [--cpu-cols 4096] [--threads 16] [--repeats 5] [--no-bytes]
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
import impute_ref as ref  # noqa: E402

STREAM_TBS = (6.0, 6.3)   # profiles/sfbm_c5.json, README
METHODS = ("zero", "mode", "mean0", "mean2", "random")
SEED = 20261018


def last_ms():
    ms = (C.c_double * 3)()
    _lib.check(_lib.load().bsn_impute_last_ms(ms))
    return list(ms)


def timed(f, repeats):
    f()                                       # warm-up: code objects, work buffers, the handle's resident counts
    ts, dev = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
        dev.append(last_ms())
        out._bed.close()                      # the result image goes back before the next one is made
    dev = np.array(dev)
    return dict(median_s=float(np.median(ts)), min_s=float(min(ts)), max_s=float(max(ts)), repeats=repeats,
                counts_rule_ms_median=float(np.median(dev[:, 0])), rewrite_ms_median=float(np.median(dev[:, 1])),
                rewrite_ms_min=float(dev[:, 1].min()), rewrite_ms_max=float(dev[:, 1].max()),
                bytes_kernels_ms_median=float(np.median(dev[:, 2])))


def _write(path, rec):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--cpu-cols", type=int, default=4096)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-bytes", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "impute_c2.json"))
    a = ap.parse_args()
    n, m = a.n, a.m
    warnings.simplefilter("ignore")
    gb = ba.bed.synthetic(n, m, na16=655)
    pitch2, pitch8 = ((n + 3) // 4 + 255) // 256 * 256, (n + 255) // 256 * 256
    rec = dict(config="C2", n=n, m=m, image="2-bit synthetic, 1 % missing (na16 = 655)", seed=SEED,
               streaming_rate_TBs=list(STREAM_TBS), pitch_2bit=pitch2, pitch_int8=pitch8,
               note="rewrite = the one kernel that reads the source image and writes the result image (HIP events around "
                    "it); counts_rule = copy of the handle's resident counts (a counting pass on the warm-up call only) "
                    "plus the per-variant rule; the call is the host clock around snp_fastImputeSimple, allocation of "
                    "the result image and the download of the per-variant values included")
    for method in METHODS:
        r = timed(lambda: ba.snp_fastImputeSimple(gb, method, seed=SEED), a.repeats)
        moved = m * (pitch2 + (pitch8 if method == "mean2" else pitch2))
        r["rewrite_bytes"] = moved
        r["rewrite_TBs"] = moved / (r["rewrite_ms_median"] * 1e-3) / 1e12
        r["share_of_streaming_rate"] = [r["rewrite_TBs"] / s for s in STREAM_TBS]
        rec[method] = r
        print(json.dumps({method: r}), flush=True)
        _write(a.out, rec)

    # the first call on a fresh handle: the counting pass is part of it
    fresh = ba.bed.synthetic(n, m, na16=655)
    t0 = time.perf_counter()
    out = ba.snp_fastImputeSimple(fresh, "mode")
    rec["mode_first_call_on_a_fresh_handle"] = dict(s=time.perf_counter() - t0, device_ms=last_ms())
    out._bed.close()
    fresh.close()
    _write(a.out, rec)

    # the CPU statement on a subset of the columns, scaled to m
    cols = np.sort(np.random.default_rng(SEED).choice(m, min(a.cpu_cols, m), replace=False))
    sub = np.asfortranarray(np.where(np.asarray(gb[:, cols]) < 0, 3, np.asarray(gb[:, cols])).astype(np.uint8))
    ref.impute(sub[:, :64], "mode", nthreads=a.threads)    # builds and loads the statement
    t0 = time.perf_counter()
    want = ref.impute(sub, "mode", nthreads=a.threads)[0]
    t_cpu = time.perf_counter() - t0
    rec["cpu_statement_mode"] = dict(threads=a.threads, subset_columns=int(cols.size), subset_s=t_cpu,
                                     scaled_s=t_cpu * m / cols.size)
    rec["device_over_cpu_mode"] = rec["cpu_statement_mode"]["scaled_s"] / rec["mode"]["median_s"]
    print(json.dumps(rec["cpu_statement_mode"]), flush=True)
    _write(a.out, rec)

    if not a.no_bytes:
        t0 = time.perf_counter()
        res = ba.snp_fastImputeSimple(gb, "mode", return_bytes=True)
        t_first = time.perf_counter() - t0
        ms = last_ms()
        rec["mode_with_fbm_bytes"] = dict(first_call_s=t_first, fbm_bytes=int(n) * int(m), bytes_kernels_ms=ms[2],
                                          equal_to_cpu_statement_on_subset=bool(np.array_equal(res.bytes[:, cols], want)),
                                          note="one call, not repeated: 10 GB over PCIe into pageable memory")
        print(json.dumps(rec["mode_with_fbm_bytes"]), flush=True)
        _write(a.out, rec)


if __name__ == "__main__":
    main()
