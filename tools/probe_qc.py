#!/usr/bin/env python3
"""bed_plinkQC and the exact Hardy-Weinberg test at config C2 -> profiles/qc_c2.json.

50 000 x 200 000 synthetic 2-bit image with 1 % missing calls (bsn_bed_synthetic, na16 = 655); 80 % of the samples are
founders counted for the test, 15 % founders that are not, 5 % non-founders.  Recorded:

* the filter call (bsn_bed_qc through bigsnpr_amd.qc, the reference's default thresholds) on the host clock, after a
  warm-up call, median of the repeats, and its four device times (bsn_qc_last_ms: per-sample counts, per-class counting
  pass, test kernel, masks);
* bed_hwe the same way;
* the test kernel alone on the counts of all samples, in both lane forms (bsn_hwe_lanes: one lane per variant / two
  adjacent lanes, one walk each), device ms by HIP events, median of the repeats, and whether the two return the same bits.
  The form the library takes (kHweLanes in csrc/qc.hip) is decided by these two numbers against each other, at this shape;
* the mean and the largest trip count (terms formed per variant, from the CPU statement);
* the CPU statement (tests/native/hwe_ref.cpp, OpenMP, OMP_NUM_THREADS threads) on the first --twin-cols variants, and
  whether the kernel returns its bits.

    python tools/probe_qc.py [--n 50000] [--m 200000] [--repeats 5] [--twin-cols 20000] [--out profiles/qc_c2.json]
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
from bigsnpr_amd import qc  # noqa: E402

SEED = 20261020


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
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--twin-cols", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qc_c2.json"))
    a = ap.parse_args()
    n, m = a.n, a.m
    gb = ba.bed.synthetic(n, m, na16=655)
    rng = np.random.default_rng(SEED)
    cls = rng.choice(3, size=n, p=(0.8, 0.15, 0.05)).astype(np.int32)
    ir, ic = np.arange(n, dtype=np.int64), np.arange(m, dtype=np.int64)
    rec = dict(config="C2", n=n, m=m, image="2-bit synthetic, 1 % missing (na16 = 655)", seed=SEED,
               classes="80 % founders counted for the test, 15 % founders not counted, 5 % non-founders",
               thresholds=dict(maf=0.01, geno=0.1, mind=0.1, hwe=1e-50),
               note="device_ms = [per-sample counts, per-class counting pass, test kernel, masks]")

    kept = {}

    def call():
        kept["r"] = qc._qc_call(gb, ir, ic, cls, 0.01, 0.1, 0.1, 1e-50, False)
    rec["bed_plinkQC"] = timed(call, a.repeats, qc.qc_last_ms)
    keep_row, keep_col, _, _ = kept["r"]
    rec["bed_plinkQC"].update(samples_kept=int(keep_row.sum()), variants_kept=int(keep_col.sum()))
    print(json.dumps({"bed_plinkQC": rec["bed_plinkQC"]}), flush=True)
    _write(a.out, rec)

    rec["bed_hwe"] = timed(lambda: ba.bed_hwe(gb), a.repeats, qc.qc_last_ms)
    print(json.dumps({"bed_hwe": rec["bed_hwe"]}), flush=True)
    _write(a.out, rec)

    p, counts = ba.bed_hwe(gb, counts=True)
    t3 = np.ascontiguousarray(counts[:3])
    lanes = {}
    for form in (0, 1, 2):                     # (0: the form the library takes)
        out = [qc._hwe_lanes(t3, False, form) for _ in range(a.repeats + 1)][1:]
        lanes[form] = out[0][0]
        rec["kernel_lanes_%d" % form] = dict(device_ms_median=float(np.median([ms for _, ms in out])),
                                             device_ms=[float(ms) for _, ms in out])
    rec["lane_forms_same_bits"] = bool(np.array_equal(lanes[1].view(np.uint64), lanes[2].view(np.uint64)) and
                                       np.array_equal(lanes[1].view(np.uint64), p.view(np.uint64)))
    rec["two_lanes_over_one"] = rec["kernel_lanes_2"]["device_ms_median"] / rec["kernel_lanes_1"]["device_ms_median"]
    print(json.dumps({k: rec[k] for k in ("kernel_lanes_1", "kernel_lanes_2", "lane_forms_same_bits", "two_lanes_over_one")}),
          flush=True)
    _write(a.out, rec)

    import hwe_ref
    k = min(a.twin_cols, m)
    hwe_ref.exact(t3[:, :64])                                  # (builds and loads the library)
    t0 = time.perf_counter()
    want, steps = hwe_ref.exact(t3[:, :k], steps=True)
    rec["cpu_statement"] = dict(variants=k, threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or None,
                                s=time.perf_counter() - t0,
                                kernel_returns_its_bits=bool(np.array_equal(want.view(np.uint64), p[:k].view(np.uint64))))
    rec["trip_count"] = dict(over_variants=k, mean=float(steps.mean()), max=int(steps.max()), min=int(steps.min()))
    print(json.dumps({k_: rec[k_] for k_ in ("cpu_statement", "trip_count")}), flush=True)
    _write(a.out, rec)
    gb.close()


if __name__ == "__main__":
    main()
