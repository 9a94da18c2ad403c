#!/usr/bin/env python3
"""bed_king at config C2 -> profiles/king_c2.json.

Synthetic 2-bit images (bsn_bed_synthetic) with 1 % missing calls (na16 = 655: the seven-product path) and without any
(na16 = 0: the two-product path), m = 200 000 variants, n = 16 384 and n = 50 000 samples, thr = 2^-4.5.  Per shape and path:

* the first call on a fresh handle (it builds the sample-major copy) and the call after it, on the host clock;
* the device times of that second call (HIP events inside the library, bsn_king_last_ms: operand, totals, pair kernel,
  compaction);
* the int8 operations the pair kernel executes — tile pairs x 64 x 64 x padded variants x products x 2 — over its time,
  beside the 5 POP/s peak of the int8 matrix pipe.

Then the CPU statement (tests/native/king_ref.cpp, OpenMP) on the first 2 048 samples of the image with missing calls,
compared with the device's table of the same samples and SCALED to each shape by its number of pairs (labelled as scaled:
the CPU did not run at those sizes).

    python tools/probe_king.py [--n 16384 50000] [--m 200000] [--cpu-n 2048] [--out profiles/king_c2.json]
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

PEAK_I8 = 5.0e15
THR = 2 ** -4.5
TILE = 64


def _write(path, rec):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def executed_ops(n, m, products):
    T = (n + TILE - 1) // TILE
    return T * (T + 1) // 2 * TILE * TILE * ((m + 511) // 512 * 512) * products * 2


def one(n, m, na16):
    gb = ba.bed.synthetic(n, m, na16=na16)
    t0 = time.perf_counter()
    t = ba.bed_king(gb, thr_king=THR)
    first = time.perf_counter() - t0
    t0 = time.perf_counter()
    t = ba.bed_king(gb, thr_king=THR)
    call = time.perf_counter() - t0
    ms = ba.king_last_ms()
    products = 2 if ms[1] > 0 else 7
    ops = executed_ops(n, m, products)
    rec = dict(n=n, m=m, na16=na16, path="two products (complete data)" if products == 2 else "seven products", rows=int(t["KINSHIP"].size),
               pairs=n * (n - 1) // 2, first_call_s=first, call_s=call, device_ms=dict(operand=ms[0], totals=ms[1], pairs=ms[2], compaction=ms[3]),
               executed_int8_ops=ops, pair_kernel_POPs=ops / (ms[2] * 1e-3) / 1e15, share_of_int8_peak=ops / (ms[2] * 1e-3) / PEAK_I8)
    gb.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[16384, 50000])
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--cpu-n", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "king_c2.json"))
    a = ap.parse_args()
    rec = dict(config="C2", thr=THR, peak_int8_ops=PEAK_I8, image="2-bit synthetic (bsn_bed_synthetic), 1 % missing (na16 = 655) / none (na16 = 0)",
               note="nothing tuned: first shape of the kernel; call_s is the second call on the handle (host clock, table on the "
                    "host), first_call_s the one that builds the sample-major copy", shapes=[])
    for n in a.n:
        for na16 in (655, 0):
            r = one(n, a.m, na16)
            rec["shapes"].append(r)
            print(json.dumps(r), flush=True)
            _write(a.out, rec)
    if a.cpu_n > 1:
        import king_ref
        nc = a.cpu_n
        gb = ba.bed.synthetic(max(nc, 256), a.m, na16=655)
        G = np.ascontiguousarray(ba.bed_to_bytes(gb, ind_row=np.arange(nc)))
        t0 = time.perf_counter()
        want = king_ref.table(G, thr=THR)
        cpu_s = time.perf_counter() - t0
        got = ba.bed_king(gb, thr_king=THR, ind_row=np.arange(nc))
        equal = all(np.array_equal(got[k], want[k], equal_nan=(k == "KINSHIP")) for k in want)
        pairs = nc * (nc - 1) // 2
        rec["cpu_twin"] = dict(n=nc, m=a.m, threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or None, seconds=cpu_s, pairs=pairs,
                               table_equal_to_device=bool(equal),
                               scaled_seconds={str(r["n"]): cpu_s * r["pairs"] / pairs for r in rec["shapes"] if r["na16"]},
                               scaled_note="SCALED by the number of pairs from the run on %d samples; not run at those sizes" % nc)
        print(json.dumps(rec["cpu_twin"]), flush=True)
        _write(a.out, rec)
        gb.close()


if __name__ == "__main__":
    main()
