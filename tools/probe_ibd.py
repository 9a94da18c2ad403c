#!/usr/bin/env python3
"""bed_ibd at config C2 -> profiles/ibd_c2.json.

The shapes of tools/probe_king.py: synthetic 2-bit images (bsn_bed_synthetic) with 1 % missing calls (na16 = 655: the
seven-product path of the pair kernel) and without any (na16 = 0: the two-product path), m = 200 000 variants, n = 16 384 and
n = 50 000 samples, pi_hat = 0.2, every sample a frequency sample.  Per shape and path:

* the first call on a fresh handle (it builds the sample-major copy) and the call after it, on the host clock;
* the device times of that second call (HIP events inside the library, bsn_ibd_last_ms: operand, totals, pair kernel,
  compaction, the counting pass of the frequency samples, the moment kernels);
* a bed_king call on the same handle in the same process, with its own split: the pair kernel is the same code.

Then the CPU statement (tests/native/ibd_ref.cpp, OpenMP) on the first 2 048 samples of the image with missing calls,
compared with the device's table of the same samples.  Everything is reported; no time is a target.

    python tools/probe_ibd.py [--n 16384 50000] [--m 200000] [--cpu-n 2048] [--out profiles/ibd_c2.json]
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

PI_HAT = 0.2
THR_KING = 2 ** -4.5


def _write(path, rec):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def one(n, m, na16):
    gb = ba.bed.synthetic(n, m, na16=na16)
    t0 = time.perf_counter()
    t = ba.bed_ibd(gb, pi_hat=PI_HAT)
    first = time.perf_counter() - t0
    t0 = time.perf_counter()
    t = ba.bed_ibd(gb, pi_hat=PI_HAT)
    call = time.perf_counter() - t0
    ms = ba.ibd_last_ms()
    t0 = time.perf_counter()
    k = ba.bed_king(gb, thr_king=THR_KING)
    king_call = time.perf_counter() - t0
    kms = ba.king_last_ms()
    rec = dict(n=n, m=m, na16=na16, path="two products (complete data)" if ms[1] > 0 else "seven products", rows=int(t["PI_HAT"].size),
               pairs=n * (n - 1) // 2, n_used=t["n_used"], E=t["E"].tolist(), first_call_s=first, call_s=call,
               device_ms=dict(operand=ms[0], totals=ms[1], pairs=ms[2], compaction=ms[3], counts=ms[4], moments=ms[5]),
               bed_king=dict(call_s=king_call, rows=int(k["KINSHIP"].size),
                             device_ms=dict(operand=kms[0], totals=kms[1], pairs=kms[2], compaction=kms[3])))
    gb.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[16384, 50000])
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--cpu-n", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ibd_c2.json"))
    a = ap.parse_args()
    rec = dict(config="C2", pi_hat=PI_HAT, thr_king=THR_KING,
               image="2-bit synthetic (bsn_bed_synthetic), 1 % missing (na16 = 655) / none (na16 = 0)",
               note="nothing tuned: reported, no target; call_s is the second call on the handle (host clock, table on the host), "
                    "first_call_s the one that builds the sample-major copy; bed_king runs after them on the same handle",
               shapes=[])
    for n in a.n:
        for na16 in (655, 0):
            r = one(n, a.m, na16)
            rec["shapes"].append(r)
            print(json.dumps(r), flush=True)
            _write(a.out, rec)
    if a.cpu_n > 1:
        import ibd_ref
        nc = a.cpu_n
        gb = ba.bed.synthetic(max(nc, 256), a.m, na16=655)
        G = np.ascontiguousarray(ba.bed_to_bytes(gb, ind_row=np.arange(nc)))
        t0 = time.perf_counter()
        want = ibd_ref.table(G, min_pi_hat=0.0)
        cpu_s = time.perf_counter() - t0
        got = ba.bed_ibd(gb, pi_hat=0.0, ind_row=np.arange(nc))
        equal = all(np.array_equal(got[k], want[k], equal_nan=True) for k in want if k != "fired")
        rec["cpu_twin"] = dict(n=nc, m=a.m, threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or None, seconds=cpu_s,
                               pairs=nc * (nc - 1) // 2, rows=int(want["PI_HAT"].size), fired=want["fired"],
                               table_equal_to_device=bool(equal))
        print(json.dumps(rec["cpu_twin"]), flush=True)
        _write(a.out, rec)
        gb.close()


if __name__ == "__main__":
    main()
