#!/usr/bin/env python3
"""Per-group genotype counts, bed_fst and snp_MAX3 at config C2 -> profiles/popstat_c2.json.

50 000 x 200 000 synthetic 2-bit image with 1 % missing calls (bsn_bed_synthetic, na16 = 655), every sample labelled with
one of G groups of about equal size.  For G = 2, 3, 16, 17 and 26:

* bed_counts_by_group as a call (host clock around the synchronous call, after a warm-up call, median of the repeats) and
  as device time (HIP events inside the library, bsn_popstat_last_ms: panel, streaming launches, finalising kernels);
* the same table the way it was obtained before, G calls of bed_counts(ind_row = the rows of one group) in the same
  process: the host clock around the G calls and the time between two events on the handle's stream around them (which
  holds the host's work between the kernels too: the library has no event pair inside bed_counts);
* the image bytes a streaming launch reads (every variant row once) over its time, beside the 6.0 - 6.3 TB/s of
  profiles/sfbm_c5.json.

Then bed_fst (26 groups, per variant and overall) and snp_MAX3 end to end, and their share spent in the statistic.

    python tools/probe_popstat.py [--n 50000] [--m 200000] [--repeats 3] [--out profiles/popstat_c2.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bigsnpr_amd as ba  # noqa: E402
from bigsnpr_amd import _lib  # noqa: E402
from bigsnpr_amd.popstat import popstat_last_ms  # noqa: E402

STREAM_TBS = (6.0, 6.3)   # profiles/sfbm_c5.json, README
GROUPS = (2, 3, 16, 17, 26)
SEED = 20261019


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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "popstat_c2.json"))
    a = ap.parse_args()
    n, m = a.n, a.m
    L = _lib.load()
    gb = ba.bed.synthetic(n, m, na16=655)
    pitch = ((n + 3) // 4 + 255) // 256 * 256
    image_bytes = m * pitch
    rng = np.random.default_rng(SEED)
    rec = dict(config="C2", n=n, m=m, image="2-bit synthetic, 1 % missing (na16 = 655)", seed=SEED, pitch=pitch,
               image_bytes_per_launch=image_bytes, streaming_rate_TBs=list(STREAM_TBS),
               note="grouped: one bed_counts_by_group call, device_ms = [panel, streaming launches, finalising kernels, "
                    "statistic]; single: G calls of bed_counts(ind_row = rows of one group), events_ms = time between two "
                    "events on the handle's stream around the G calls (host work between the kernels included)")
    for G in GROUPS:
        lab = rng.integers(0, G, size=n)
        rows = [np.nonzero(lab == g)[0] for g in range(G)]
        grouped = timed(lambda: ba.bed_counts_by_group(gb, lab, n_groups=G), a.repeats, popstat_last_ms)
        launches = (G + 31) // 32
        stream_ms = grouped["device_ms_median"][1]
        grouped["launches"] = launches
        grouped["column_blocks"] = 2 if G > 16 else 1
        grouped["streaming_TBs"] = launches * image_bytes / (stream_ms * 1e-3) / 1e12
        grouped["share_of_streaming_rate"] = [grouped["streaming_TBs"] / s for s in STREAM_TBS]

        ev = []

        def single():
            L.bsn_timer_start(gb.handle)
            out = [ba.bed_counts(gb, ind_row=r) for r in rows]
            ms = C.c_double(0)
            L.bsn_timer_stop(gb.handle, C.byref(ms))
            ev.append(ms.value)
            return out
        one = timed(single, a.repeats)
        one["events_ms_median"] = float(np.median(ev[1:]))
        equal = bool(np.array_equal(np.stack(single()), ba.bed_counts_by_group(gb, lab, n_groups=G)))
        rec["G=%d" % G] = dict(grouped=grouped, single_calls=one, tables_equal=equal,
                               call_ratio_single_over_grouped=one["median_s"] / grouped["median_s"],
                               device_ratio_single_events_over_grouped=one["events_ms_median"] / sum(grouped["device_ms_median"]))
        print(json.dumps({"G": G, **rec["G=%d" % G]}), flush=True)
        _write(a.out, rec)

    lab = rng.integers(0, 26, size=n)
    for name, f in (("bed_fst_26_per_variant", lambda: ba.bed_fst(gb, lab, n_groups=26)),
                    ("bed_fst_26_overall", lambda: ba.bed_fst(gb, lab, n_groups=26, overall=True)),
                    ("snp_MAX3", lambda: ba.snp_MAX3(gb, lab % 2)),
                    ("snp_MAXL_33", lambda: ba.snp_MAX3(gb, lab % 2, val=np.linspace(0, 1, 33)))):
        rec[name] = timed(f, a.repeats, popstat_last_ms)
        print(json.dumps({name: rec[name]}), flush=True)
        _write(a.out, rec)
    # the two-step form of Fst: the frequencies come to the host and go back
    t0 = time.perf_counter()
    ov = ba.snp_fst(ba.bed_MAF_by_group(gb, lab, n_groups=26), overall=True)
    rec["snp_fst_of_bed_MAF_by_group_26_overall"] = dict(s=time.perf_counter() - t0,
                                                         equal_to_bed_fst=bool(ov == ba.bed_fst(gb, lab, n_groups=26, overall=True)))
    print(json.dumps(rec["snp_fst_of_bed_MAF_by_group_26_overall"]), flush=True)
    _write(a.out, rec)
    gb.close()


if __name__ == "__main__":
    main()
