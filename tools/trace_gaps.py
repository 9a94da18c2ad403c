#!/usr/bin/env python3
"""Per-solve summary of a rocprofv3 --kernel-trace CSV of bench.py: busy time by kernel, idle gaps, and — since a solve
queues u / v on a second stream (early Rayleigh-Ritz) — how much of each kernel ran BESIDE another one.  "busy" is the
union of the kernel intervals, "idle" the rest of the span; "beside" is the part of a kernel's own time during which
some other kernel was running too.
usage: tools/trace_gaps.py <kernel_trace.csv>"""
import csv, re, sys
from collections import defaultdict
rows = []
for r in csv.DictReader(open(sys.argv[1])):
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void bsn::", "").replace("bsn::", "")))
rows.sort()
# a solve starts at k_random
solves, cur = [], None
for st, en, name in rows:
    if name.startswith("k_random"):
        cur = []
        solves.append(cur)
    if cur is not None:
        cur.append((st, en, name))
for i, s in enumerate(solves):
    t0, t1 = s[0][0], max(en for _, en, _ in s)
    busy = defaultdict(float)
    gap_after = defaultdict(float)
    beside = defaultdict(float)
    tot_busy, reach, reach_name = 0.0, t0, None   # union of the intervals: `reach` = end of everything seen so far, set by `reach_name`
    active = []                                   # earlier kernels (start order) that still run at the current start
    for j, (st, en, name) in enumerate(s):
        short = re.sub(r"<.*", "", name)
        busy[short] += (en - st) / 1e6
        if st > reach and reach_name is not None:
            gap_after[reach_name] += (st - reach) / 1e6   # charged to the kernel whose end the device idled from
        tot_busy += max(0, en - max(st, reach)) / 1e6
        if en > reach or reach_name is None:
            reach, reach_name = max(reach, en), short
        # time of this kernel shared with any other one: the earlier ones still running, and the later ones that start
        # before it ends (the list is in start order, so the scan stops at the first that does not)
        active = [(s2, e2) for s2, e2 in active if e2 > st]
        cover = [(max(st, s2), min(en, e2)) for s2, e2 in active]
        for st2, en2, _ in s[j + 1:]:
            if st2 >= en:
                break
            cover.append((st2, min(en, en2)))
        active.append((st, en))
        at = st
        for a, b in sorted(cover):
            if b > at:
                beside[short] += (b - max(a, at)) / 1e6
                at = b
    print("solve %d: span %.1f ms, busy %.1f ms, idle %.1f ms, %d kernels" % (i, (t1 - t0) / 1e6, tot_busy, (t1 - t0) / 1e6 - tot_busy, len(s)))
    print("   busy: " + ", ".join("%s %.2f" % (k, v) for k, v in sorted(busy.items(), key=lambda kv: -kv[1])[:8]))
    print("   idle after: " + ", ".join("%s %.2f" % (k, v) for k, v in sorted(gap_after.items(), key=lambda kv: -kv[1])[:8]))
    print("   beside another kernel: " + (", ".join("%s %.2f of %.2f" % (k, v, busy[k]) for k, v in sorted(beside.items(), key=lambda kv: -kv[1])[:8]) or "nothing"))
