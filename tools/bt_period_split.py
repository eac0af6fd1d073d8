#!/usr/bin/env python3
"""tools/bt_period_split.py <kernel_trace.csv> [last N periods, default 13] -- the period of one decoder object out of a
`rocprofv3 --kernel-trace --output-format csv` run of bench.py: per stream (= per decoder object; per queue where the
trace has no stream column) the decode kernel, the back-trace, the gaps between them and the period, over the last N
batches (the timed steps)."""
import csv
import statistics
import sys
from collections import defaultdict


def main():
    path = sys.argv[1]
    last = int(sys.argv[2]) if len(sys.argv) > 2 else 13
    rows = list(csv.DictReader(open(path)))
    key = "Stream_Id" if rows and "Stream_Id" in rows[0] else "Queue_Id"
    per = defaultdict(list)
    for r in rows:
        name = r["Kernel_Name"]
        kind = "bt" if "fltx_backtrace" in name else "dec" if "fltx_decode_kernel" in name else None
        if kind:
            per[r[key]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind, name))
    for sid in sorted(per):
        ev = sorted(per[sid])
        dec = [e for e in ev if e[2] == "dec"]
        bt = [e for e in ev if e[2] == "bt"]
        if len(dec) < 3 or len(bt) < 3:
            continue
        pairs = []  # (decode, its back-trace)
        for d in dec:
            nxt = [b for b in bt if b[0] >= d[1]]
            if nxt:
                pairs.append((d, nxt[0]))
        pairs = pairs[-(last + 1):]
        series = defaultdict(list)
        for i, (d, b) in enumerate(pairs):
            series["decode"].append(d[1] - d[0])
            series["dec->bt"].append(b[0] - d[1])
            series["backtrace"].append(b[1] - b[0])
            if i + 1 < len(pairs):
                series["bt->dec"].append(pairs[i + 1][0][0] - b[1])
                series["period"].append(pairs[i + 1][0][0] - d[0])
        print("%s %s  (%s | %s)" % (key, sid, pairs[-1][0][3][:60], pairs[-1][1][3][:60]))
        for k in ("decode", "dec->bt", "backtrace", "bt->dec", "period"):
            v = [x / 1000.0 for x in series[k]]
            print("  %-9s n=%d mean=%.1f med=%.1f min=%.1f max=%.1f us" %
                  (k, len(v), statistics.mean(v), statistics.median(v), min(v), max(v)))


if __name__ == "__main__":
    main()
