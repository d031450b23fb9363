#!/usr/bin/env python3
"""Per-launch durations of the named kernels in a rocprofv3 `--kernel-trace` output directory: count, median, minimum, maximum in ms, the first launch left out.

    python tools/kernel_launch_stats.py <dir> lbd_describe orb_describe

One JSON line.  For a run whose launches are alone on the device (tools/descriptor_alone.py synchronises after every call) these are the kernels' alone times."""
import csv
import glob
import json
import os
import statistics
import sys


def main():
    d, wanted = sys.argv[1], sys.argv[2:]
    dur = {w: [] for w in wanted}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            base = row["Kernel_Name"].split("(")[0]
            for w in wanted:
                if base.endswith("::" + w) or base == w:
                    dur[w].append((float(row["End_Timestamp"]) - float(row["Start_Timestamp"])) * 1e-6)
    out = {}
    for w, v in dur.items():
        v = v[1:] if len(v) > 2 else v
        out[w] = dict(launches=len(v), median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) if v else None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
