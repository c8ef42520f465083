#!/usr/bin/env python3
"""The timeline of one steady step out of a rocprofv3 --kernel-trace of `bench.py --steps K`: start and end of every dispatch
relative to the step's first, and the idle time in front of each (previous end -> this start).

    kernel_timeline.py kernel_trace.csv [STEP]          STEP counts from the end, default 3 (the third step from the last)

A step begins at every dispatch of k_byte_presence or, where a fill precedes it, at that fill.  Prints a markdown table."""
import csv
import re
import sys


def short(name):
    name = re.sub(r"\bvoid\s+", "", name).replace("sfx::", "").replace("detail::", "")
    head = name.split("(")[0]
    return head if len(head) <= 48 else head[:45] + "..."


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    back = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    begins = []
    for i, r in enumerate(rows):
        if "k_byte_presence" in r["Kernel_Name"]:
            begins.append(i - 1 if i and "fillBuffer" in rows[i - 1]["Kernel_Name"] else i)
    b = begins[-back]
    e = begins[-back + 1] if back > 1 else len(rows)
    step = rows[b:e]
    t0 = int(step[0]["Start_Timestamp"])
    prev_end = None
    busy = 0
    print("| # | dispatch | start µs | end µs | duration µs | idle before µs |")
    print("|---|---|---|---|---|---|")
    for k, r in enumerate(step):
        s, t = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        gap = "" if prev_end is None else f"{(s - prev_end) / 1e3:.1f}"
        busy += t - s
        print(f"| {k + 1} | `{short(r['Kernel_Name'])}` | {(s - t0) / 1e3:.1f} | {(t - t0) / 1e3:.1f} | {(t - s) / 1e3:.1f} | {gap} |")
        prev_end = t
    span = int(step[-1]["End_Timestamp"]) - t0
    print(f"\n{len(step)} dispatches, first start to last end {span / 1e3:.1f} µs, kernels {busy / 1e3:.1f} µs, idle {(span - busy) / 1e3:.1f} µs")


if __name__ == "__main__":
    main()
