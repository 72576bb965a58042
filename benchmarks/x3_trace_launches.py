#!/usr/bin/env python3
"""per-launch statistics of the split-f16 GEMM launches in a rocprofv3 kernel_trace.csv, by (kernel, grid); the N = 768 grid split into proj / fc2 by launch
order; appended to the trace_by_grid.py summary in profiles/x3_tiles_trace_by_grid_*.txt.  usage: x3_trace_launches.py <csv> <steps in the trace> <warm-up steps>"""
import collections
import csv
import statistics
import sys

steps, warm = int(sys.argv[2]), int(sys.argv[3])
rows = [r for r in csv.DictReader(open(sys.argv[1])) if "sgemm_nt_bf16x3_kernel" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
by = collections.defaultdict(list)
for r in rows:
    name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
    grid = r.get("Grid_Size_X", r.get("Grid_Size", "?"))
    by[(name, grid)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)


def line(tag, d):
    print(f"{tag:70s} n={len(d):4d} min={min(d):7.1f} median={statistics.median(d):7.1f} mean={statistics.mean(d):7.1f} max={max(d):7.1f} us  spread={max(d) - min(d):6.1f}")


def both(tag, d):
    line(tag, d)
    if len(d) % steps == 0:
        line("    ... of which the launches of the timed steps", d[len(d) // steps * warm:])


print(f"\nper-launch times of the split-f16 GEMM (us), every launch of the trace ({steps} steps, the first {warm} warm-up):")
for (name, grid), d in sorted(by.items(), key=lambda kv: -sum(kv[1])):
    both(f"{name} grid={grid}", d)
    if grid in ("98304", "131072") and len(d) % 2 == 0 and len(d) >= 24:
        both("  even launches in order (proj, K = 768)", d[0::2])
        both("  odd launches in order (fc2, K = 3072)", d[1::2])
