#!/usr/bin/env python3
"""per-launch statistics (min, median, mean, max) of the grid-1,572,864 GEMM launches in a rocprofv3 kernel_trace.csv -- the last product of the frozen tokenizer's
mini-PointNet on the f32 fused kernel or on the split-f16 kernel; appended to the trace_by_grid.py summary in profiles/pn_f16x3_trace_by_grid_*.txt.
usage: grid_trace_launches.py <csv> <steps in the trace> <warm-up steps>"""
import collections, csv, statistics, sys
steps, warm = int(sys.argv[2]), int(sys.argv[3])
rows = [r for r in csv.DictReader(open(sys.argv[1])) if r.get("Grid_Size_X", r.get("Grid_Size")) == "1572864" and
        ("sgemm_nt16_kernel" in r["Kernel_Name"] or "sgemm_nt_bf16x3_kernel" in r["Kernel_Name"])]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
by = collections.defaultdict(list)
for r in rows:
    name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
    by[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
def line(tag, d):
    print(f"{tag:86s} n={len(d):4d} min={min(d):7.1f} median={statistics.median(d):7.1f} mean={statistics.mean(d):7.1f} max={max(d):7.1f} us")
print(f"\nper-launch times (us) of the grid-1,572,864 GEMM launches ({steps} steps in the trace, the first {warm} warm-up):")
for name, d in sorted(by.items(), key=lambda kv: -sum(kv[1])):
    line(name, d)
    if len(d) % steps == 0:
        line("    ... of which the launches of the timed steps", d[len(d) // steps * warm:])
