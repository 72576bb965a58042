#!/usr/bin/env python3
"""per-launch statistics (min, median, mean, max) of chosen launches in a rocprofv3 kernel_trace.csv, by (kernel, grid); appended to the trace_by_grid.py
summary in profiles/*_trace_by_grid_*.txt.
usage: grid_trace_launches.py <csv> <steps in the trace> <warm-up steps> [<grid x>:<kernel name part> ...]
Without selectors: the grid-1,572,864 GEMM launches -- the last product of the frozen tokenizer's mini-PointNet on the f32 fused kernel or on the split-f16
kernel (profiles/pn_f16x3_trace_by_grid_*.txt).  With selectors, e.g. the teacher's prompt keys / values (profiles/prompt_kv_f16x3_trace_by_grid_*.txt):
  49152:prompt_kv_correct_kernel 528640:prompt_kv_rows_kernel 12288:sgemm_nt_asm_kernel 524288:prompt_layernorm_fwd_kernel 196608:sgemm_nt_bf16x3_kernel"""
import collections, csv, statistics, sys
steps, warm = int(sys.argv[2]), int(sys.argv[3])
sel = [tuple(a.split(":", 1)) for a in sys.argv[4:]] or [("1572864", "sgemm_nt16_kernel"), ("1572864", "sgemm_nt_bf16x3_kernel")]
rows = [r for r in csv.DictReader(open(sys.argv[1])) if any(r.get("Grid_Size_X", r.get("Grid_Size")) == g and part in r["Kernel_Name"] for g, part in sel)]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
by = collections.defaultdict(list)
for r in rows:
    name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
    if len(sys.argv) > 4: name += " grid=" + r.get("Grid_Size_X", r.get("Grid_Size"))
    by[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
def line(tag, d):
    print(f"{tag:86s} n={len(d):4d} min={min(d):7.1f} median={statistics.median(d):7.1f} mean={statistics.mean(d):7.1f} max={max(d):7.1f} us")
what = "the grid-1,572,864 GEMM launches" if len(sys.argv) <= 4 else "the launches of " + ", ".join(f"{p} (grid {g})" for g, p in sel)
print(f"\nper-launch times (us) of {what} ({steps} steps in the trace, the first {warm} warm-up):")
for name, d in sorted(by.items(), key=lambda kv: -sum(kv[1])):
    line(name, d)
    if len(d) % steps == 0:
        line("    ... of which the launches of the timed steps", d[len(d) // steps * warm:])
