#!/usr/bin/env python3
"""The split-f16 / split-bf16 product launches of a rocprofv3 kernel_trace.csv by their position within the step: for every (kernel, grid) the launches of a
step come in a fixed order, so launch p of the step is the same product in every step and in both builds of an A/B pair.  Prints, per position, the median
(min ... max) and the spread max - min over the timed steps; with a second csv (the change; the first is the parent) prints the gain of every position against
the parent's own spread at that position -- the bar the split-f16 changes are held to (notebook/x3_ktile.md).
usage: x3_launches_by_position.py <parent csv> <steps in the trace> <warm-up steps> [<change csv>]"""
import collections, csv, statistics, sys

# what the positions are in the Stage-II step (bench.py defaults: B = 128, 12 teacher blocks); a key that is not listed is printed without a name
NAMES = {
    ("<128, 192, 2, 4, 0, false, true, false, false>", "131072"): lambda p: ("teacher proj", "teacher fc2")[p % 2] + f" block {p // 2}",
    ("<128, 128, 2, 2, 1, true, true, false, false>", "393216"): lambda p: f"teacher fc1 block {p}",
    ("<128, 128, 2, 2, 0, false, true, false, false>", "294912"): lambda p: f"teacher qkv block {p}",
    ("<128, 128, 2, 2, 0, false, true, false, false>", "196608"): lambda p: f"prompt keys / values block {p}",
    ("<128, 128, 2, 2, 0, false, true, false, false>", "1048576"): lambda p: "tokenizer head",
    ("<128, 128, 2, 2, 0, false, true, true, true>", "1572864"): lambda p: "mini-PointNet group-max product",
    ("<128, 128, 2, 2, 0, false, true, false, false>", "131072"): lambda p: f"dgcnn_{p // 2 + 1} layer {p % 2 + 2}",
    ("<128, 128, 2, 2, 0, false, true, false, false>", "262144"): lambda p: f"dgcnn_{p + 1} layer 4",
}


def positions(path, steps, warm):
    """(template arguments, grid) -> [per position: the launch times (us) of the timed steps]"""
    rows = [r for r in csv.DictReader(open(path)) if "sgemm_nt_bf16x3_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    by = collections.defaultdict(list)
    for r in rows:
        name = r["Kernel_Name"]
        by[(name[name.index("<"):name.index(">") + 1], r.get("Grid_Size_X", r.get("Grid_Size")))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    for key, d in by.items():
        if len(d) % steps:
            print(f"{key}: {len(d)} launches, not a multiple of {steps} steps: skipped")
            continue
        per = len(d) // steps
        out[key] = [[d[s * per + p] for s in range(warm, steps)] for p in range(per)]
    return out


def main():
    steps, warm = int(sys.argv[2]), int(sys.argv[3])
    parent = positions(sys.argv[1], steps, warm)
    change = positions(sys.argv[4], steps, warm) if len(sys.argv) > 4 else None
    med = statistics.median
    for key in sorted(parent, key=lambda k: -sum(med(p) for p in parent[k])):
        per = parent[key]
        print(f"\nsgemm_nt_bf16x3_kernel{key[0]} grid {key[1]}: {len(per)} per step, sum of the positions' medians {sum(med(p) for p in per) / 1e3:.3f} ms/step"
              + (f" -> {sum(med(p) for p in change[key]) / 1e3:.3f}" if change and key in change and len(change[key]) == len(per) else ""))
        gains, bars = collections.defaultdict(list), collections.defaultdict(list)
        for p, d in enumerate(per):
            name = NAMES[key](p) if key in NAMES else f"launch {p}"
            line = f"  {name:36s} n={len(d):3d} median={med(d):7.1f} ({min(d):7.1f} ... {max(d):7.1f}) spread={max(d) - min(d):6.1f}"
            if change and key in change and len(change[key]) == len(per):
                c = change[key][p]
                line += f"   change median={med(c):7.1f} ({min(c):7.1f} ... {max(c):7.1f})  gain={med(d) - med(c):6.1f}  {'>' if med(d) - med(c) > max(d) - min(d) else '<='} bar"
                product = name.split(" block ")[0]
                gains[product].append(med(d) - med(c)); bars[product].append(max(d) - min(d))
            print(line)
        for product in gains:
            g, b = gains[product], bars[product]
            print(f"  => {product}: gain per launch median {med(g):.1f} us (sum {sum(g):.1f} us/step); the parent's spread per position median {med(b):.1f} us; "
                  f"{sum(x > y for x, y in zip(g, b))} of {len(g)} positions above their bar; median gain {'>' if med(g) > med(b) else '<='} median bar")


if __name__ == "__main__":
    main()
