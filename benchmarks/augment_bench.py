#!/usr/bin/env python3
"""The five-transform augmentation chain (ScaleAndTranslate, Rotate, Jitter, RandomInputDropout, Flip) of csrc/augment.hip: one JSON line.

    python benchmarks/augment_bench.py [--reps 5] [--inner 20000] [--commit ID] [--out profiles/augment_bench.json]

At 128 x 1024 and 32 x 8192 points the chain is timed three ways, the draws coming from Philox inside the kernel each time:
  fused   one launch of the whole chain (the cloud staged in LDS);
  per_op  five one-op launches, what the chain costs when every transform is a launch of its own;
  global  one launch on the forced global path (no LDS staging).
Each time is the median of ``--reps`` repetitions (with min / max) of a device-event window around ``--inner`` back-to-back calls (0.2 to 1.2 s
at the default), after a warm-up; the three versions alternate inside a repetition and the cloud is restored every 1000 calls.  The calls are
enqueued from Python as a training step enqueues them, so a time includes what the host needs per call where that is the longer of the two.  ``model_bytes`` is what the algorithm has to move -- the batch read once and written
once per launch -- and ``frac_of_hbm_peak`` that over the time over the 8.0 TB/s peak: at 1.5 to 3 MB per launch the chain is bound by launch
and latency, not by bandwidth.  No bar is set on any of these figures.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0
SHAPES = ((128, 1024), (32, 8192))


def spread(vals, digits=2):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


RESTORE_EVERY = 1000       # calls between two restores of the cloud: repeated dropout would collapse it onto point 0, repeated scaling drift it


def window_us(fn, inner, restore):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(inner):
        if i % RESTORE_EVERY == 0:
            restore()                                          # one 3 to 6 MB device copy per 1000 calls: below 0.1 % of the window
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20000)
    ap.add_argument("--commit", type=str, default=os.environ.get("ACT_BENCH_COMMIT"))
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs a GPU: a time taken without one says nothing")
    import act_amd.kernels as K
    dev = torch.device("cuda:0")
    ops = [(K.AUG_SCALE_TRANSLATE, 2. / 3., 1.5, 0.2), (K.AUG_ROTATE_Y, 0., 0., 0.), (K.AUG_JITTER, 0.01, 0.05, 0.), (K.AUG_DROPOUT, 0.5, 0., 0.),
           (K.AUG_FLIP, 1., 0., 0.)]
    res = {"bench": "augment_chain", "commit": args.commit, "device": torch.cuda.get_device_name(0), "ops": len(ops), "reps": args.reps,
           "inner": args.inner, "shapes": {}}
    for B, N in SHAPES:
        g = torch.Generator().manual_seed(B + N)
        pc0 = (torch.randn(B, N, 3, generator=g) * 0.3).to(dev)
        pc = pc0.clone()
        ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        versions = {
            "fused": lambda: K.augment(pc, ops, None, seed=1, seed_dev=ctr),
            "per_op": lambda: [K.augment(pc, [op], None, seed=1 + i, seed_dev=ctr) for i, op in enumerate(ops)],
            "global": lambda: K.augment(pc, ops, None, seed=1, seed_dev=ctr, force_global=True),
        }
        for fn in versions.values():                          # warm-up: code objects, the LDS attribute
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in versions}
        for _ in range(args.reps):
            for k, fn in versions.items():                    # alternate: a drift of the machine lands on all three
                us[k].append(window_us(fn, args.inner, lambda: pc.copy_(pc0)))
        launches = {"fused": 1, "per_op": len(ops), "global": 1}
        entry = {}
        for k in versions:
            by = 24 * B * N * launches[k]
            med = statistics.median(us[k])
            entry[k] = {"us": spread(us[k]), "launches": launches[k], "model_bytes": by, "frac_of_hbm_peak": round(by / (med * 1e-6) / (PEAK_TBS * 1e12), 4)}
        entry["fused_over_per_op"] = round(statistics.median(us["fused"]) / statistics.median(us["per_op"]), 3)
        entry["fused_over_global"] = round(statistics.median(us["fused"]) / statistics.median(us["global"]), 3)
        res["shapes"][f"{B}x{N}"] = entry
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
