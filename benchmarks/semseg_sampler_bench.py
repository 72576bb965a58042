#!/usr/bin/env python3
"""S3DIS training blocks sampled on the device from resident rooms (act_amd/datasets/S3DISDevice.py, csrc/s3dis_sample.hip): one JSON line.

    python benchmarks/semseg_sampler_bench.py [--commit ID] [--out profiles/semseg_sampler_bench.json]

Rooms: uniform random boxes of 200,000 points (6 x 5 x 3 m) and 1,000,000 points (10 x 8 x 3 m), float64, random labels.  Per room:
  * the device time of one batch (B = 32, N = 2048, one launch): ``--windows`` windows of ``--calls`` back-to-back calls between two device
    events, every call with fresh item ids; the median window (with min / max) over the calls of a window;
  * the index build time (build_index on the resident tensor, host clock around a device synchronise) and the resident bytes;
  * ``S3DISDataset.sample_block`` per item on the same room on the host (``--host_items`` items, host clock) and 32 x that, the cost of a batch
    on one core.
The training step the sampler feeds (benchmarks/semseg_bench.py's step at B = 32, N = 2048, default form) is timed in the same session.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOMS = [(200_000, 6.0, 5.0), (1_000_000, 10.0, 8.0)]


def room(n, w, d, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform([0.0, 0.0, 0.0], [w, d, 3.0], size=(n, 3)), rng.integers(0, 13, n).astype(np.float64)


def one(n, w, d, args, dev):
    from act_amd.datasets.S3DISDevice import DeviceS3DISBlocks, build_index
    from act_amd.datasets.S3DISDataset import sample_block
    pts, lab = room(n, w, d, n)
    blocks = DeviceS3DISBlocks([pts], [lab], args.npoint, device=dev)
    build = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        build_index(blocks.index.xyz, [0, n], 1.0)
        torch.cuda.synchronize()
        build.append((time.perf_counter() - t0) * 1e3)
    B = args.batch
    rooms = torch.zeros(B, dtype=torch.int32, device=dev)
    ids = [torch.arange(i * B, (i + 1) * B, dtype=torch.int32, device=dev) for i in range(args.calls)]
    out = blocks.sample(rooms, ids[0], 0, 0)
    torch.cuda.synchronize()
    windows = []
    for wdw in range(args.windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(args.calls):
            out = blocks.sample(rooms, ids[i], 0, wdw, validate=False)
        b.record()
        b.synchronize()
        windows.append(a.elapsed_time(b) / args.calls)
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    for _ in range(args.host_items):
        sample_block(pts, lab, args.npoint, 1.0, rng)
    host = (time.perf_counter() - t0) * 1e3 / args.host_items
    room_bytes, index_bytes = blocks.resident_bytes()
    dev_ms = statistics.median(windows)
    return {"points": n, "footprint_m": [w, d], "device_ms_per_batch": {"median": round(dev_ms, 4), "min": round(min(windows), 4),
                                                                         "max": round(max(windows), 4)},
            "index_build_ms": round(statistics.median(build), 2), "resident_bytes": {"rooms": room_bytes, "index": index_bytes},
            "max_window": blocks.index.max_window, "mean_count": round(float(out.count.float().mean()), 1),
            "mean_attempts": round(float(out.info.float().abs().mean()), 3), "fallbacks": int((out.info < 0).sum()),
            "host_sample_block_ms_per_item": round(host, 3), "host_ms_per_batch_one_core": round(host * B, 1),
            "host_batch_over_device_batch": round(host * B / dev_ms, 1)}


def train_step_ms(args, dev):
    spec = importlib.util.spec_from_file_location("semseg_bench", os.path.join(ROOT, "benchmarks", "semseg_bench.py"))
    sb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sb)
    ms, _ = sb.time_steps(argparse.Namespace(batch=args.batch, npoint=args.npoint, steps=20, warmup=5), dev, True)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--npoint", type=int, default=2048)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--host_items", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--commit", type=str, default=os.environ.get("ACT_BENCH_COMMIT"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("semseg_sampler_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    runs = [one(n, w, d, args, dev) for n, w, d in ROOMS]
    step = train_step_ms(args, dev)
    res = {"workload": "semseg_device_sampler", "commit": args.commit, "batch": args.batch, "npoint": args.npoint, "windows": args.windows,
           "calls_per_window": args.calls, "runs": runs, "train_step_ms": round(step, 3),
           "sampler_share_of_train_step": [round(r["device_ms_per_batch"]["median"] / step, 4) for r in runs]}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
