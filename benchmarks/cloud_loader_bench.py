#!/usr/bin/env python3
"""Object-dataset batches made on the device from a resident split (act_amd/datasets/DeviceClouds.py, csrc/cloud_sample.hip): one JSON line.

    python benchmarks/cloud_loader_bench.py [--commit ID] [--parent_tree DIR --parent_commit ID] [--out profiles/cloud_loader_bench.json]

  * the device time of one batch (one launch) for 128 x (8192 -> 1024) normalised, 32 x (8192 -> 8192) permuted only and 32 x (8192 -> 8192)
    normalised: ``--windows`` windows of ``--calls`` back-to-back calls between two device events, every call with fresh ids; the median window
    (with min / max).  The difference of the last two shapes is what the normalisation (LDS staging, the serial column sums, the divisions) adds;
  * host clouds/s of the file-backed ``ShapeNet`` DataLoader (batch 128, pinned, persistent workers, one warm-up epoch) on ``--host_files``
    8192-point .npy files written to a temporary directory, at num_workers 0, 4 and 8;
  * the Stage-II step rate of ``runner_pretrain.train_step`` (the loop of run_net: one batch of look-ahead) fed by that DataLoader at each worker
    count, by the resident loader over the same files, and by a pool of batches already on the device (bench.py's feed);
  * with ``--parent_tree`` (a built checkout of the parent commit): ``bench.py --gpus 1`` of that tree and of this one, in this session.
Figures that were not taken are reported as "not measured yet".
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("128x8192to1024_normalised", 128, 1024, True, True), ("32x8192to8192_permute_only", 32, 8192, True, False),
          ("32x8192to8192_normalised", 32, 8192, True, True)]
NOT_MEASURED = "not measured yet"


def kernel_times(args, dev):
    import act_amd.kernels as K
    M = 512
    clouds = torch.randn(M, 8192, 3, device=dev)
    out = {}
    for name, B, n, permute, normalize in SHAPES:
        ids = [((torch.arange(B, device=dev) + i * B) % M).to(torch.int32) for i in range(args.calls)]
        draws = [torch.arange(i * B, (i + 1) * B, dtype=torch.int32, device=dev) for i in range(args.calls)]
        K.cloud_sample(clouds, ids[0], draws[0], n, 0, 0, permute, normalize)
        torch.cuda.synchronize()
        windows = []
        for w in range(args.windows):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(args.calls):
                K.cloud_sample(clouds, ids[i], draws[i], n, 0, w, permute, normalize, validate=False)
            b.record()
            b.synchronize()
            windows.append(a.elapsed_time(b) / args.calls)
        med = statistics.median(windows)
        out[name] = {"B": B, "N": 8192, "n": n, "permute": permute, "normalize": normalize,
                     "device_ms_per_batch": {"median": round(med, 4), "min": round(min(windows), 4), "max": round(max(windows), 4)},
                     "clouds_per_s": round(B / med * 1e3, 1)}
    out["normalisation_adds_ms_at_32x8192"] = round(out[SHAPES[2][0]]["device_ms_per_batch"]["median"] -
                                                    out[SHAPES[1][0]]["device_ms_per_batch"]["median"], 4)
    return out


def write_files(root, count):
    from act_amd.datasets.SyntheticDataset import ShapeNet
    from act_amd.utils.config import EasyDict
    pc = os.path.join(root, "pc")
    os.makedirs(pc)
    g = np.random.default_rng(0)
    with open(os.path.join(root, "train.txt"), "w") as f:
        for i in range(count):
            np.save(os.path.join(pc, f"{i % 55:08d}-{i:06d}.npy"), g.standard_normal((8192, 3)).astype(np.float32))
            f.write(f"{i % 55:08d}-{i:06d}.npy\n")
    return ShapeNet(EasyDict(N_POINTS=8192, subset="train", npoints=1024, DATA_PATH=root, PC_PATH=pc))


def host_loader(ds, workers, batch):
    from act_amd.utils.misc import worker_init_fn
    return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True, drop_last=True, num_workers=workers, worker_init_fn=worker_init_fn,
                                       pin_memory=True, persistent_workers=workers > 0)


def loader_rate(loader, batch, epochs=2):
    for _ in loader:                                                         # warm-up: the workers start, the files enter the page cache
        pass
    t0 = time.perf_counter()
    n = 0
    for _ in range(epochs):
        for _ in loader:
            n += batch
    return n / (time.perf_counter() - t0)


def stage2(dev):
    from act_amd.models import build_model_from_cfg
    from act_amd.tools import builder
    from act_amd.tools.runner_pretrain import freeze_unused_heads, _Single
    from act_amd.utils.config import cfg_from_yaml_file
    from act_amd.utils.logger import get_logger
    import logging
    for n in ("ACT", "Transformer"):
        get_logger(n).setLevel(logging.ERROR)
    config = cfg_from_yaml_file("cfgs/pretrain/pretrain_act_distill.yaml")
    config.model.dvae_config.ckpt = "none"
    torch.manual_seed(0)
    model = build_model_from_cfg(config.model)
    freeze_unused_heads(model)
    model.to(dev).train()
    wrapped = _Single(model)
    optimizer, _ = builder.build_opti_sche(wrapped, config)
    return wrapped, optimizer, config


def step_rate(feed, state, dev, batch, steps, warmup):
    """clouds/s of run_net's loop over ``feed`` (a callable -> a fresh iterator of batch tuples, called again when an epoch ends)"""
    from act_amd.tools.runner_pretrain import train_step
    wrapped, optimizer, config = state

    def batches():
        while True:
            for nxt in feed():
                yield nxt[2].to(dev, non_blocking=True)
    it = batches()
    points = next(it)
    t0 = None
    for i in range(warmup + steps):
        if i == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        nxt = next(it)
        loss = train_step(wrapped, optimizer, points, config, next_points=nxt)
        points = nxt
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if not np.isfinite(float(loss)):
        raise RuntimeError("cloud_loader_bench: non-finite loss")
    return {"clouds_per_s": round(batch * steps / dt, 1), "ms_per_step": round(1e3 * dt / steps, 3)}


def bench_py(tree, steps, warmup):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline",
                        "--no-other-workloads", "--no-instrument"], cwd=tree, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} failed:\n{r.stderr[-2000:]}")
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return {"clouds_per_s": round(d["value"], 1), "ms_per_step": round(d["ms_per_step"], 3), "metric": d["metric"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--host_files", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--workers", type=int, nargs="*", default=[0, 4, 8])
    ap.add_argument("--parent_tree", type=str, default=None, help="a built checkout of the parent commit: its bench.py is run in this session")
    ap.add_argument("--parent_commit", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--commit", type=str, default=os.environ.get("ACT_BENCH_COMMIT"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cloud_loader_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    from act_amd.datasets import DeviceClouds, DeviceCloudLoader

    kernels = kernel_times(args, dev)
    res = {"workload": "object_dataset_device_loader", "commit": args.commit, "windows": args.windows, "calls_per_window": args.calls,
           "kernel": kernels, "host_files": args.host_files, "batch": args.batch, "cpus_available": len(os.sched_getaffinity(0))}
    with tempfile.TemporaryDirectory() as tmp:
        ds = write_files(tmp, args.host_files)
        state = stage2(dev)
        steps, res["host_loader_clouds_per_s"] = {}, {}
        for w in args.workers:                                               # one set of workers alive at a time
            l = host_loader(ds, w, args.batch)
            res["host_loader_clouds_per_s"][str(w)] = round(loader_rate(l, args.batch), 1)
            steps[f"host_loader_{w}_workers"] = step_rate(lambda: iter(l), state, dev, args.batch, args.steps, args.warmup)
            del l
        t0 = time.perf_counter()
        dc = DeviceClouds.from_dataset(ds, device=dev)
        torch.cuda.synchronize()
        res["resident"] = {"clouds": len(dc), "bytes": dc.resident_bytes(), "load_s": round(time.perf_counter() - t0, 2)}
        resident = DeviceCloudLoader(dc, args.batch, shuffle=True, drop_last=True)
        steps["device_loader"] = step_rate(lambda: iter(resident), state, dev, args.batch, args.steps, args.warmup)
        pool = [("", "", torch.randn(args.batch, 1024, 3, device=dev)) for _ in range(4)]
        steps["resident_pool_no_loader"] = step_rate(lambda: (tuple(p[:2]) + (p[2].clone(),) for p in pool), state, dev, args.batch, args.steps,
                                                     args.warmup)
        res["stage2_train_step"] = steps
    del state
    torch.cuda.empty_cache()
    res["bench_py_this_commit"] = bench_py(ROOT, 20, 5)
    res["parent_commit"] = args.parent_commit
    res["bench_py_parent_commit"] = bench_py(args.parent_tree, 20, 5) if args.parent_tree else NOT_MEASURED
    dev_ms = kernels[SHAPES[0][0]]["device_ms_per_batch"]["median"]
    parent = res["bench_py_parent_commit"]
    res["device_batch_share_of_parent_step"] = round(dev_ms / parent["ms_per_step"], 5) if isinstance(parent, dict) else NOT_MEASURED
    best = max(res["host_loader_clouds_per_s"].values())
    res["device_batch_over_best_host_loader"] = round(kernels[SHAPES[0][0]]["clouds_per_s"] / best, 1)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
