#!/usr/bin/env python3
"""Stage-I reconstruction evaluation (tools/runner_autoencoder.py evaluate, csrc/recon_eval.hip): one JSON line.

    python benchmarks/recon_eval_bench.py [--samples 128] [--batch 32] [--reps 5] [--commit ID] [--out profiles/recon_eval_bench.json]

Reports (a) the device time of one ``kernels.recon_eval`` launch at B = 1, 32, 128, 256 with the Stage-I sizes (coarse 512, dense 2048, gt 1024)
and the distance evaluations per second it achieves (2 * N * (nd + nc) per cloud), and (b) the wall time per cloud of a whole ``evaluate``
pass at the given batch size against a reference-form pass written here: batch size 1, the six ``ChamferDistance*`` module calls of the
reference's validate + Metrics, an ``.item()`` read after each, and the F-Score on the host through ``scipy.spatial.cKDTree`` (standing in for
open3d's KD-tree).  Both passes run the full-size synthetic Stage-I model (cfgs/synthetic/act_dvae_with_pretrained_transformer.yaml, random
weights) over the same synthetic clouds with the same gumbel noise.  Kernel times are device events around ``inner`` back-to-back launches;
pass times are wall clock ending in a synchronise; every figure is the median of ``--reps`` repetitions after a warm-up, with min / max.
"""
import argparse
import json
import logging
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NC, ND, N = 512, 2048, 1024


def spread(vals, digits=4):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def kernel_times(dev, reps, inner=20):
    from act_amd import kernels as K
    out = {}
    g = torch.Generator(device="cpu").manual_seed(0)
    for B in (1, 32, 128, 256):
        gt = torch.randn(B, N, 3, generator=g)
        gt = (gt / gt.norm(dim=2).amax(dim=1)[:, None, None]).to(dev)
        dense = torch.cat([gt, gt], dim=1) + 0.004 * torch.randn(B, ND, 3, generator=g).to(dev)
        coarse = gt[:, :NC] + 0.004 * torch.randn(B, NC, 3, generator=g).to(dev)
        rows = torch.zeros(B, K.RECON_FIELDS, dtype=torch.float64, device=dev)
        for _ in range(5):
            K.recon_eval(coarse, dense, gt, rows, 0)
        torch.cuda.synchronize()
        us = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                K.recon_eval(coarse, dense, gt, rows, 0)
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) / inner * 1e3)
        evals = 2.0 * B * N * (ND + NC)
        med = statistics.median(us)
        out[f"B{B}"] = {"us": spread(us, 2), "us_per_cloud": round(med / B, 2), "distance_evals": int(evals),
                        "Gevals_per_s": round(evals / med * 1e-3, 1), "f_score_mean": round(float(rows[:, K.RECON_FSCORE].mean()), 4)}
    return out


def reference_form_pass(model, loader, dev, seed=0):
    """the reference's validate loop (runner_autoencoder.py:219-283) in its own form: one cloud at a time, six Chamfer module calls with an
    .item() after each, the F-Score from host KD-tree queries"""
    from scipy.spatial import cKDTree
    from act_amd.extensions.chamfer_dist import ChamferDistanceL1, ChamferDistanceL2
    from act_amd.tools.runner_autoencoder import gumbel_noise
    from act_amd.utils.draws import Draws
    l1, l2, z1, z2 = ChamferDistanceL1(), ChamferDistanceL2(), ChamferDistanceL1(ignore_zeros=True), ChamferDistanceL2(ignore_zeros=True)
    losses, per = np.zeros(4), {}
    n = 0
    with torch.no_grad():
        for idx, (tax, _, data) in enumerate(loader):
            points = data.to(dev)
            ret = model(points, temperature=1., hard=True, draws=Draws({"gumbel": gumbel_noise(model, [idx], seed, dev)}))
            coarse, dense = ret[0], ret[1]
            losses += [l1(coarse, points).item() * 1000, l2(coarse, points).item() * 1000, l1(dense, points).item() * 1000,
                       l2(dense, points).item() * 1000]
            cd1, cd2 = z1(dense, points).item() * 1000, z2(dense, points).item() * 1000
            p, q = dense.squeeze().cpu().numpy().astype(np.float64), points.squeeze().cpu().numpy().astype(np.float64)
            d1, _ = cKDTree(q).query(p, k=1)
            d2, _ = cKDTree(p).query(q, k=1)
            recall, precision = float(sum(d < 0.01 for d in d2)) / len(d2), float(sum(d < 0.01 for d in d1)) / len(d1)
            f = 2 * recall * precision / (recall + precision) if recall + precision else 0
            per.setdefault(tax[0], []).append([f, cd1, cd2])
            n += 1
    torch.cuda.synchronize()
    overall = np.mean([np.mean(v, axis=0) for v in per.values()], axis=0)
    return list(losses / n), [float(v) for v in overall]


def passes(dev, samples, batch, reps):
    from act_amd.models import build_model_from_cfg
    from act_amd.tools import builder
    from act_amd.tools import runner_autoencoder as RA
    from act_amd.utils.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file("cfgs/synthetic/act_dvae_with_pretrained_transformer.yaml")
    cfg.dataset.test._base_.NUM_SAMPLES = samples
    cfg.dataset.test._base_.NUM_TAXONOMIES = 4
    cfg.dataset.test.others.bs = batch
    args = argparse.Namespace(log_name="recon_eval_bench", use_gpu=True, local_rank=0, distributed=False, num_workers=0)
    torch.manual_seed(0)
    model = build_model_from_cfg(cfg.model).to(dev).eval()
    _, loader = builder.dataset_builder(args, cfg.dataset.test)
    one = torch.utils.data.DataLoader(loader.dataset, batch_size=1, shuffle=False)
    m = RA.evaluate(model, loader, 0, args, cfg)                                      # warm-up of both sides (first-use GEMM tuning, allocator)
    ref_losses, ref_overall = reference_form_pass(model, one, dev)
    t_eval, t_ref = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = RA.evaluate(model, loader, 0, args, cfg)
        torch.cuda.synchronize()
        t_eval.append((time.perf_counter() - t0) / samples * 1e3)
        t0 = time.perf_counter()
        ref_losses, ref_overall = reference_form_pass(model, one, dev)
        t_ref.append((time.perf_counter() - t0) / samples * 1e3)
    e, r = spread(t_eval), spread(t_ref)
    return {"model": "ACTPromptedDiscreteVAEwithVIT (synthetic cfg, random weights)", "samples": samples, "evaluate_batch": batch,
            "evaluate_ms_per_cloud": e, "reference_form_ms_per_cloud": r, "speedup_median": round(r["median"] / e["median"], 2),
            "evaluate_not_slower_beyond_spread": bool(e["min"] <= r["max"]),
            "evaluate_overall": [round(v, 4) for v in m.state_dict().values()], "reference_form_overall": [round(v, 4) for v in ref_overall],
            "evaluate_losses": [round(v, 4) for v in m.losses], "reference_form_losses": [round(float(v), 4) for v in ref_losses]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--commit", type=str, default=os.environ.get("ACT_BENCH_COMMIT"),
                    help="commit the figures are measured at (default: $ACT_BENCH_COMMIT, else git rev-parse of the checkout)")
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from act_amd.utils.logger import get_logger
    get_logger("recon_eval_bench").setLevel(logging.ERROR)
    dev = torch.device("cuda:0")
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    out = {"workload": "stage1_recon_eval", "sizes": {"coarse": NC, "dense": ND, "gt": N}, "commit": commit, "reps": args.reps,
           "kernel": kernel_times(dev, args.reps), "pass": passes(dev, args.samples, args.batch, args.reps)}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
