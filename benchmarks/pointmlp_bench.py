#!/usr/bin/env python3
"""PointMLP's two kernels (csrc/pointmlp.hip) and networks (models/pointmlp.py): one JSON line.

    python benchmarks/pointmlp_bench.py [--reps 10] [--commit ID] [--out FILE]        # FILE defaults to profiles/pointmlp_bench.json

Device-event medians (with min / max) of ``--reps`` repetitions after a warm-up:
  * K.geo_affine_group (cat=False, the form the network uses) forward and forward + backward at the four stage shapes of pointmlp at B = 32,
    (N -> S, k, D) = (1,024 -> 512, 24, 64), (512 -> 256, 24, 128), (256 -> 128, 24, 256), (128 -> 64, 24, 512), against the torch composition on
    the same device: indexing, torch.std over the cloud, the affine.  ``fwd_bytes_over_hbm_peak_ms`` is the forward's compulsory traffic (the rows
    written once, the table and the indices read once) over 8 TB/s, the figure notebook/pointmlp.md sets the measured time against;
  * K.batch_norm_add_relu forward + backward at 393,216 x 128 and 49,152 x 1,024 against K.batch_norm_act(relu=False) + add + relu;
  * one training step (forward, cross-entropy, backward) of pointmlp(40) and pointmlp_elite(40) at 32 x 1,024, FPS and kNN included.
Fused and composed forms are timed in one process, ALTERNATING repetition by repetition, on the same inputs; the worst difference of their outputs
is reported, not asserted.  The capability is new, so there is no earlier time of this project to compare with: ``--commit`` names the parent.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from benchmarks.dgcnn_seg_bench import timed_pair                # noqa: E402
from benchmarks.sa_bench import spread, timed                    # noqa: E402

GROUPER = [(32, 1024, 512, 24, 64), (32, 512, 256, 24, 128), (32, 256, 128, 24, 256), (32, 128, 64, 24, 512)]
TAIL = [(393216, 128), (49152, 1024)]
HBM_PEAK = 8.0e12


def _fwd(fn):
    def run():
        with torch.no_grad():
            fn()
    return run


def grouper(B, N, S, k, D, reps, K, dev):
    from act_amd.knn_cuda import knn_group
    from act_amd.pointnet2_ops import pointnet2_utils as pu
    g = torch.Generator(device="cpu").manual_seed(D + S)
    xyz = torch.rand(B, N, 3, generator=g).to(dev)
    fps = pu.furthest_point_sample(xyz, S, skip_near_origin=False)
    new_xyz = torch.gather(xyz, 1, fps.long().unsqueeze(-1).expand(B, S, 3)).contiguous()
    idx = knn_group(xyz, new_xyz, k)[0]
    feat = torch.randn(B, N, D, generator=g).to(dev).requires_grad_(True)
    alpha = (1 + 0.1 * torch.randn(D, generator=g)).to(dev).requires_grad_(True)
    beta = (0.1 * torch.randn(D, generator=g)).to(dev).requires_grad_(True)
    cot = torch.randn(B * S * k, D, generator=g).to(dev)
    batch = torch.arange(B, device=dev)
    fps64 = fps.long()

    def fused():
        return K.geo_affine_group(feat, fps, idx, alpha, beta, validate=False)

    def composed():
        e = feat[batch.view(B, 1, 1), idx] - feat[batch.view(B, 1), fps64].unsqueeze(2)
        std = torch.std(e.reshape(B, -1), dim=-1).view(B, 1, 1, 1)
        return (alpha * (e * (1.0 / (std + 1e-5))) + beta).reshape(B * S * k, D)

    def step(fn):
        def run():
            feat.grad = alpha.grad = beta.grad = None
            fn().backward(cot)
        return run

    with torch.no_grad():
        diff = float((fused() - composed()).abs().max())
    tf, tc = timed_pair(_fwd(fused), _fwd(composed), reps)
    sf, sc = timed_pair(step(fused), step(composed), reps)
    med = statistics.median
    rows = B * S * k
    model_ms = 4.0 * (rows * D + B * N * D + rows + B * S) / HBM_PEAK * 1e3
    return {"B": B, "N": N, "S": S, "k": k, "D": D, "fused_fwd_ms": spread(tf), "composed_fwd_ms": spread(tc), "fused_fwd_bwd_ms": spread(sf),
            "composed_fwd_bwd_ms": spread(sc), "composed_over_fused_fwd": round(med(tc) / med(tf), 2),
            "composed_over_fused_fwd_bwd": round(med(sc) / med(sf), 2), "max_abs_difference_of_the_outputs": float("%.3g" % diff),
            "fwd_bytes_over_hbm_peak_ms": float("%.4g" % model_ms), "fwd_over_byte_model": round(med(tf) / model_ms, 2)}


def tail(R, C, reps, K, dev):
    g = torch.Generator(device="cpu").manual_seed(C)
    y = torch.randn(R, C, generator=g).to(dev).requires_grad_(True)
    res = torch.randn(R, C, generator=g).to(dev).requires_grad_(True)
    cot = torch.randn(R, C, generator=g).to(dev)
    bns = [torch.nn.BatchNorm1d(C).to(dev).train(), torch.nn.BatchNorm1d(C).to(dev).train()]

    def fused():
        return K.batch_norm_add_relu(y, res, bns[0], True)

    def composed():
        return torch.relu(K.batch_norm_act(y, bns[1], True, relu=False) + res)

    def step(fn):
        def run():
            y.grad = res.grad = None
            for bn in bns:
                bn.zero_grad(set_to_none=True)
            fn().backward(cot)
        return run

    with torch.no_grad():
        diff = float((fused() - composed()).abs().max())
    sf, sc = timed_pair(step(fused), step(composed), reps)
    med = statistics.median
    return {"R": R, "C": C, "fused_fwd_bwd_ms": spread(sf), "composed_fwd_bwd_ms": spread(sc),
            "composed_over_fused_fwd_bwd": round(med(sc) / med(sf), 2), "max_abs_difference_of_the_outputs": float("%.3g" % diff)}


def network(make, reps, K, dev):
    B, N, classes = 32, 1024, 40
    g = torch.Generator(device="cpu").manual_seed(0)
    net = make(classes).to(dev).train()
    pts = torch.rand(B, N, 3, generator=g).to(dev)
    lab = torch.randint(0, classes, (B,), generator=g).to(dev)

    def step():
        net.zero_grad(set_to_none=True)
        K.softmax_xent(net(pts), lab)[0].backward()
    return {"B": B, "N": N, "parameters": sum(p.numel() for p in net.parameters()), "step_ms": spread(timed(step, reps), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "pointmlp_bench.json"))
    ap.add_argument("--commit", type=str, default=os.environ.get("ACT_BENCH_COMMIT"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointmlp_bench needs a GPU: there is nothing to time without one")
    from act_amd import kernels as K
    from act_amd.models import pointmlp as M
    dev = torch.device("cuda:0")
    res = {"workload": "pointmlp", "parent_commit": args.commit, "reps": args.reps,
           "geo_affine_group": [grouper(*s, args.reps, K, dev) for s in GROUPER],
           "batch_norm_add_relu": [tail(*s, args.reps, K, dev) for s in TAIL],
           "pointmlp_step": network(M.pointmlp, args.reps, K, dev),
           "pointmlp_elite_step": network(M.pointmlp_elite, args.reps, K, dev)}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
