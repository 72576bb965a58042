#!/usr/bin/env python3
"""Three-NN feature propagation and the three PointNet++ networks (csrc/sa.hip, models/pointnet2.py, models/pointnet2_nets.py):
one JSON line.

    python benchmarks/fp_bench.py [--reps 10] [--commit ID] [--out FILE]        # FILE defaults to profiles/fp_bench.json

Clouds uniform in the unit ball, the known points by FPS.  Device-event medians (with min / max) of ``--reps`` repetitions after a warm-up:
  * the search (K.three_nn, without and with the adjacency) at 32 x 2,048 <- 512, 32 x 4,096 <- 1,024 and 16 x 8,192 <- 2,048, against the
    torch formulation of the same search on the same device (pairwise difference-form distances, a full sort, the first three) -- the index
    sets agree;
  * one PointNetFeaturePropagationAny layer (32 x 2,048 <- 512, D1 = 128, D2 = 256, mlp [256, 128]) forward + backward;
  * one training step (forward, loss, backward) of each network at its published sizes: the classifier on 32 x 1,024 points, the part
    segmentation network on 16 x 2,048, the semantic segmentation network on 16 x 4,096 x 9 channels.

Rate.  A distance test is one (unknown, known) distance and its insertion compare.  ``tests_per_s`` is B * n * m over the search time;
notebook/fp.md sets it against the vector-issue model of the ball query (notebook/sa.md).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from benchmarks.sa_bench import spread, timed, ball                    # noqa: E402

SEARCH_SHAPES = [(32, 2048, 512), (32, 4096, 1024), (16, 8192, 2048)]


def torch_sort_search(u, k):
    d = u[:, :, None, :] - k[:, None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d3, idx = d2.sort(dim=-1)
    return d3[:, :, :3], idx[:, :, :3]


def clouds(B, n, m, pu, dev):
    rs = np.random.RandomState(n + m)
    u = torch.from_numpy(ball(rs, B, n)).to(dev)
    _, k = pu.furthest_point_sample_with_centers(u, m, skip_near_origin=False)
    return u, k


def search(B, n, m, reps, K, pu, dev):
    u, k = clouds(B, n, m, pu, dev)
    idx = K.three_nn(u, k, want_adj=False)[0]
    same = bool(torch.equal(idx.long().sort(-1)[0], torch_sort_search(u, k)[1].sort(-1)[0]))
    t = timed(lambda: K.three_nn(u, k, want_adj=False), reps)
    t_adj = timed(lambda: K.three_nn(u, k), reps)
    t_sort = timed(lambda: torch_sort_search(u, k), max(2, reps // 3))
    per_s = B * n * m / (statistics.median(t) * 1e-3)
    return {"B": B, "n": n, "m": m, "three_nn_ms": spread(t), "with_adjacency_ms": spread(t_adj), "torch_sort_ms": spread(t_sort, 3),
            "same_index_sets_as_torch": same, "speedup_over_torch_sort": round(statistics.median(t_sort) / statistics.median(t), 1),
            "tests_per_s": float("%.4g" % per_s)}


def fp_layer(reps, P, pu, dev):
    B, n, m, D1, D2 = 32, 2048, 512, 128, 256
    u, k = clouds(B, n, m, pu, dev)
    layer = P.PointNetFeaturePropagationAny(D1 + D2, [256, 128]).to(dev).train()
    x1, x2 = u.transpose(1, 2).contiguous(), k.transpose(1, 2).contiguous()
    p1 = torch.randn(B, D1, n, device=dev, requires_grad=True)
    p2 = torch.randn(B, D2, m, device=dev, requires_grad=True)

    def step():
        layer.zero_grad(set_to_none=True)
        p1.grad = p2.grad = None
        layer(x1, x2, p1, p2).square().mean().backward()
    return {"B": B, "N": n, "S": m, "D1": D1, "D2": D2, "mlp": [256, 128], "fwd_bwd_ms": spread(timed(step, reps), 3)}


def network_steps(reps, K, M, dev):
    from act_amd.models import partseg, semseg
    rs = np.random.RandomState(0)
    out = {}
    cls = M.pointnet2_cls_ssg(40).to(dev).train()
    pts = torch.from_numpy(ball(rs, 32, 1024)).to(dev)
    lab = torch.randint(0, 40, (32,), device=dev)

    def cls_step():
        cls.zero_grad(set_to_none=True)
        K.softmax_xent(cls(pts), lab)[0].backward()
    out["pointnet2_cls_ssg"] = {"B": 32, "N": 1024, "step_ms": spread(timed(cls_step, reps), 3)}
    part = M.pointnet2_part_seg_msg(50).to(dev).train()
    ppts = torch.from_numpy(ball(rs, 16, 2048)).to(dev).transpose(1, 2).contiguous()
    onehot = partseg.to_categorical(torch.randint(0, 16, (16,), device=dev), 16)
    ptgt = torch.randint(0, 50, (16 * 2048,), device=dev)
    pcrit = partseg.get_loss()

    def part_step():
        part.zero_grad(set_to_none=True)
        pcrit(part(ppts, onehot), ptgt).backward()
    out["pointnet2_part_seg_msg"] = {"B": 16, "N": 2048, "step_ms": spread(timed(part_step, reps), 3)}
    sem = M.pointnet2_sem_seg(13).to(dev).train()
    spts = torch.cat((torch.from_numpy(ball(rs, 16, 4096)).to(dev), torch.rand(16, 4096, 6, device=dev)), dim=-1).transpose(1, 2).contiguous()
    stgt = torch.randint(0, 13, (16 * 4096,), device=dev)
    scrit = semseg.get_loss()

    def sem_step():
        sem.zero_grad(set_to_none=True)
        scrit(sem(spts), stgt).backward()
    out["pointnet2_sem_seg"] = {"B": 16, "N": 4096, "channels": 9, "step_ms": spread(timed(sem_step, reps), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "fp_bench.json"))
    ap.add_argument("--commit", type=str, default=os.environ.get("ACT_BENCH_COMMIT"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fp_bench needs a GPU: there is nothing to time without one")
    from act_amd import kernels as K
    from act_amd.pointnet2_ops import pointnet2_utils as pu
    from act_amd.models import pointnet2 as P, pointnet2_nets as M
    dev = torch.device("cuda:0")
    res = {"workload": "feature_propagation", "commit": args.commit, "reps": args.reps,
           "search": [search(*shape, args.reps, K, pu, dev) for shape in SEARCH_SHAPES],
           "fp_layer": fp_layer(args.reps, P, pu, dev),
           "networks": network_steps(args.reps, K, M, dev)}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
