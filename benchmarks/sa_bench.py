#!/usr/bin/env python3
"""PointNet++ set abstraction (models/pointnet2.py, csrc/sa.hip): one JSON line.

    python benchmarks/sa_bench.py [--reps 10] [--commit ID] [--out profiles/sa_bench.json]

Clouds uniform in the unit ball, centres by FPS.  Per shape -- 32 x 2048 -> 512 (r 0.2, nsample 32) and 32 x 8192 -> 1024 (r 0.1, nsample 32):
the device time (device-event medians of ``--reps`` repetitions after a warm-up, with min / max) of
  * the ball query (inclusive rule), and of the sort-based torch formulation of the same search on the same device (written here: pairwise
    difference-form distances, indices outside the radius set to N, sort, keep nsample, pad with the first) -- both give the same indices;
  * grouped rows forward and backward at D = 64;
  * one set-abstraction layer (in 3 + 64, mlp [64, 64, 128]) forward + backward.
The capability is new, so there is no earlier time of this project to compare with.

Rates.  A hit test is one (query, point) distance and compare.  The vector-issue model (notebook/sa.md): the walk issues 12 vector instructions
per 64 hit tests (counted in the gfx950 code of a step without a hit), a wave64 instruction occupies its SIMD for 2 cycles, and the chip has
256 compute units x 4 SIMDs, so it can do at most 1024 * 64 / (12 * 2) = 2731 hit tests per cycle, 6.55e12 per second at 2.4 GHz.
``hit_tests`` counts the points the kernel really walks
(a wave leaves once nsample hits are out; counted on the host from cnt and the index of the last hit), ``share_of_issue_model`` is hit tests
per second over the model.
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

CLOCK_HZ, CUS, SIMDS, WALK_VALU_PER_64, CYCLES_PER_WAVE_OP = 2.4e9, 256, 4, 12, 2
MODEL_TESTS_PER_S = CUS * SIMDS * 64 / (WALK_VALU_PER_64 * CYCLES_PER_WAVE_OP) * CLOCK_HZ
SHAPES = [(32, 2048, 512, 0.2, 32), (32, 8192, 1024, 0.1, 32)]
D = 64


def spread(vals, digits=4):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def ball(rs, B, N):
    x = rs.standard_normal((B, N, 3))
    x *= (rs.rand(B, N, 1) ** (1.0 / 3.0)) / np.linalg.norm(x, axis=2, keepdims=True)
    return x.astype(np.float32)


def torch_sort_query(xyz, new_xyz, radius, nsample):
    """the reference's formulation with the project's distance: [B,S,N] distances, a full sort per query"""
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    d = new_xyz[:, :, None, :] - xyz[:, None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    idx = torch.arange(N, device=xyz.device).view(1, 1, N).repeat(B, S, 1)
    idx[d2 > radius * radius] = N
    idx = idx.sort(dim=-1)[0][:, :, :nsample]
    first = idx[:, :, :1].expand(-1, -1, nsample)
    return torch.where(idx == N, first, idx)


def one(B, N, S, radius, ns, reps, K, pu, P):
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(N)
    xyz = torch.from_numpy(ball(rs, B, N)).to(dev)
    feat = torch.from_numpy(rs.standard_normal((B, N, D)).astype(np.float32)).to(dev)
    _, new_xyz = pu.furthest_point_sample_with_centers(xyz, S, skip_near_origin=False)
    idx, cnt = K.ball_query(xyz, new_xyz, radius, ns, inclusive=True, want_cnt=True)
    ref_idx = torch_sort_query(xyz, new_xyz, np.float32(radius).item(), ns)
    same = bool(torch.equal(ref_idx.to(torch.int32), idx))
    # points walked: the whole cloud unless nsample hits came out, then up to the 64-point step that holds the last kept index
    last = idx.max(dim=-1)[0].long()
    walked = torch.where(cnt >= ns, (last // 64 + 1) * 64, torch.full_like(last, N)).clamp(max=N)
    tests = float(walked.sum().item())
    t_bq = timed(lambda: K.ball_query(xyz, new_xyz, radius, ns, inclusive=True), reps)
    t_sort = timed(lambda: torch_sort_query(xyz, new_xyz, np.float32(radius).item(), ns), max(2, reps // 3))
    t_fwd = timed(lambda: K.group_rows(xyz, new_xyz, feat, idx), reps)
    f = feat.clone().requires_grad_(True)
    rows = K.group_rows(xyz, new_xyz, f, idx)
    cot = torch.randn_like(rows)
    t_bwd = timed(lambda: torch.autograd.grad(rows, f, cot, retain_graph=True), reps)
    layer = P.PointNetSetAbstraction(S, radius, ns, 3 + D, [64, 64, 128], False).to(dev).train()
    xyz_t, pts_t = xyz.transpose(1, 2).contiguous(), feat.transpose(1, 2).contiguous().requires_grad_(True)

    def step():
        layer.zero_grad(set_to_none=True)
        pts_t.grad = None
        layer(xyz_t, pts_t)[1].square().mean().backward()
    t_layer = timed(step, reps)
    per_s = tests / (statistics.median(t_bq) * 1e-3)
    return {"B": B, "N": N, "S": S, "radius": radius, "nsample": ns, "D": D,
            "mean_hits": round(float(cnt.float().mean().item()), 2), "full_rows": round(float((cnt >= ns).float().mean().item()), 4),
            "ball_query_ms": spread(t_bq), "torch_sort_query_ms": spread(t_sort, 3), "same_indices_as_torch": same,
            "speedup_over_torch_sort": round(statistics.median(t_sort) / statistics.median(t_bq), 1),
            "hit_tests": tests, "hit_tests_per_s": float("%.4g" % per_s), "share_of_issue_model": round(per_s / MODEL_TESTS_PER_S, 4),
            "group_rows_fwd_ms": spread(t_fwd), "group_rows_bwd_ms": spread(t_bwd), "sa_layer_fwd_bwd_ms": spread(t_layer, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--commit", type=str, default=os.environ.get("ACT_BENCH_COMMIT"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sa_bench needs a GPU: there is nothing to time without one")
    from act_amd import kernels as K
    from act_amd.pointnet2_ops import pointnet2_utils as pu
    from act_amd.models import pointnet2 as P
    res = {"workload": "set_abstraction", "commit": args.commit, "reps": args.reps,
           "issue_model_hit_tests_per_s": float("%.4g" % MODEL_TESTS_PER_S),
           "runs": [one(*shape, args.reps, K, pu, P) for shape in SHAPES]}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
