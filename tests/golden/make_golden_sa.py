#!/usr/bin/env python3
"""Generates tests/golden/g25_sa.npz by importing the REFERENCE's part_segmentation/models/pointnet2_utils.py on the CPU.  Run in the build
container (needs the reference tree); the .npz is the committed fixture, this script is its provenance.

    python tests/golden/make_golden_sa.py

Recorded:
  (a) query_ball_point and sample_and_group on lattice clouds (coordinates multiples of 1/8: every squared distance is exact in float32 in
      the reference's expanded form and in the project's difference form, points exactly on the sphere included);
  (b) one PointNetSetAbstraction (B=2, N=96, npoint=16, r=0.5, nsample=8, D=5, mlp=[16,32]) and one PointNetSetAbstractionMsg (radii 0.5 / 0.75,
      nsample 4 / 8, mlp [[8,16],[16,32]]) in train mode with the weights of fill.py: outputs, running statistics, and the gradients of
      sum(out * cotangent) with respect to every parameter and to ``points``; then the eval-mode output with the updated running statistics;
  (c) a group_all layer and a points=None layer: outputs, running statistics and the eval-mode output only.  (The exact gradient of a conv bias
      ahead of a train-mode BatchNorm is zero; with points=None the reference's float32 value of it, 1e-4, is its own rounding noise and as
      large as the tests' bar -- its float64 run gives 1e-13 -- so that layer is no oracle for gradients.)
The FPS start is pinned to index 0 for every call by patching torch.randint.  Both modules also run in float64, and the file is written only if
every max-pool arg-max agrees between the float32 and float64 runs (SEED is chosen so that it does): the gradient comparison then needs no
allowance for flipped arg-maxes.
"""
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import save, REF                                      # noqa: E402
from fill import fill_module                                           # noqa: E402

SEED = 25
B, N, D, NPOINT = 2, 96, 5, 16
SA = dict(npoint=NPOINT, radius=0.5, nsample=8, in_channel=3 + D, mlp=[16, 32], group_all=False)
MSG = dict(npoint=NPOINT, radius_list=[0.5, 0.75], nsample_list=[4, 8], in_channel=D, mlp_list=[[8, 16], [16, 32]])
SA_ALL = dict(npoint=None, radius=None, nsample=None, in_channel=3 + D, mlp=[16, 32], group_all=True)
SA_XYZ = dict(npoint=NPOINT, radius=0.5, nsample=8, in_channel=3, mlp=[16, 32], group_all=False)
QUERIES = [(0.5, 8), (0.75, 5), (1.0, 64)]                           # (radius, nsample) of the recorded searches (the reference needs nsample <= N)


def lattice(rs, b, n, half):
    """coordinates: multiples of 1/8 in [-half, half]"""
    return (rs.randint(-8 * half, 8 * half + 1, size=(b, n, 3)) / 8.0).astype(np.float32)


def inputs(seed=SEED):
    rs = np.random.RandomState(seed)
    xyz = lattice(rs, B, N, 1)
    points = rs.standard_normal((B, N, D)).astype(np.float32)
    return xyz, points


class pinned_start:
    """torch.randint -> zeros: farthest_point_sample starts at index 0"""

    def __enter__(self):
        self.orig = torch.randint
        torch.randint = lambda low, high, size, **kw: torch.zeros(size, dtype=kw.get("dtype", torch.long))

    def __exit__(self, *exc):
        torch.randint = self.orig


class record_argmax:
    """torch.max(x, dim) -> records the indices of every call (the max-pool over the group)"""

    def __init__(self):
        self.args = []

    def __enter__(self):
        self.orig = torch.max

        def wrapped(*a, **kw):
            r = self.orig(*a, **kw)
            if len(a) == 2 and isinstance(a[1], int) and a[0].dim() == 4:
                self.args.append(r[1].clone())
            return r
        torch.max = wrapped
        return self

    def __exit__(self, *exc):
        torch.max = self.orig


def run(ref, cls, kw, prefix, xyz, points, cot, dtype):
    """train-mode forward + backward, then the eval-mode forward -> dict of arrays, list of arg-max tensors"""
    model = fill_module(cls(**kw), prefix).to(dtype).train()
    x = torch.from_numpy(xyz).to(dtype).transpose(1, 2)
    p = None if points is None else torch.from_numpy(points).to(dtype).transpose(1, 2).clone().requires_grad_(True)
    fps = ref.farthest_point_sample
    ref.farthest_point_sample = lambda c, n: fps(c.float(), n)          # its running distances are float32 (lattice coordinates: exact either way)
    try:
        with pinned_start(), record_argmax() as rec:
            new_xyz, out = model(x, p)
    finally:
        ref.farthest_point_sample = fps
    out_d = dict(new_xyz=new_xyz.detach(), out=out.detach())
    if cot is not None:
        (out * torch.from_numpy(cot).to(dtype)).sum().backward()
        for n, q in model.named_parameters():
            out_d["grad." + n] = q.grad
        if p is not None:
            out_d["grad_points"] = p.grad
    for n, bufr in model.named_buffers():
        if n.endswith("running_mean") or n.endswith("running_var"):
            out_d["buf." + n] = bufr.clone()
    model.eval()
    ref.farthest_point_sample = lambda c, n: fps(c.float(), n)
    try:
        with torch.no_grad(), pinned_start():
            out_d["out_eval"] = model(x, None if p is None else p.detach())[1]
    finally:
        ref.farthest_point_sample = fps
    return out_d, rec.args, model


def main():
    os.chdir(REF)
    sys.path.insert(0, os.path.join(REF, "part_segmentation", "models"))
    sys.modules.pop("pointnet2_utils", None)
    import pointnet2_utils as ref                                       # part_segmentation/models/pointnet2_utils.py
    torch.set_num_threads(8)
    out = dict(seed=np.int64(SEED))

    # (a) the search and the grouping on lattice clouds in [-2, 2] (sparse) and [-1, 1] (dense)
    rs = np.random.RandomState(SEED + 1000)
    for tag, half, n in (("wide", 2, 130), ("dense", 1, 96)):
        xyz = lattice(rs, 3, n, half)
        feat = rs.standard_normal((3, n, 4)).astype(np.float32)
        t = torch.from_numpy(xyz)
        with pinned_start():
            fps = ref.farthest_point_sample(t, 7)
        new_xyz = ref.index_points(t, fps)
        out[f"{tag}_xyz"], out[f"{tag}_feat"], out[f"{tag}_fps"], out[f"{tag}_new_xyz"] = xyz, feat, fps.to(torch.int32), new_xyz
        for qi, (r, ns) in enumerate(QUERIES):
            out[f"{tag}_idx{qi}"] = ref.query_ball_point(r, ns, t, new_xyz).to(torch.int32)
        with pinned_start():
            nx, npts = ref.sample_and_group(7, 0.5, 8, t, torch.from_numpy(feat))
        out[f"{tag}_sg_new_xyz"], out[f"{tag}_sg_new_points"] = nx, npts
    out["query_radius"] = np.array([q[0] for q in QUERIES], np.float64)
    out["query_nsample"] = np.array([q[1] for q in QUERIES], np.int64)

    # (b), (c) the modules
    xyz, points = inputs()
    out["xyz"], out["points"] = xyz, points
    with pinned_start():
        out["fps_idx"] = ref.farthest_point_sample(torch.from_numpy(xyz), NPOINT).to(torch.int32)
    rs = np.random.RandomState(SEED + 2000)
    for tag, cls, kw, pts, width, S in (("sa", ref.PointNetSetAbstraction, SA, points, 32, NPOINT),
                                        ("msg", ref.PointNetSetAbstractionMsg, MSG, points, 48, NPOINT),
                                        ("all", ref.PointNetSetAbstraction, SA_ALL, points, 32, 1),
                                        ("xyzonly", ref.PointNetSetAbstraction, SA_XYZ, None, 32, NPOINT)):
        cot = rs.standard_normal((B, width, S)).astype(np.float32) if tag in ("sa", "msg") else None
        r32, a32, model = run(ref, cls, kw, f"g25.{tag}.", xyz, pts, cot, torch.float32)
        r64, a64, _ = run(ref, cls, kw, f"g25.{tag}.", xyz, pts, cot, torch.float64)
        assert len(a32) == len(a64) > 0
        flips = sum(int((x != y).sum()) for x, y in zip(a32, a64))
        if flips:
            raise SystemExit(f"{tag}: {flips} max-pool arg-maxes differ between float32 and float64: choose another SEED")
        worst = max(float((r32[k].double() - r64[k]).abs().max()) for k in r32)
        print(f"[g25] {tag}: arg-maxes agree; max |float32 - float64| over all recorded tensors = {worst:.3e}")
        if cot is not None:
            out[f"{tag}_cot"] = cot
        for k, v in r32.items():
            out[f"{tag}.{k}"] = v
        sd = model.state_dict()
        out[f"{tag}_sd_keys"] = np.array(list(sd.keys()))
        out[f"{tag}_sd_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    save("g25_sa", **out)


if __name__ == "__main__":
    main()
