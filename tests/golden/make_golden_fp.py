#!/usr/bin/env python3
"""Generates tests/golden/g26_fp.npz by importing the REFERENCE's part_segmentation/models/pointnet2_utils.py on the CPU.  Run in the build
container (needs the reference tree); the .npz is the committed fixture, this script is its provenance.

    python tests/golden/make_golden_fp.py

Recorded: the reference's PointNetFeaturePropagation in train mode with the weights of fill.py on 1/8-lattice clouds (every squared distance
exact in float32, in the reference's expanded form and in the project's difference form; coordinates in [-4, 4]), B = 2, N = 96:

    s16    S = 16 with points1 (D1 = 5, D2 = 7, mlp [16, 32])
    s16np  S = 16 with points1 = None
    s2     S = 2
    s1     S = 1

per case the output, the running statistics, the gradients of sum(out * cotangent) with respect to every parameter, ``points1`` and
``points2``, and the eval-mode output afterwards.

S = 2: the reference's forward keeps two sorted columns, normalises the two weights and then calls ``weight.view(B, N, 3, 1)``, which raises on
a two-column tensor; the network definitions never reach that line (their coarsest level has 1, 16 or 128 points).  The S = 2 case is therefore
recorded from the reference's own forward with that one view widened to ``view(B, N, -1, 1)`` (``two_column_view`` below patches Tensor.view
for the duration of the call).

The file is not written if any point has equal third and fourth nearest distances: torch.sort fixes no order among equal keys, so the
reference's choice there is not a rule.  (Ties inside the first three only reorder a sum.)
"""
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import save, REF                                      # noqa: E402
from fill import fill_module                                           # noqa: E402

SEED = 26
B, N, D1, D2 = 2, 96, 5, 7
MLP = [16, 32]
HALF = 4                        # coordinates in [-4, 4]: squared distances are integers / 64 up to 12,288, sparse enough for tie-free clouds
CASES = {"s16": (16, True), "s16np": (16, False), "s2": (2, True), "s1": (1, True)}       # tag -> (S, with points1)


def lattice(rs, b, n, half=HALF):
    return (rs.randint(-8 * half, 8 * half + 1, size=(b, n, 3)) / 8.0).astype(np.float32)


def inputs(tag):
    """-> xyz1 [B,N,3], xyz2 [B,S,3], points1 [B,N,D1] or None, points2 [B,S,D2], cotangent [B,MLP[-1],N]; the seed search keeps the third and
    fourth nearest distances of every point apart"""
    S, with_p1 = CASES[tag]
    for attempt in range(1000):
        rs = np.random.RandomState(SEED * 1000 + 100 * list(CASES).index(tag) + attempt)
        xyz1, xyz2 = lattice(rs, B, N), lattice(rs, B, S)
        if S > 3:
            d = np.sort(((xyz1[:, :, None, :] - xyz2[:, None, :, :]) ** 2).sum(-1), axis=-1)
            if (d[..., 2] == d[..., 3]).any():
                continue
        p1 = rs.standard_normal((B, N, D1)).astype(np.float32) if with_p1 else None
        p2 = rs.standard_normal((B, S, D2)).astype(np.float32)
        cot = rs.standard_normal((B, MLP[-1], N)).astype(np.float32)
        return xyz1, xyz2, p1, p2, cot
    raise SystemExit(f"{tag}: no cloud without a third/fourth tie in 1000 draws")


class two_column_view:
    """Tensor.view(B, N, 3, 1) of a tensor that does not hold B * N * 3 elements -> view(B, N, -1, 1): lets the reference's own forward run at
    S == 2 (in the manner of make_golden_sa.py's pinned_start)"""

    def __enter__(self):
        orig = self.orig = torch.Tensor.view

        def view(t, *shape):
            if len(shape) == 4 and shape[2] == 3 and shape[3] == 1 and t.numel() != shape[0] * shape[1] * 3:
                return orig(t, shape[0], shape[1], -1, 1)
            return orig(t, *shape)
        torch.Tensor.view = view

    def __exit__(self, *exc):
        torch.Tensor.view = self.orig


def call_s2(model, *args):
    with two_column_view():
        return model(*args)


def run(ref, tag, dtype):
    S, with_p1 = CASES[tag]
    xyz1, xyz2, p1, p2, cot = inputs(tag)
    model = fill_module(ref.PointNetFeaturePropagation((D1 if with_p1 else 0) + D2, MLP), f"g26.{tag}.").to(dtype).train()
    t = lambda a: torch.from_numpy(a).to(dtype).transpose(1, 2)
    x1, x2 = t(xyz1), t(xyz2)
    q1 = None if p1 is None else t(p1).clone().requires_grad_(True)
    q2 = t(p2).clone().requires_grad_(True)
    call = (lambda *a: call_s2(model, *a)) if S == 2 else model
    out = call(x1, x2, q1, q2)
    (out * torch.from_numpy(cot).to(dtype)).sum().backward()
    rec = dict(out=out.detach(), grad_points2=q2.grad)
    if q1 is not None:
        rec["grad_points1"] = q1.grad
    for n, q in model.named_parameters():
        rec["grad." + n] = q.grad
    for n, bufr in model.named_buffers():
        if n.endswith("running_mean") or n.endswith("running_var"):
            rec["buf." + n] = bufr.clone()
    model.eval()
    with torch.no_grad():
        rec["out_eval"] = call(x1, x2, None if q1 is None else q1.detach(), q2.detach())
    return rec, model, dict(xyz1=xyz1, xyz2=xyz2, points2=p2, cot=cot, **({} if p1 is None else dict(points1=p1)))


def main():
    os.chdir(REF)
    sys.path.insert(0, os.path.join(REF, "part_segmentation", "models"))
    sys.modules.pop("pointnet2_utils", None)
    import pointnet2_utils as ref                                       # part_segmentation/models/pointnet2_utils.py
    torch.set_num_threads(8)
    out = dict(seed=np.int64(SEED))
    for tag in CASES:
        r32, model, inp = run(ref, tag, torch.float32)
        r64, _, _ = run(ref, tag, torch.float64)
        worst = max(float((r32[k].double() - r64[k]).abs().max()) for k in r32)
        print(f"[g26] {tag}: max |float32 - float64| over all recorded tensors = {worst:.3e}")
        for k, v in inp.items():
            out[f"{tag}_{k}"] = v
        for k, v in r32.items():
            out[f"{tag}.{k}"] = v
        sd = model.state_dict()
        out[f"{tag}_sd_keys"] = np.array(list(sd.keys()))
        out[f"{tag}_sd_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    save("g26_fp", **out)


if __name__ == "__main__":
    main()
