#!/usr/bin/env python3
"""Generate tests/golden/g22_transforms.npz from the REFERENCE'S OWN seven transforms (datasets/data_transforms.py), on the CPU, with the import
shims of make_golden.py (its `.cuda()` shim included).  Build machine only: the reference never travels, only this data file is committed.

Every draw of the reference is recorded next to the output it produced: np.random.uniform (scale, shift, rotation), np.random.random (dropout),
random.random (flip) and Tensor.normal_ (jitter; the recorder draws the N(0,1) values, stores them and returns value * std + mean, which is what
normal_(mean, std) computes).  The flip's conditional draws are stored in three fixed slots (gate, first horizontal axis, second); a slot the
reference never drew holds 1.0.  The seeds are searched so that the file holds a cloud with the gate open and exactly one flipped axis, a
cloud with the gate closed, and a dropout cloud in which point 0 is itself dropped.

Run:  python tests/golden/make_golden_transforms.py
"""
import os
import random
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
from fill import clouds  # noqa: E402

B, N = 2, 128


class Recorder:
    """records what the four generators return while a transform runs"""

    def __enter__(self):
        self.log = {"uniform": [], "np_random": [], "py_random": [], "normal": []}
        self.real = (np.random.uniform, np.random.random, random.random, torch.Tensor.normal_)
        real_u, real_r, real_p, real_n = self.real
        log = self.log

        def uniform(*a, **k):
            v = real_u(*a, **k); log["uniform"].append(np.array(v, dtype=np.float64)); return v

        def np_random(*a, **k):
            v = real_r(*a, **k); log["np_random"].append(np.array(v, dtype=np.float64)); return v

        def py_random():
            v = real_p(); log["py_random"].append(v); return v

        def normal_(t, mean=0.0, std=1.0, **k):
            real_n(t, 0.0, 1.0, **k); log["normal"].append(t.clone().numpy()); return t.mul_(std).add_(mean)
        np.random.uniform, np.random.random, random.random, torch.Tensor.normal_ = uniform, np_random, py_random, normal_
        return self

    def __exit__(self, *exc):
        np.random.uniform, np.random.random, random.random, torch.Tensor.normal_ = self.real


def run(transform, pc, seed):
    np.random.seed(seed); random.seed(seed); torch.manual_seed(seed)
    with Recorder() as r:
        out = transform(torch.from_numpy(pc.copy()))
    return out.numpy(), r.log


def main():
    os.chdir(MG.REF)
    MG.install_shims()
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_dt", f"{MG.REF}/datasets/data_transforms.py")
    dt = importlib.util.module_from_spec(spec); spec.loader.exec_module(dt)
    pc = clouds(22, B, N)
    g = {"pc": pc}

    out, log = run(dt.PointcloudScale(), pc, 1)
    g["scale_out"], g["scale_scale"] = out, np.stack(log["uniform"]).astype(np.float32)
    out, log = run(dt.PointcloudTranslate(), pc, 2)
    g["translate_out"], g["translate_shift"] = out, np.stack(log["uniform"]).astype(np.float32)
    out, log = run(dt.PointcloudScaleAndTranslate(), pc, 3)
    g["st_out"], g["st_scale"], g["st_shift"] = out, np.stack(log["uniform"][0::2]).astype(np.float32), np.stack(log["uniform"][1::2]).astype(np.float32)
    out, log = run(dt.PointcloudRotate(), pc, 4)
    g["rotate_out"], g["rotate_u"] = out, np.array(log["uniform"], dtype=np.float64).reshape(B)
    out, log = run(dt.PointcloudJitter(), pc, 5)
    g["jitter_out"], g["jitter_noise"] = out, np.stack(log["normal"]).astype(np.float32)

    for seed in range(10000):                                  # a cloud in which point 0 is itself dropped
        out, log = run(dt.PointcloudRandomInputDropout(), pc, seed)
        ratio, drop_u = np.array(log["np_random"][0::2], dtype=np.float64).reshape(B), np.stack(log["np_random"][1::2])
        if (drop_u[:, 0] <= ratio * 0.5).any() and (drop_u[:, 0] > ratio * 0.5).any():
            break
    else:
        raise SystemExit("no dropout seed found")
    g["dropout_out"], g["dropout_ratio"], g["dropout_drop_u"], g["dropout_seed"] = out, ratio.astype(np.float32), drop_u.astype(np.float32), seed

    for seed in range(100000):                                 # one cloud with the gate open and one flipped axis, one with the gate closed
        random.seed(seed)
        u = np.ones((B, 3))
        for i in range(B):
            u[i, 0] = random.random()
            if u[i, 0] < 0.95:
                u[i, 1], u[i, 2] = random.random(), random.random()
        opened = (u[:, 0] < 0.95) & ((u[:, 1] < 0.5) != (u[:, 2] < 0.5))
        if opened.any() and (u[:, 0] >= 0.95).any():
            break
    else:
        raise SystemExit("no flip seed found")
    out, log = run(dt.RandomHorizontalFlip(), pc, seed)
    flat, u = list(log["py_random"]), np.ones((B, 3), dtype=np.float64)
    for i in range(B):                                         # the conditional draws, in the order the reference made them
        u[i, 0] = flat.pop(0)
        if u[i, 0] < 0.95:
            u[i, 1], u[i, 2] = flat.pop(0), flat.pop(0)
    assert not flat
    g["flip_out"], g["flip_u"], g["flip_seed"] = out, u.astype(np.float32), seed
    MG.save("g22_transforms", **g)


if __name__ == "__main__":
    main()
