#!/usr/bin/env python3
"""Generates tests/golden/g20_wholescene.npz by running the REFERENCE's whole-room test (semantic_segmentation/main_test.py main() with
dataset.py ScannetDatasetWholeScene) under the shims of make_golden.py.  Run in the build container (needs the reference tree); the .npz is the
committed fixture, this script is its provenance.

    python tests/golden/make_golden_wholescene.py

Two small rooms (3 m x 3.2 m, 2000 points; one float32 file, one float64 file) with points exactly on, and one ulp either side of, interior
block thresholds, written as Area_5_*.npy to a temporary directory.  main() runs with block_points = 256, batch size 4, one vote, under
np.random.seed(SEED), with a stand-in model module whose log-probs are a fixed seeded function of each row's float32 input (xyz . W), so the
vote pool depends on the rows alone.  ``Tensor.cuda`` / ``Module.cuda`` are identities (CPU only) and ``np.float`` is ``float`` (main_test.py
predates NumPy 1.24).  Recorded per room (in the reference's file order): the room file, index_room (int32), data_room[:, :, :3] (float32), the
sample weights, the vote pool add_vote built; and labelweights, the printed metric lines, parse_args() defaults, np.__version__.
"""
import contextlib
import io
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import install_shims, save, REF                      # noqa: E402

SEED, BLOCK_POINTS, BATCH, NPTS = 20, 256, 4, 2000
W_SEED = 2020


def room(rs, dtype, W=3.0, D=3.2, H=2.8):
    """xyzrgbl [NPTS, 7]: corners pin coord_min / coord_max; labels over 12 of the 13 classes (class 11 absent: an infinite labelweight)"""
    xyz = rs.uniform([0, 0, 0], [W, D, H], size=(NPTS, 3)).astype(dtype)
    xyz[0] = (0, 0, 0)
    xyz[1] = (W, D, H)
    cmin, cmax = xyz.min(0), xyz.max(0)
    # interior thresholds, formed as dataset.py forms them (the file's dtype), and points on / one ulp either side of them
    k = 2
    for axis, extent in ((0, cmax[0] - cmin[0]), (1, cmax[1] - cmin[1])):
        grid = int(np.ceil(float(extent - 1.0) / 0.5) + 1)
        for i in range(1, grid - 1):
            s = cmin[axis] + i * 0.5
            e = min(s + 1.0, cmax[axis])
            s = e - 1.0
            for t in (s - 0.001, e + 0.001):
                if not (cmin[axis] < t < cmax[axis]):
                    continue
                for v in (np.nextafter(t, -np.inf), t, np.nextafter(t, np.inf)):
                    xyz[k, axis] = v
                    k += 1
    lab = rs.randint(0, 12, size=NPTS)
    lab[lab == 11] = 12
    rgb = rs.randint(0, 256, size=(NPTS, 3)).astype(dtype)
    return np.concatenate([xyz, rgb, lab[:, None].astype(dtype)], axis=1), k - 2


def main():
    os.chdir(REF)
    install_shims()
    sys.path.insert(0, os.path.join(REF, "semantic_segmentation"))
    for name in ("dataset", "main_test", "pointnet_util"):
        sys.modules.pop(name, None)
    if not hasattr(np, "float"):
        np.float = float
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    import main_test as ref                                             # semantic_segmentation/main_test.py (cwd: the reference root)

    W = torch.from_numpy(np.random.RandomState(W_SEED).standard_normal((3, 13)).astype(np.float32))

    class FakeModel(torch.nn.Module):
        def forward(self, x):                                           # [B, 3, N] -> log-probs [B, N, 13]
            return torch.log_softmax(x.transpose(2, 1) @ W, dim=-1)

        def load_model_from_ckpt_withrename(self, path):
            return None

    sys.modules["wholescene_fake_model"] = types.SimpleNamespace(get_model=lambda n: FakeModel())

    rs = np.random.RandomState(SEED)
    rooms = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "rooms") + "/"
        os.makedirs(root)
        for tag, dtype in (("f32", np.float32), ("f64", np.float64)):
            rooms[tag], nedge = room(rs, dtype)
            np.save(root + "Area_5_room_%s.npy" % tag, rooms[tag])
            print(tag, "threshold points", nedge)

        got = {"items": [], "pools": []}
        orig_get = ref.ScannetDatasetWholeScene.__getitem__
        orig_vote = ref.add_vote

        def get(self, index):
            out = orig_get(self, index)
            got["items"].append((index, out))
            return out

        def vote(pool, idx, pred, w):
            pool = orig_vote(pool, idx, pred, w)
            got["pools"].append(pool)
            return pool
        ref.ScannetDatasetWholeScene.__getitem__ = get
        ref.add_vote = vote
        cwd = os.path.join(tmp, "run")
        os.makedirs(os.path.join(cwd, "log", "semantic_seg", "g20"))
        argv = ["main_test.py", "--model", "wholescene_fake_model", "--log_dir", "g20", "--root", root, "--num_point", str(BLOCK_POINTS),
                "--batch_size", str(BATCH), "--num_votes", "1", "--test_area", "5"]
        sys.argv = argv
        np.random.seed(SEED)
        buf = io.StringIO()
        os.chdir(cwd)
        try:
            with contextlib.redirect_stdout(buf):
                ref.main(ref.parse_args())
        finally:
            os.chdir(REF)
        printed = buf.getvalue()
        ds = ref.ScannetDatasetWholeScene(root, split="test", test_area=5, block_points=BLOCK_POINTS)
        file_list = list(ds.file_list)

    sys.argv = ["main_test.py"]
    defaults = vars(ref.parse_args())
    lines = [l for l in printed.splitlines() if l.startswith(("Mean IoU of", "class ", "eval "))]
    print("\n".join(lines))
    out = dict(numpy_version=np.__version__, seed=SEED, block_points=BLOCK_POINTS, batch_size=BATCH, w_seed=W_SEED,
               file_list=np.array(file_list), labelweights=ds.labelweights, printed=np.array(lines),
               args_names=np.array(sorted(defaults)), args_values=np.array([repr(defaults[k]) for k in sorted(defaults)]))
    assert [i for i, _ in got["items"]] == list(range(len(file_list)))
    for (i, (data_room, label_room, smpw, index_room)), name in zip(got["items"], file_list):
        tag = name[len("Area_5_room_"):-4]
        out["room_" + tag] = rooms[tag]
        out["index_room_" + tag] = index_room.astype(np.int32)
        out["data_room_" + tag] = data_room[:, :, :3].astype(np.float32)
        out["sample_weight_" + tag] = smpw
    # the pool after the last add_vote of each room (add_vote returns the room's running pool)
    per_room, k = [], 0
    for i, (_, (data_room, _, _, _)) in enumerate(got["items"]):
        nb = (data_room.shape[0] + BATCH - 1) // BATCH
        per_room.append(got["pools"][k + nb - 1])
        k += nb
    for name, pool in zip(file_list, per_room):
        out["pool_" + name[len("Area_5_room_"):-4]] = pool.astype(np.int32)
    save("g20_wholescene", **out)


if __name__ == "__main__":
    main()
