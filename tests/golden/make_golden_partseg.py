#!/usr/bin/env python3
"""Generates tests/golden/g19_partseg.npz by importing the REFERENCE's part-segmentation model (part_segmentation/models/pt.py with its
models/pointnet2_utils.py) under the same shims as make_golden.py, weights from fill.py.  Run in the build container (needs the reference
tree); the .npz is the committed fixture, this script is its provenance.

    python tests/golden/make_golden_partseg.py

Recorded at B = 4 (three distinct categories: with B = 2 the label branch's BatchNorm sees two rows, x_hat = +-1, and its input gradient vanishes),
N = 256 (G = 128 x M = 32, d = 384, depth 12 are fixed by the reference model), DropPath and Dropout off:
  (a) the unmodified reference module: log-probs in train and eval mode on the first 64 points of every cloud, the NLL, gradient norms;
  (b) the same with ``square_distance`` replaced by the difference form (dx*dx + dy*dy) + dz*dz -- the project's convention:
      the full train-mode log-probs, eval-mode log-probs on the first 64 points, the NLL, gradient norms;
  the three nearest centres of both forms, the state_dict keys / shapes, and the defaults of main.py parse_args.
"""
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import install_shims, save, REF                      # noqa: E402
from fill import fill_module, clouds                                   # noqa: E402

B, N, NPART, NCAT, KEEP = 4, 256, 50, 16, 64
CATS = np.array([0, 4, 10, 4])                                         # Airplane, Chair, Motorbike, Chair
FIRST = [0, 4, 6, 8, 12, 16, 19, 22, 24, 28, 30, 36, 38, 41, 44, 47, 50]


def inputs():
    """cloud, category ids, part labels of the fixture (the tests rebuild them from here)"""
    pts = clouds(19, B, N).astype(np.float32)
    rs = np.random.RandomState(19)
    labels = np.stack([rs.randint(FIRST[c], FIRST[c + 1], size=N) for c in CATS]).astype(np.int64)
    return pts, CATS.astype(np.int64), labels


def difference_square_distance(src, dst):
    d = src[:, :, None, :] - dst[:, None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def main():
    os.chdir(REF)
    install_shims()
    sys.path.insert(0, os.path.join(REF, "part_segmentation"))
    sys.path.insert(0, os.path.join(REF, "part_segmentation", "models"))
    for name in ("pointnet2_utils", "logger", "pt", "main", "provider", "dataset", "pointnet_util"):
        sys.modules.pop(name, None)
    import pointnet2_utils as ref_pn2                                   # part_segmentation/models/pointnet2_utils.py
    import pt as ref_pt                                                 # part_segmentation/models/pt.py
    torch.set_num_threads(8)
    pts_np, cls_np, labels_np = inputs()
    pts = torch.from_numpy(pts_np).transpose(1, 2)                     # [B, 3, N] view of [B, N, 3], as main.py passes it
    cls_label = torch.eye(NCAT)[torch.from_numpy(cls_np).view(B, 1)]   # main.py to_categorical(label [B,1], 16) -> [B, 1, 16]
    target = torch.from_numpy(labels_np).reshape(-1)

    model = fill_module(ref_pt.get_model(NPART), "g19.")
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "drop_prob"):
            m.drop_prob = 0.0
    init = {k: v.clone() for k, v in model.state_dict().items()}
    criterion = ref_pt.get_loss()
    out = dict(pts=pts_np, cls=cls_np, labels=labels_np,
               sd_keys=np.array(list(init.keys())), sd_shapes=np.array([",".join(map(str, v.shape)) for v in init.values()]))
    expansion = ref_pn2.square_distance
    for tag, sqd in (("a", expansion), ("b", difference_square_distance)):
        ref_pn2.square_distance = sqd
        model.load_state_dict(init)
        model.zero_grad(set_to_none=True)
        model.train()
        logp = model(pts, cls_label)
        loss = criterion(logp.contiguous().view(-1, NPART), target)
        loss.backward()
        names = [n for n, p in model.named_parameters()]
        out[f"{tag}_logp_train"] = logp.detach() if tag == "b" else logp.detach()[:, :KEEP]
        out[f"{tag}_loss"] = loss
        out[f"{tag}_grad_names"] = np.array(names)
        out[f"{tag}_grad_norms"] = np.array([dict(model.named_parameters())[n].grad.norm().item() for n in names])
        model.eval()
        with torch.no_grad():
            out[f"{tag}_logp_eval"] = model(pts, cls_label)[:, :KEEP]
            _, center = model.group_divider(pts.transpose(1, 2).contiguous())
            d, idx = sqd(pts.transpose(1, 2), center).sort(dim=-1)
            out[f"{tag}_nn3_idx"] = idx[:, :, :3].to(torch.int32)
    ref_pn2.square_distance = expansion
    # argument defaults of the reference's training script (main.py parse_args)
    argv, sys.argv = sys.argv, ["main.py"]
    try:
        import main as ref_main
        defaults = vars(ref_main.parse_args())
    finally:
        sys.argv = argv
    out["args_names"] = np.array(sorted(defaults))
    out["args_values"] = np.array([repr(defaults[k]) for k in sorted(defaults)])
    save("g19_partseg", **out)


if __name__ == "__main__":
    main()
