#!/usr/bin/env python3
"""Generates tests/golden/g18_semseg.npz by importing the REFERENCE's semantic-segmentation model (semantic_segmentation/models/pt.py with
its models/pointnet2_utils.py) under the same shims as make_golden.py, weights from fill.py.  Run in the build container (needs the reference
tree); the .npz is the committed fixture, this script is its provenance.

    python tests/golden/make_golden_semseg.py

Recorded at B = 2, N = 512 (G = 128 x M = 32, d = 384, depth 12 are fixed by the reference model), DropPath and Dropout off:
  (a) the unmodified reference module: log-probs in train and eval mode, the weighted NLL, per-parameter gradient norms, state_dict keys / shapes;
  (b) the same with ``square_distance`` replaced by the difference form (dx*dx + dy*dy) + dz*dz -- the project's convention.
"""
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import install_shims, save, REF                      # noqa: E402
from fill import fill_module, clouds                                   # noqa: E402

B, N, NCLS = 2, 512, 13


def inputs():
    """cloud, labels, class weights of the fixture (the tests rebuild them from here)"""
    pts = clouds(18, B, N)
    pts[:, :, 2] += np.float32(1.5)                                     # S3DIS-like height above the floor (larger |p|^2)
    rs = np.random.RandomState(18)
    labels = rs.randint(0, NCLS, size=(B, N)).astype(np.int64)
    weight = (1.0 + rs.rand(NCLS)).astype(np.float32)
    return pts.astype(np.float32), labels, weight


def difference_square_distance(src, dst):
    d = src[:, :, None, :] - dst[:, None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def main():
    os.chdir(REF)
    install_shims()
    sys.path.insert(0, os.path.join(REF, "semantic_segmentation"))
    sys.path.insert(0, os.path.join(REF, "semantic_segmentation", "models"))
    for name in ("pointnet2_utils", "logger", "pt"):
        sys.modules.pop(name, None)
    import pointnet2_utils as ref_pn2                                   # semantic_segmentation/models/pointnet2_utils.py
    import pt as ref_pt                                                 # semantic_segmentation/models/pt.py
    torch.set_num_threads(8)
    pts_np, labels_np, weight_np = inputs()
    pts = torch.from_numpy(pts_np).transpose(1, 2)                     # [B, 3, N] view of [B, N, 3], as main.py passes it
    target = torch.from_numpy(labels_np).reshape(-1)
    weight = torch.from_numpy(weight_np)

    model = fill_module(ref_pt.get_model(NCLS), "g18.")
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "drop_prob"):
            m.drop_prob = 0.0
    init = {k: v.clone() for k, v in model.state_dict().items()}
    criterion = ref_pt.get_loss()
    out = dict(pts=pts_np, labels=labels_np, weight=weight_np,
               sd_keys=np.array(list(init.keys())), sd_shapes=np.array([",".join(map(str, v.shape)) for v in init.values()]))
    expansion = ref_pn2.square_distance
    for tag, sqd in (("a", expansion), ("b", difference_square_distance)):
        ref_pn2.square_distance = sqd
        model.load_state_dict(init)
        model.zero_grad(set_to_none=True)
        model.train()
        logp = model(pts)
        loss = criterion(logp.contiguous().view(-1, NCLS), target, weight)
        loss.backward()
        names = [n for n, p in model.named_parameters()]
        out[f"{tag}_logp_train"] = logp
        out[f"{tag}_loss"] = loss
        out[f"{tag}_grad_names"] = np.array(names)
        out[f"{tag}_grad_norms"] = np.array([dict(model.named_parameters())[n].grad.norm().item() for n in names])
        model.eval()
        with torch.no_grad():
            out[f"{tag}_logp_eval"] = model(pts)
        # three nearest centres of the reference's propagation (FPS of the shim = the in-tree sampler, start index 0)
        with torch.no_grad():
            _, center = model.group_divider(pts.transpose(1, 2).contiguous())
            d, idx = sqd(pts.transpose(1, 2), center).sort(dim=-1)
            out[f"{tag}_nn3_idx"] = idx[:, :, :3].to(torch.int32)
    ref_pn2.square_distance = expansion
    # argument defaults of the reference's training script (main.py parse_args)
    sys.modules.pop("main", None)
    argv, sys.argv = sys.argv, ["main.py"]
    try:
        import main as ref_main
        defaults = vars(ref_main.parse_args())
    finally:
        sys.argv = argv
    out["args_names"] = np.array(sorted(defaults))
    out["args_values"] = np.array([repr(defaults[k]) for k in sorted(defaults)])
    save("g18_semseg", **out)


if __name__ == "__main__":
    main()
