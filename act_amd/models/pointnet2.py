"""PointNet++ set abstraction on the HIP kernels (reference: {part,semantic}_segmentation/models/pointnet2_utils.py:84-259).

Same public names, constructor arguments, ``state_dict`` keys and shapes, and the same call shape as the reference:

    forward(xyz [B,3,N], points [B,D,N] or None) -> (new_xyz [B,3,S], new_points [B,C',S])

so reference checkpoints load with ``strict=True``.  The layers run as rows: farthest point sampling -> ball query (``inclusive=True``: the
reference keeps sqrdists <= radius ** 2) -> grouped rows [B*S*nsample, 3+D] written once in the layout the row GEMMs read (the reference's
[B, S, nsample, 3+D] tensor is never permuted) -> per MLP layer K.linear + K.batch_norm_act (train-mode statistics over all B*S*nsample rows,
padded repeats included, as the reference's BatchNorm2d) -> K.group_max over the nsample rows of every group.

Deviations from the reference, all documented in README "PointNet++ set abstraction":
  * FPS starts from index 0 (the reference draws a random start with torch.randint); ``fps_idx=`` injects the centres.
  * distances are the fp32 difference form (dx*dx + dy*dy) + dz*dz, the project's convention, not the expansion form; the threshold is the
    fp32 product radius * radius.
  * a centre with no point in reach (impossible when the centres are cloud points) groups point 0; the reference would index out of range.

The decoder half: ``PointNetFeaturePropagation`` is the Transformer segmentation head's class (models/semseg.py: row layout, xyz as points1,
3 <= G <= 512 centres); ``PointNetFeaturePropagationAny`` below takes the reference's call shape at any N and S >= 1 (README "PointNet++
feature propagation and networks").
"""
import torch
import torch.nn as nn

from .. import kernels as K
from .. import _C
from ..pointnet2_ops import pointnet2_utils as pu
from .semseg import PointNetFeaturePropagation                        # noqa: F401  (the decoder half: the file mirrors the reference's)


def _w2d(conv):
    w = conv.weight
    return w.view(w.shape[0], w.shape[1])


def _check_mlp(name, mlp):
    if not mlp or any(int(c) < 4 or int(c) % 4 for c in mlp):
        raise ValueError(f"{name}: every mlp width must be a positive multiple of 4 (the row kernels move float4s), got {list(mlp)}")


def _inputs(name, xyz, points, in_channel):
    """[B,3,N] / [B,D,N] -> rows-major [B,N,3] / [B,N,D]; ``in_channel`` is the width of the first conv, 3 + D"""
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 3 or xyz.shape[1] != 3:
        raise _C.ActHipError(f"{name}: xyz: expected shape [B, 3, N], got {list(getattr(xyz, 'shape', ()))}")
    if not xyz.is_cuda:
        raise _C.ActHipError(f"{name}: xyz: expected a CUDA tensor (the HIP kernels have no CPU fallback)")
    if xyz.dtype != torch.float32:
        raise _C.ActHipError(f"{name}: xyz: expected float32, got {xyz.dtype}")
    B, _, N = xyz.shape
    D = 0
    if points is not None:
        if points.dim() != 3 or points.shape[0] != B or points.shape[2] != N:
            raise _C.ActHipError(f"{name}: points: expected shape [{B}, D, {N}], got {list(points.shape)}")
        if not points.is_cuda:
            raise _C.ActHipError(f"{name}: points: expected a CUDA tensor (the HIP kernels have no CPU fallback)")
        if points.dtype != torch.float32:
            raise _C.ActHipError(f"{name}: points: expected float32, got {points.dtype}")
        D = points.shape[1]
    if in_channel != 3 + D:
        raise _C.ActHipError(f"{name}: in_channel: the first conv takes {in_channel} channels but xyz + points carry 3 + {D}")
    return xyz.transpose(1, 2).contiguous(), (None if points is None else points.transpose(1, 2).contiguous())


def _centres(name, xyz, npoint, fps_idx):
    """-> new_xyz [B,S,3]: FPS from index 0 (no near-origin skip: the reference's pure-torch sampler has none) or the injected indices"""
    B, N, _ = xyz.shape
    if fps_idx is None:
        fps_idx = pu.furthest_point_sample(xyz, npoint, skip_near_origin=False)
    elif tuple(fps_idx.shape) != (B, npoint):
        raise _C.ActHipError(f"{name}: fps_idx: expected shape [{B}, {npoint}], got {list(fps_idx.shape)}")
    return torch.gather(xyz, 1, fps_idx.to(xyz.device, torch.int64).unsqueeze(-1).expand(B, npoint, 3)).contiguous()


def _chain(rows, convs, bns, training, first_weight=None):
    for i, (conv, bn) in enumerate(zip(convs, bns)):
        w = first_weight if (i == 0 and first_weight is not None) else _w2d(conv)
        rows = K.batch_norm_act(K.linear(rows, w, conv.bias), bn, training, relu=True)
    return rows


class PointNetSetAbstraction(nn.Module):
    """pointnet2_utils.PointNetSetAbstraction: parameters ``mlp_convs.{i}`` (Conv2d 1x1) / ``mlp_bns.{i}`` (BatchNorm2d).
    ``forward(xyz, points, fps_idx=None)``: ``fps_idx`` int [B, npoint] replaces the sampler (the reference starts FPS at a random index,
    this one at index 0)."""

    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all):
        super().__init__()
        _check_mlp("PointNetSetAbstraction", mlp)
        self.npoint, self.radius, self.nsample = npoint, radius, nsample
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last = in_channel
        for out in mlp:
            self.mlp_convs.append(nn.Conv2d(last, out, 1))
            self.mlp_bns.append(nn.BatchNorm2d(out))
            last = out
        self.group_all = group_all

    def forward(self, xyz, points, fps_idx=None):
        xyz, points = _inputs("PointNetSetAbstraction", xyz, points, self.mlp_convs[0].in_channels)
        B, N, _ = xyz.shape
        if self.group_all:                              # one group holds the whole cloud; raw xyz, not centred; new_xyz is zeros
            new_xyz = torch.zeros(B, 1, 3, dtype=xyz.dtype, device=xyz.device)
            rows = (xyz if points is None else torch.cat((xyz, points), dim=-1)).reshape(B * N, -1)
            S, ns = 1, N
        else:
            S, ns = self.npoint, self.nsample
            new_xyz = _centres("PointNetSetAbstraction", xyz, S, fps_idx)
            idx = K.ball_query(xyz, new_xyz, self.radius, ns, inclusive=True)
            rows = K.group_rows(xyz, new_xyz, points, idx, use_xyz=True)
        rows = _chain(rows, self.mlp_convs, self.mlp_bns, self.training)
        out = K.group_max(rows, ns)                                      # [B*S, C']
        return new_xyz.transpose(1, 2), out.view(B, S, -1).transpose(1, 2)


class PointNetSetAbstractionMsg(nn.Module):
    """pointnet2_utils.PointNetSetAbstractionMsg: one FPS, one (ball query, MLP, max) chain per radius, concatenated.  Parameters
    ``conv_blocks.{k}.{i}`` / ``bn_blocks.{k}.{i}``; ``in_channel`` is D (the constructor adds the 3 xyz channels, as the reference's).
    The reference orders the first conv's inputs (features, xyz); the grouped rows are (xyz, features), so the first weight's columns are
    rotated on the way in."""

    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list):
        super().__init__()
        self.npoint, self.radius_list, self.nsample_list = npoint, radius_list, nsample_list
        self.conv_blocks = nn.ModuleList()
        self.bn_blocks = nn.ModuleList()
        for mlp in mlp_list:
            _check_mlp("PointNetSetAbstractionMsg", mlp)
            convs, bns = nn.ModuleList(), nn.ModuleList()
            last = in_channel + 3
            for out in mlp:
                convs.append(nn.Conv2d(last, out, 1))
                bns.append(nn.BatchNorm2d(out))
                last = out
            self.conv_blocks.append(convs)
            self.bn_blocks.append(bns)

    def forward(self, xyz, points, fps_idx=None):
        xyz, points = _inputs("PointNetSetAbstractionMsg", xyz, points, self.conv_blocks[0][0].in_channels)
        B, N, _ = xyz.shape
        S = self.npoint
        D = 0 if points is None else points.shape[2]
        new_xyz = _centres("PointNetSetAbstractionMsg", xyz, S, fps_idx)
        outs = []
        for k, radius in enumerate(self.radius_list):
            ns = self.nsample_list[k]
            idx = K.ball_query(xyz, new_xyz, radius, ns, inclusive=True)
            rows = K.group_rows(xyz, new_xyz, points, idx, use_xyz=True)
            w0 = _w2d(self.conv_blocks[k][0])
            if D:
                w0 = torch.cat((w0[:, D:], w0[:, :D]), dim=1)            # (features, xyz) columns -> the rows' (xyz, features)
            rows = _chain(rows, self.conv_blocks[k], self.bn_blocks[k], self.training, first_weight=w0)
            outs.append(K.group_max(rows, ns).view(B, S, -1))
        return new_xyz.transpose(1, 2), torch.cat(outs, dim=-1).transpose(1, 2)


class PointNetFeaturePropagationAny(nn.Module):
    """pointnet2_utils.PointNetFeaturePropagation with the reference's call shape, at any size: parameters ``mlp_convs.{i}`` (Conv1d) /
    ``mlp_bns.{i}`` (BatchNorm1d), so reference checkpoints load with ``strict=True``.

        forward(xyz1 [B,3,N], xyz2 [B,3,S], points1 [B,D1,N] or None, points2 [B,D2,S]) -> [B, mlp[-1], N]

    Any N >= 1 and S >= 1: the three nearest of the S known points by K.three_nn (difference-form distances, ties to the lower index),
    inverse-distance weights normalised over the slots that exist (S == 2: two columns; S == 1: the single row repeated), then the MLP on
    cat(points1, interpolated) as rows with train-mode BatchNorm over all B*N rows.  The weights are constants: the cloud is a leaf."""

    def __init__(self, in_channel, mlp):
        super().__init__()
        _check_mlp("PointNetFeaturePropagationAny", mlp)
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last = in_channel
        for out in mlp:
            self.mlp_convs.append(nn.Conv1d(last, out, 1))
            self.mlp_bns.append(nn.BatchNorm1d(out))
            last = out

    def forward(self, xyz1, xyz2, points1, points2):
        name = "PointNetFeaturePropagationAny"
        if points2 is None:
            raise _C.ActHipError(f"{name}: points2: expected [B, D2, S], got None")
        D1 = 0 if points1 is None else (points1.shape[1] if isinstance(points1, torch.Tensor) and points1.dim() == 3 else -1)
        D2 = points2.shape[1] if isinstance(points2, torch.Tensor) and points2.dim() == 3 else -1
        cin = self.mlp_convs[0].in_channels
        if D1 >= 0 and D2 >= 0 and D1 + D2 != cin:
            raise _C.ActHipError(f"{name}: in_channel: the first conv takes {cin} channels but points1 + points2 carry {D1} + {D2}")
        x1, p1 = _inputs(name, xyz1, points1, 3 + D1)
        x2, p2 = _inputs(name, xyz2, points2, 3 + D2)
        B, N, _ = x1.shape
        S = x2.shape[1]
        if x2.shape[0] != B:
            raise _C.ActHipError(f"{name}: xyz2: expected {B} clouds, got {x2.shape[0]}")
        nn3 = K.three_nn(x1, x2, want_adj=torch.is_grad_enabled() and p2.requires_grad)
        rows = K.interp_rows(p2.reshape(B * S, D2), nn3, B, N, S)
        if p1 is not None:
            rows = torch.cat((p1.reshape(B * N, D1), rows), dim=1)
        rows = _chain(rows, self.mlp_convs, self.mlp_bns, self.training)
        return rows.view(B, N, -1).transpose(1, 2)
