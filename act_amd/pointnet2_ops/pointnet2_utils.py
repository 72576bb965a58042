"""Drop-in for the pointnet2_ops entry points: ``furthest_point_sample`` and ``gather_operation`` (the two ACT uses, utils/misc.py:44-45),
backed by act_fps_f32 / act_gather_points_f32, and the grouping family of a PointNet++ baseline -- ``ball_query``, ``grouping_operation``,
``QueryAndGroup``, ``GroupAll`` -- backed by csrc/sa.hip (include/act_hip.h), and ``three_nn`` / ``three_interpolate`` in upstream's form
(distances and caller-supplied weights) on the general three-NN and interpolation kernels of the same file."""
import torch
import torch.nn as nn

from .. import _C


def _need(t, dtype, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")            # upstream: TORCH_CHECK is_cuda
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be a {dtype} tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous tensor")


def _scratch(xyz, B, N):
    n = _C.lib.act_fps_scratch_floats(B, N)              # > 0 only for clouds beyond 16,384 points (running distances in HBM)
    return torch.empty(n, dtype=torch.float32, device=xyz.device) if n else None


def _skip(flag):
    """``skip_near_origin=None`` -> the process-wide default: ACT_FPS_SKIP_NEAR_ORIGIN=1 reproduces upstream pointnet2_ops, which
    never selects points with |p|^2 <= 1e-3; the default (0) is the in-tree pure-torch FPS of the reference."""
    return SKIP_NEAR_ORIGIN if flag is None else bool(flag)


SKIP_NEAR_ORIGIN = __import__("os").environ.get("ACT_FPS_SKIP_NEAR_ORIGIN", "0") == "1"


def furthest_point_sample(xyz, npoint, skip_near_origin=None):
    """xyz f32 [B,N,3] -> int32 [B,npoint]; first index 0, lowest-index tie-break.  Non-differentiable.

    ``skip_near_origin=True`` reproduces upstream pointnet2_ops' |p|^2 <= 1e-3 skip."""
    _need(xyz, torch.float32, "xyz")
    B, N, C = xyz.shape
    if C != 3:
        raise RuntimeError("xyz must be [B, N, 3]")
    idx = torch.empty(B, npoint, dtype=torch.int32, device=xyz.device)
    _C.check(_C.lib.act_fps_f32(_C.ptr(xyz), B, N, int(npoint), _C.ptr(idx), None, int(_skip(skip_near_origin)), _C.ptr(_scratch(xyz, B, N)),
                                _C.stream()), "act_fps_f32")
    return idx


def furthest_point_sample_with_centers(xyz, npoint, skip_near_origin=None):
    """fused FPS + gather: -> (idx int32 [B,G], centers f32 [B,G,3]) in one launch."""
    _need(xyz, torch.float32, "xyz")
    B, N, _ = xyz.shape
    idx = torch.empty(B, npoint, dtype=torch.int32, device=xyz.device)
    centers = torch.empty(B, npoint, 3, dtype=torch.float32, device=xyz.device)
    _C.check(_C.lib.act_fps_f32(_C.ptr(xyz), B, N, int(npoint), _C.ptr(idx), _C.ptr(centers), int(_skip(skip_near_origin)),
                                _C.ptr(_scratch(xyz, B, N)), _C.stream()), "act_fps_f32")
    return idx, centers


class GatherOperation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx):
        _need(features, torch.float32, "features"); _need(idx, torch.int32, "idx")
        B, C, N = features.shape
        S = idx.shape[1]
        out = torch.empty(B, C, S, dtype=torch.float32, device=features.device)
        _C.check(_C.lib.act_gather_points_f32(_C.ptr(features), _C.ptr(idx), B, C, N, S, _C.ptr(out), _C.stream()),
                 "act_gather_points_f32")
        ctx.save_for_backward(idx)
        ctx.N = N
        ctx.mark_non_differentiable(idx)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        B, C, S = grad_out.shape
        gf = torch.empty(B, C, ctx.N, dtype=torch.float32, device=grad_out.device)
        _C.check(_C.lib.act_gather_points_bwd_f32(_C.ptr(grad_out), _C.ptr(idx), B, C, ctx.N, S, _C.ptr(gf), _C.stream()),
                 "act_gather_points_bwd_f32")
        return gf, None


gather_operation = GatherOperation.apply


def ball_query(radius, nsample, xyz, new_xyz):
    """upstream's signature and rule: xyz [B,N,3], new_xyz [B,S,3] -> int32 [B,S,nsample], the first ``nsample`` indices with d2 < radius^2
    in ascending order, the rest of the row repeating the first hit (a row of zeros when nothing is in reach).  Non-differentiable."""
    from .. import kernels as K
    return K.ball_query(xyz, new_xyz, radius, nsample, inclusive=False)


def grouping_operation(features, idx):
    """features f32 [B,C,N], idx int32 [B,S,nsample] -> [B,C,S,nsample]; differentiable in ``features`` (deterministic backward)"""
    from .. import kernels as K
    return K.grouping_operation(features, idx)


class QueryAndGroup(nn.Module):
    """upstream QueryAndGroup: forward(xyz [B,N,3], new_xyz [B,S,3], features [B,C,N] or None) -> [B, 3 + C, S, nsample]
    (grouped xyz minus the centre first; [B, C, S, nsample] with ``use_xyz=False``)."""

    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, new_xyz, features=None):
        idx = ball_query(self.radius, self.nsample, xyz, new_xyz)
        grouped_xyz = grouping_operation(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)
        if features is None:
            assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
            return grouped_xyz
        grouped = grouping_operation(features, idx)
        return torch.cat([grouped_xyz, grouped], dim=1) if self.use_xyz else grouped


class GroupAll(nn.Module):
    """upstream GroupAll: forward(xyz [B,N,3], new_xyz ignored, features [B,C,N] or None) -> [B, 3 + C, 1, N]"""

    def __init__(self, use_xyz=True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
        if features is None:
            return grouped_xyz
        grouped = features.unsqueeze(2)
        return torch.cat([grouped_xyz, grouped], dim=1) if self.use_xyz else grouped


def three_nn(unknown, known):
    """upstream's signature: unknown [B,n,3], known [B,m,3] -> (dist [B,n,3] = sqrt(d2), idx int32 [B,n,3]): the three nearest known points in
    ascending (distance, index) order, equal distances to the lower index.  m < 3: the missing slots carry dist = +inf and idx 0.
    Non-differentiable."""
    from .. import kernels as K
    for t, name in ((unknown, "unknown"), (known, "known")):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError(f"three_nn: {name} must be [B, {'n' if name == 'unknown' else 'm'}, 3], got {list(getattr(t, 'shape', ()))}")
    if unknown.shape[0] != known.shape[0]:
        raise ValueError(f"three_nn: unknown has {unknown.shape[0]} clouds, known {known.shape[0]}")
    if unknown.shape[0] < 1 or unknown.shape[1] < 1 or known.shape[1] < 1:
        raise ValueError(f"three_nn: unknown {list(unknown.shape)} / known {list(known.shape)} must not be empty")
    _need(unknown, torch.float32, "unknown"); _need(known, torch.float32, "known")
    idx, _, _, _, d2 = K.three_nn(unknown, known, want_adj=False, want_d2=True)
    return torch.sqrt(d2), idx


class ThreeInterpolate(torch.autograd.Function):
    """upstream three_interpolate: features [B,C,m], idx int32 [B,n,3], weight [B,n,3] -> [B,C,n], out[b,:,i] = sum_k weight[b,i,k] *
    features[b,:,idx[b,i,k]].  Differentiable in ``features`` only; the backward gathers over an inverse adjacency in ascending entry order (no
    atomics, bit-identical run to run).  A slot of weight exactly 0 is skipped, not multiplied."""

    @staticmethod
    def forward(ctx, features, idx, weight):
        from .. import kernels as K
        if not isinstance(features, torch.Tensor) or features.dim() != 3:
            raise ValueError(f"three_interpolate: features must be [B, C, m], got {list(getattr(features, 'shape', ()))}")
        B, C, m = features.shape
        for t, name in ((idx, "idx"), (weight, "weight")):
            if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[0] != B or t.shape[2] != 3:
                raise ValueError(f"three_interpolate: {name} must be [{B}, n, 3], got {list(getattr(t, 'shape', ()))}")
        if idx.shape[1] != weight.shape[1]:
            raise ValueError(f"three_interpolate: idx names {idx.shape[1]} points, weight {weight.shape[1]}")
        _need(features, torch.float32, "features"); _need(idx, torch.int32, "idx"); _need(weight, torch.float32, "weight")
        n = idx.shape[1]
        if B < 1 or C < 1 or m < 1 or n < 1:
            raise ValueError(f"three_interpolate: features {list(features.shape)} / idx {list(idx.shape)} must not be empty")
        rows = features.transpose(1, 2).reshape(B * m, C)
        out = K.interp_rows_fwd(rows, idx, weight, B, n, m)
        ctx.save_for_backward(idx, weight)
        ctx.dims = (B, n, m)
        return out.view(B, n, C).transpose(1, 2).contiguous()

    @staticmethod
    def backward(ctx, grad_out):
        from .. import kernels as K
        idx, weight = ctx.saved_tensors
        B, n, m = ctx.dims
        C = grad_out.shape[1]
        off, ent = K.three_adjacency(idx, m)
        d = K.interp_rows_bwd(grad_out.transpose(1, 2).reshape(B * n, C), off, ent, weight, B, n, m)
        return d.view(B, m, C).transpose(1, 2).contiguous(), None, None


def three_interpolate(features, idx, weight):
    return ThreeInterpolate.apply(features, idx, weight)
