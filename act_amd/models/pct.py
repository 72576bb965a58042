"""Point Cloud Transformer (PCT; Guo et al., CVM 2021; the layer table of the widely used PyTorch port of the classifier) on the HIP kernels:
csrc/offset_attn.hip for the offset attention, the library's FPS, kNN, grouping, GEMM, BatchNorm and group-max kernels for the rest.

    Pct       forward(pts [B,N,3]) -> logits [B, output_channels]                                          (MODELS: ``PCT``)
    pct(num_classes=40): the published configuration; widths, point counts and nsample are keywords

The modules carry the port's attribute names (``conv1``, ``bn1``, ``gather_local_{0,1}.conv1``, ``pt_last.sa{1..4}.q_conv``, ``conv_fuse.{0,1}``,
``linear1``, ``bn6``, ...), so a ``state_dict`` of that layout loads with ``strict=True``; ``q_conv.weight`` IS ``k_conv.weight`` (one Parameter under
two keys), as in the port.  The forward calls the kernels, never the Sequentials.  Everything runs as rows:

  * ``Local_op`` reads cat(x_j - x_i, x_i): Wa (x_j - x_i) + Wb x_i = Wa x_j + (Wb - Wa) x_i, so the neighbour rows are gathered once
    (``K.group_rows``), the centre's half is one product per CENTRE added in the epilogue of the per-row product (``K.linear_group_add``), and the
    repeated half is never materialised; the max over the neighbours is ``K.group_max``;
  * ``SA_Layer`` forms the shared query / key projection once and hands it to ``K.offset_attention`` as both operands, with x fused:
    x + ReLU(after_norm(trans_conv(x - x_r)));
  * ``conv_fuse`` and the head are ``K.linear`` + ``K.batch_norm_act(slope=0.2)``, the max over the points ``K.group_max``.

Choices are injectable through ``draws``: the centres of stage i under ``fps.{i}`` (FPS starts at index 0), its neighbour lists under ``knn.{i}``
(``knn_group(xyz, new_xyz, nsample)``; the port's radius argument is unused), the dropout keep-masks under ``head.dp1`` / ``head.dp2``.  Not
implemented: the part-segmentation network, the NPCT / SPCT variants, the port's label-smoothing loss, gradients through the neighbour choice.
"""
import torch
import torch.nn as nn

from .. import kernels as K
from ..knn_cuda import knn_group
from ..pointnet2_ops import pointnet2_utils as pu
from .build import MODELS
from .pointnet2_nets import _dropout, _load

SLOPE = 0.2


def _w2d(conv):
    w = conv.weight
    return w.view(w.shape[0], w.shape[1])


def _width(who, c):
    c = int(c)
    if c < 4 or c % 4:
        raise ValueError(f"{who}: every width must be a positive multiple of 4 (the row kernels move float4s), got {c}")
    return c


def sample_and_group(xyz, npoint, nsample, draws=None, stage=None):
    """-> (fps_idx [B,S], new_xyz [B,S,3], idx [B,S,nsample]): FPS from index 0 and the nsample nearest points of every centre, or the injected lists"""
    B = xyz.shape[0]
    make = lambda: pu.furthest_point_sample(xyz, npoint, skip_near_origin=False)
    fps_idx = (draws.get(f"fps.{stage}", make) if draws is not None and stage is not None else make()).to(xyz.device)
    new_xyz = torch.gather(xyz, 1, fps_idx.to(torch.int64).unsqueeze(-1).expand(B, npoint, 3)).contiguous()
    knn = lambda: knn_group(xyz, new_xyz, nsample)[0]
    idx = draws.get(f"knn.{stage}", knn) if draws is not None and stage is not None else knn()
    return fps_idx, new_xyz, idx.to(xyz.device)


class Local_op(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        if in_channels % 2:
            raise ValueError(f"Local_op: in_channels is twice the feature width, got {in_channels}")
        self.conv1 = nn.Conv1d(in_channels, _width("Local_op", out_channels), kernel_size=1, bias=False)
        self.conv2 = nn.Conv1d(out_channels, out_channels, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm1d(out_channels)
        self.bn2 = nn.BatchNorm1d(out_channels)

    def rows(self, feat, fps_idx, idx):
        """feat [B,N,D], fps_idx [B,S], idx [B,S,k] -> [B*S, out]: conv1 on cat(x_j - x_i, x_i) by the EdgeConv identity"""
        B, N, D = feat.shape
        S, k = idx.shape[1], idx.shape[2]
        W = _w2d(self.conv1)
        Wa = W[:, :D].contiguous()
        centres = torch.gather(feat, 1, fps_idx.to(torch.int64).unsqueeze(-1).expand(B, S, D)).reshape(B * S, D)
        per_centre = K.linear(centres, W[:, D:] - Wa)
        x = K.linear_group_add(K.group_rows(None, None, feat, idx, use_xyz=False), Wa, per_centre, k)
        x = K.batch_norm_act(x, self.bn1, self.training, relu=True)
        x = K.batch_norm_act(K.linear(x, _w2d(self.conv2)), self.bn2, self.training, relu=True)
        return K.group_max(x, k)


class SA_Layer(nn.Module):
    def __init__(self, channels):
        super().__init__()
        _width("SA_Layer", channels // 4)
        self.q_conv = nn.Conv1d(channels, channels // 4, 1, bias=False)
        self.k_conv = nn.Conv1d(channels, channels // 4, 1, bias=False)
        self.q_conv.weight = self.k_conv.weight
        self.v_conv = nn.Conv1d(channels, channels, 1)
        self.trans_conv = nn.Conv1d(channels, channels, 1)
        self.after_norm = nn.BatchNorm1d(channels)
        self.act = nn.ReLU()
        self.softmax = nn.Softmax(dim=-1)

    def rows(self, x, B, N):
        """x [B*N, c] -> x + ReLU(after_norm(trans_conv(x - x_r)))"""
        q = K.linear(x, _w2d(self.q_conv))
        k = q if self.k_conv.weight is self.q_conv.weight else K.linear(x, _w2d(self.k_conv))      # two products only once the weights are untied
        v = K.linear(x, _w2d(self.v_conv), self.v_conv.bias)
        d = K.offset_attention(q, k, v, B, N, x=x)
        return x + K.batch_norm_act(K.linear(d, _w2d(self.trans_conv), self.trans_conv.bias), self.after_norm, self.training, relu=True)


class Point_Transformer_Last(nn.Module):
    def __init__(self, channels=256):
        super().__init__()
        self.conv1 = nn.Conv1d(channels, channels, kernel_size=1, bias=False)
        self.conv2 = nn.Conv1d(channels, channels, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm1d(channels)
        self.bn2 = nn.BatchNorm1d(channels)
        self.sa1, self.sa2, self.sa3, self.sa4 = SA_Layer(channels), SA_Layer(channels), SA_Layer(channels), SA_Layer(channels)

    def rows(self, x, B, N):
        """x [B*N, c] -> cat(x1, x2, x3, x4) [B*N, 4c]"""
        x = K.batch_norm_act(K.linear(x, _w2d(self.conv1)), self.bn1, self.training, relu=True)
        x = K.batch_norm_act(K.linear(x, _w2d(self.conv2)), self.bn2, self.training, relu=True)
        outs = []
        for sa in (self.sa1, self.sa2, self.sa3, self.sa4):
            x = sa.rows(x, B, N)
            outs.append(x)
        return torch.cat(outs, dim=1)


class Pct(nn.Module):
    def __init__(self, output_channels=40, dropout=0.5, points=1024, npoint=(512, 256), nsample=32, width=64, fuse=1024, head=(512, 256), **kwargs):
        super().__init__()
        self.points, self.npoint, self.nsample = int(points), (int(npoint[0]), int(npoint[1])), int(nsample)
        if not self.points >= self.npoint[0] >= self.npoint[1] >= 1 or not 1 <= self.nsample <= self.npoint[0]:
            raise ValueError(f"pct: need points >= npoint[0] >= npoint[1] >= 1 and 1 <= nsample <= npoint[0], got {points}, {npoint}, {nsample}")
        if self.npoint[1] > 1024:
            raise ValueError(f"pct: the offset attention takes at most 1024 points, got npoint[1] = {self.npoint[1]}")
        width = _width("pct", width)
        self.conv1 = nn.Conv1d(3, width, kernel_size=1, bias=False)
        self.conv2 = nn.Conv1d(width, width, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm1d(width)
        self.bn2 = nn.BatchNorm1d(width)
        self.gather_local_0 = Local_op(2 * width, 2 * width)
        self.gather_local_1 = Local_op(4 * width, 4 * width)
        self.pt_last = Point_Transformer_Last(4 * width)
        self.conv_fuse = nn.Sequential(nn.Conv1d(20 * width, _width("pct", fuse), kernel_size=1, bias=False), nn.BatchNorm1d(fuse),
                                       nn.LeakyReLU(negative_slope=SLOPE))
        self.linear1 = nn.Linear(fuse, _width("pct", head[0]), bias=False)
        self.bn6 = nn.BatchNorm1d(head[0])
        self.dp1 = nn.Dropout(p=dropout)
        self.linear2 = nn.Linear(head[0], _width("pct", head[1]))
        self.bn7 = nn.BatchNorm1d(head[1])
        self.dp2 = nn.Dropout(p=dropout)
        self.linear3 = nn.Linear(head[1], output_channels)

    def forward_features(self, pts, draws=None):
        """pts [B,N,3] -> (logits, the [B, fuse] global feature the head reads)"""
        if pts.dim() != 3 or pts.shape[2] != 3:
            raise ValueError(f"pct: pts: expected [B, N, 3], got {list(pts.shape)}")
        B, N, _ = pts.shape
        if N != self.points:
            raise ValueError(f"pct: built for clouds of {self.points} points, got {N}")
        xyz, tr = pts.contiguous(), self.training
        x = K.batch_norm_act(K.linear(xyz.reshape(B * N, 3), _w2d(self.conv1)), self.bn1, tr, relu=True)
        x = K.batch_norm_act(K.linear(x, _w2d(self.conv2)), self.bn2, tr, relu=True)
        S1, S2 = self.npoint
        fps_idx, xyz1, idx = sample_and_group(xyz, S1, self.nsample, draws, 1)
        f0 = self.gather_local_0.rows(x.view(B, N, -1), fps_idx, idx)                      # [B*S1, 2w]
        fps_idx, _, idx = sample_and_group(xyz1, S2, self.nsample, draws, 2)
        f1 = self.gather_local_1.rows(f0.view(B, S1, -1), fps_idx, idx)                    # [B*S2, 4w]
        x = torch.cat((self.pt_last.rows(f1, B, S2), f1), dim=1)
        x = K.batch_norm_act(K.linear(x, _w2d(self.conv_fuse[0])), self.conv_fuse[1], tr, slope=SLOPE)
        f = K.group_max(x, S2)
        h = K.batch_norm_act(K.linear(f, self.linear1.weight), self.bn6, tr, slope=SLOPE)
        h = _dropout(h, self.dp1, tr, draws, "head.dp1")
        h = K.batch_norm_act(K.linear(h, self.linear2.weight, self.linear2.bias), self.bn7, tr, slope=SLOPE)
        h = _dropout(h, self.dp2, tr, draws, "head.dp2")
        return K.linear(h, self.linear3.weight, self.linear3.bias), f

    def forward(self, pts, draws=None):
        return self.forward_features(pts, draws)[0]


def pct(num_classes=40, **kwargs):
    return Pct(output_channels=num_classes, **kwargs)


@MODELS.register_module()
class PCT(Pct):
    """``pct`` behind the config interface of ``PointTransformer``: key ``cls_dim`` and, optionally, any keyword of ``Pct`` (``points``, ``npoint``,
    ``nsample``, ``width``, ``fuse``, ``head``, ``dropout``)"""

    def __init__(self, config, **kwargs):
        table = {k: config.get(k) for k in ("dropout", "points", "npoint", "nsample", "width", "fuse", "head") if config.get(k) is not None}
        super().__init__(output_channels=config.cls_dim, **table)
        self.config = config
        self.build_loss_func()

    def build_loss_func(self):
        self.loss_ce = nn.CrossEntropyLoss()          # kept for interface parity; get_loss_acc runs the HIP kernel

    def get_loss_acc(self, ret, gt):
        """-> (mean cross-entropy, top-1 accuracy in percent), both on the device, no host sync."""
        loss, acc = K.softmax_xent(ret, gt)
        return loss, acc * 100

    def load_model_from_ckpt(self, bert_ckpt_path, custom_loading=False):
        return _load(self, bert_ckpt_path, 'PCT')
