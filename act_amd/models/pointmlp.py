"""PointMLP (Ma et al., ICLR 2022; the layer table of the authors' classification code) on the HIP kernels: csrc/pointmlp.hip for the geometric
affine grouping and the residual block tail, the library's FPS, kNN, GEMM, BatchNorm and group-max kernels for the rest.

    LocalGrouper   forward(xyz [B,N,3], points [B,N,D]) -> (new_xyz [B,S,3], new_points [B,S,k,2D (+3 with use_xyz)])    upstream's call shape
    Model          forward(pts [B,N,3])                 -> logits [B,class_num]                                           (MODELS: ``PointMLP``)
    pointmlp(num_classes=40), pointmlp_elite(num_classes=40): the two published configurations; every entry of their tables is a keyword

The modules carry upstream's attribute names (``embedding.net.0``, ``local_grouper_list.{i}.affine_alpha``, ``pre_blocks_list.{i}.transfer.net.0``,
``pre_blocks_list.{i}.operation.{j}.net1.0``, ``pos_blocks_list.{i}.operation.{j}.net2.1``, ``classifier.{0,1,4,5,8}``), so a ``state_dict`` of that
layout loads with ``strict=True``; the forward calls the kernels, never the Sequentials.  Everything runs as rows:

  * the grouper writes the normalised neighbour rows [B*S*k, D] once (``K.geo_affine_group``, cat=False) -- upstream's [B,S,k,2D] tensor with the
    anchor repeated k times is formed only by the public ``LocalGrouper.forward``;
  * ``transfer`` reads cat(normalised row, anchor row): its anchor half is one product per ANCHOR, added in the epilogue of the per-row product
    (``K.linear_group_add``), so the repeated half is never materialised;
  * a residual block is ``K.batch_norm_add_relu(K.linear(K.batch_norm_act(K.linear(x))), x)``;
  * the max over the k neighbours and the final max over the points are ``K.group_max``.

Choices are injectable through ``draws``: the anchors of stage i under ``fps.{i}`` (FPS starts at index 0), its neighbour lists under ``knn.{i}``
(``knn_group(xyz, new_xyz, k)``), the dropout keep-masks under ``head.dp1`` / ``head.dp2``.  Not implemented: normalize="center" / None, conv
groups > 1, upstream's label-smoothing loss, the part-segmentation network, gradients through the neighbour choice.
"""
import torch
import torch.nn as nn

from .. import kernels as K
from ..knn_cuda import knn_group
from ..pointnet2_ops import pointnet2_utils as pu
from .build import MODELS
from .pointnet2_nets import _dropout, _load


def _w2d(conv):
    w = conv.weight
    return w.view(w.shape[0], w.shape[1])


def _act(activation):
    if activation != "relu":
        raise ValueError(f"pointmlp: only activation='relu' is implemented, got {activation!r}")
    return nn.ReLU(inplace=True)


def _width(who, c):
    c = int(c)
    if c < 4 or c % 4:
        raise ValueError(f"{who}: every width must be a positive multiple of 4 (the row kernels move float4s), got {c}")
    return c


class ConvBNReLU1D(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=1, bias=True, activation="relu"):
        super().__init__()
        if kernel_size != 1:
            raise ValueError("ConvBNReLU1D: kernel_size must be 1")
        self.act = _act(activation)
        self.net = nn.Sequential(nn.Conv1d(in_channels, _width("ConvBNReLU1D", out_channels), kernel_size=1, bias=bias), nn.BatchNorm1d(out_channels),
                                 self.act)

    def rows(self, x):
        """x [R, in] -> [R, out]"""
        return K.batch_norm_act(K.linear(x, _w2d(self.net[0]), self.net[0].bias), self.net[1], self.training, relu=True)

    def forward(self, x):
        """x [B, in, N] -> [B, out, N] (upstream's call shape)"""
        B, C, N = x.shape
        return self.rows(x.transpose(1, 2).reshape(B * N, C)).view(B, N, -1).transpose(1, 2)


class ConvBNReLURes1D(nn.Module):
    def __init__(self, channel, kernel_size=1, groups=1, res_expansion=1.0, bias=True, activation="relu"):
        super().__init__()
        if kernel_size != 1 or groups != 1:
            raise ValueError("ConvBNReLURes1D: kernel_size must be 1 and groups must be 1 (grouped convolutions are not implemented)")
        mid = _width("ConvBNReLURes1D", int(channel * res_expansion))
        self.act = _act(activation)
        self.net1 = nn.Sequential(nn.Conv1d(_width("ConvBNReLURes1D", channel), mid, kernel_size=1, bias=bias), nn.BatchNorm1d(mid), self.act)
        self.net2 = nn.Sequential(nn.Conv1d(mid, channel, kernel_size=1, bias=bias), nn.BatchNorm1d(channel))

    def rows(self, x):
        """x [R, channel] -> ReLU(net2(net1(x)) + x)"""
        h = K.batch_norm_act(K.linear(x, _w2d(self.net1[0]), self.net1[0].bias), self.net1[1], self.training, relu=True)
        return K.batch_norm_add_relu(K.linear(h, _w2d(self.net2[0]), self.net2[0].bias), x, self.net2[1], self.training)

    def forward(self, x):
        B, C, N = x.shape
        return self.rows(x.transpose(1, 2).reshape(B * N, C)).view(B, N, C).transpose(1, 2)


class LocalGrouper(nn.Module):
    def __init__(self, channel, groups, kneighbors, use_xyz=True, normalize="anchor", **kwargs):
        super().__init__()
        if normalize != "anchor":
            raise ValueError(f"LocalGrouper: only normalize='anchor' is implemented (both published networks use it), got {normalize!r}")
        self.groups, self.kneighbors, self.use_xyz, self.normalize = int(groups), int(kneighbors), bool(use_xyz), normalize
        width = channel + (3 if self.use_xyz else 0)
        self.affine_alpha = nn.Parameter(torch.ones([1, 1, 1, width]))
        self.affine_beta = nn.Parameter(torch.zeros([1, 1, 1, width]))

    def choose(self, xyz, draws=None, stage=None):
        """-> (fps_idx int32 [B,S], new_xyz [B,S,3], idx [B,S,k]): FPS from index 0 and the k nearest points of every anchor, or the injected lists"""
        B, N, _ = xyz.shape
        make = lambda: pu.furthest_point_sample(xyz, self.groups, skip_near_origin=False)
        fps_idx = draws.get(f"fps.{stage}", make) if draws is not None and stage is not None else make()
        fps_idx = fps_idx.to(xyz.device)
        new_xyz = torch.gather(xyz, 1, fps_idx.to(torch.int64).unsqueeze(-1).expand(B, self.groups, 3)).contiguous()
        knn = lambda: knn_group(xyz, new_xyz, self.kneighbors)[0]
        idx = draws.get(f"knn.{stage}", knn) if draws is not None and stage is not None else knn()
        return fps_idx, new_xyz, idx.to(xyz.device)

    def rows(self, xyz, points, draws=None, stage=None, cat=False, validate=None):
        """xyz [B,N,3], points [B,N,D] -> (new_xyz [B,S,3], anchors [B*S, D], rows [B*S*k, D'] (cat: [.., 2D']), D' = D + 3 with use_xyz)"""
        B, N, D = points.shape
        xyz = xyz.contiguous()
        fps_idx, new_xyz, idx = self.choose(xyz, draws, stage)
        table = torch.cat((points, xyz), dim=-1) if self.use_xyz else points
        injected = draws is not None and stage is not None and (draws.has(f"fps.{stage}") or draws.has(f"knn.{stage}"))
        rows = K.geo_affine_group(table, fps_idx, idx, self.affine_alpha, self.affine_beta, eps=1e-5, cat=cat,
                                  validate=injected if validate is None else validate)
        anchors = torch.gather(points, 1, fps_idx.to(torch.int64).unsqueeze(-1).expand(B, self.groups, D)).reshape(B * self.groups, D)
        return new_xyz, anchors, rows

    def forward(self, xyz, points):
        B, N, D = points.shape
        S, k = self.groups, self.kneighbors
        new_xyz, anchors, rows = self.rows(xyz, points, cat=not self.use_xyz)
        if self.use_xyz:                                  # upstream repeats the anchor's FEATURES only: [normalised (D + 3) | anchor (D)]
            rows = torch.cat((rows.view(B, S, k, D + 3), anchors.view(B, S, 1, D).expand(B, S, k, D)), dim=-1)
        return new_xyz, rows.view(B, S, k, -1)


class PreExtraction(nn.Module):
    def __init__(self, channels, out_channels, blocks=1, groups=1, res_expansion=1, bias=True, activation="relu", use_xyz=True):
        super().__init__()
        self.channels = int(channels)
        in_channels = 3 + 2 * channels if use_xyz else 2 * channels
        self.transfer = ConvBNReLU1D(in_channels, out_channels, bias=bias, activation=activation)
        self.operation = nn.Sequential(*[ConvBNReLURes1D(out_channels, groups=groups, res_expansion=res_expansion, bias=bias, activation=activation)
                                         for _ in range(blocks)])

    def rows(self, rows, anchors, k):
        """rows [B*S*k, D'] (the normalised neighbours), anchors [B*S, D] -> [B*S, out]"""
        conv, bn = self.transfer.net[0], self.transfer.net[1]
        W, Dg = _w2d(conv), rows.shape[1]
        per_anchor = K.linear(anchors, W[:, Dg:].contiguous(), conv.bias)
        x = K.batch_norm_act(K.linear_group_add(rows, W[:, :Dg].contiguous(), per_anchor, k), bn, self.training, relu=True)
        for block in self.operation:
            x = block.rows(x)
        return K.group_max(x, k)

    def forward(self, x):
        """x [B,S,k,d] (LocalGrouper's output) -> [B, out, S]"""
        B, S, k, d = x.shape
        Dg = d - self.channels
        x = x.reshape(B * S * k, d)
        anchors = x.view(B * S, k, d)[:, 0, Dg:].contiguous()
        return self.rows(x[:, :Dg].contiguous(), anchors, k).view(B, S, -1).transpose(1, 2)


class PosExtraction(nn.Module):
    def __init__(self, channels, blocks=1, groups=1, res_expansion=1, bias=True, activation="relu"):
        super().__init__()
        self.operation = nn.Sequential(*[ConvBNReLURes1D(channels, groups=groups, res_expansion=res_expansion, bias=bias, activation=activation)
                                         for _ in range(blocks)])

    def rows(self, x):
        for block in self.operation:
            x = block.rows(x)
        return x

    def forward(self, x):
        B, C, N = x.shape
        return self.rows(x.transpose(1, 2).reshape(B * N, C)).view(B, N, C).transpose(1, 2)


class Model(nn.Module):
    def __init__(self, points=1024, class_num=40, embed_dim=64, groups=1, res_expansion=1.0, activation="relu", bias=True, use_xyz=True,
                 normalize="center", dim_expansion=(2, 2, 2, 2), pre_blocks=(2, 2, 2, 2), pos_blocks=(2, 2, 2, 2), k_neighbors=(32, 32, 32, 32),
                 reducers=(2, 2, 2, 2), **kwargs):
        super().__init__()
        if not len(pre_blocks) == len(k_neighbors) == len(reducers) == len(pos_blocks) == len(dim_expansion):
            raise ValueError("pointmlp: dim_expansion, pre_blocks, pos_blocks, k_neighbors and reducers must have one entry per stage")
        self.stages, self.class_num, self.points = len(pre_blocks), class_num, int(points)
        self.embedding = ConvBNReLU1D(3, embed_dim, bias=bias, activation=activation)
        self.local_grouper_list, self.pre_blocks_list, self.pos_blocks_list = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        last, anchors = int(embed_dim), self.points
        for i in range(self.stages):
            out = last * int(dim_expansion[i])
            anchors = anchors // int(reducers[i])
            self.local_grouper_list.append(LocalGrouper(last, anchors, k_neighbors[i], use_xyz, normalize))
            self.pre_blocks_list.append(PreExtraction(last, out, pre_blocks[i], groups=groups, res_expansion=res_expansion, bias=bias,
                                                      activation=activation, use_xyz=use_xyz))
            self.pos_blocks_list.append(PosExtraction(out, pos_blocks[i], groups=groups, res_expansion=res_expansion, bias=bias, activation=activation))
            last = out
        self.act = _act(activation)
        self.classifier = nn.Sequential(nn.Linear(last, 512), nn.BatchNorm1d(512), self.act, nn.Dropout(0.5),
                                        nn.Linear(512, 256), nn.BatchNorm1d(256), self.act, nn.Dropout(0.5), nn.Linear(256, class_num))

    def forward_features(self, pts, draws=None):
        """pts [B,N,3] -> (logits, the [B, C] global feature the classifier reads)"""
        if pts.dim() != 3 or pts.shape[2] != 3:
            raise ValueError(f"pointmlp: pts: expected [B, N, 3], got {list(pts.shape)}")
        B, N, _ = pts.shape
        if N != self.points:
            raise ValueError(f"pointmlp: built for clouds of {self.points} points (the anchor counts derive from it), got {N}")
        xyz, tr, c = pts.contiguous(), self.training, self.classifier
        x = self.embedding.rows(xyz.reshape(B * N, 3)).view(B, N, -1)
        for i in range(self.stages):
            grouper = self.local_grouper_list[i]
            xyz, anchors, rows = grouper.rows(xyz, x, draws, i + 1)
            x = self.pos_blocks_list[i].rows(self.pre_blocks_list[i].rows(rows, anchors, grouper.kneighbors)).view(B, grouper.groups, -1)
        f = K.group_max(x.reshape(B * x.shape[1], -1), x.shape[1])
        h = K.batch_norm_act(K.linear(f, c[0].weight, c[0].bias), c[1], tr, relu=True)
        h = _dropout(h, c[3], tr, draws, "head.dp1")
        h = K.batch_norm_act(K.linear(h, c[4].weight, c[4].bias), c[5], tr, relu=True)
        h = _dropout(h, c[7], tr, draws, "head.dp2")
        return K.linear(h, c[8].weight, c[8].bias), f

    def forward(self, pts, draws=None):
        return self.forward_features(pts, draws)[0]


POINTMLP = dict(points=1024, embed_dim=64, groups=1, res_expansion=1.0, activation="relu", bias=False, use_xyz=False, normalize="anchor",
                dim_expansion=[2, 2, 2, 2], pre_blocks=[2, 2, 2, 2], pos_blocks=[2, 2, 2, 2], k_neighbors=[24, 24, 24, 24], reducers=[2, 2, 2, 2])
POINTMLP_ELITE = dict(POINTMLP, embed_dim=32, res_expansion=0.25, dim_expansion=[2, 2, 2, 1], pre_blocks=[1, 1, 2, 1], pos_blocks=[1, 1, 2, 1])


def pointmlp(num_classes=40, **kwargs):
    return Model(class_num=num_classes, **dict(POINTMLP, **kwargs))


def pointmlp_elite(num_classes=40, **kwargs):
    return Model(class_num=num_classes, **dict(POINTMLP_ELITE, **kwargs))


@MODELS.register_module()
class PointMLP(Model):
    """``pointmlp`` / ``pointmlp_elite`` behind the config interface of ``PointTransformer``: keys ``cls_dim``, ``variant`` (``pointmlp`` or ``elite``)
    and, optionally, any entry of the variant's table (``points``, ``embed_dim``, ``k_neighbors``, ...)"""

    def __init__(self, config, **kwargs):
        variant = config.get("variant", "pointmlp")
        if variant not in ("pointmlp", "elite"):
            raise ValueError(f"PointMLP: variant must be 'pointmlp' or 'elite', got {variant!r}")
        table = dict(POINTMLP if variant == "pointmlp" else POINTMLP_ELITE)
        table.update({k: config.get(k) for k in table if config.get(k) is not None})
        super().__init__(class_num=config.cls_dim, **table)
        self.config = config
        self.build_loss_func()

    def build_loss_func(self):
        self.loss_ce = nn.CrossEntropyLoss()          # kept for interface parity; get_loss_acc runs the HIP kernel

    def get_loss_acc(self, ret, gt):
        """-> (mean cross-entropy, top-1 accuracy in percent), both on the device, no host sync."""
        loss, acc = K.softmax_xent(ret, gt)
        return loss, acc * 100

    def load_model_from_ckpt(self, bert_ckpt_path, custom_loading=False):
        return _load(self, bert_ckpt_path, 'PointMLP')
