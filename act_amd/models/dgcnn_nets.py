"""The DGCNN classifier (Wang et al. 2019; the layer table of the widely used PyTorch port) on the HIP kernels of csrc/edgeconv.hip.

    EdgeConv   forward(x [B,N,C], idx=None)   -> [B,N,out]       one dynamic-graph layer: kNN in the layer's own features, edge convolution,
                                                                BatchNorm over all B*N*k edges, LeakyReLU(0.2), max over the k neighbours
    dgcnn_cls  forward(pts [B,N,3])           -> logits [B,cls_dim]                               (MODELS: ``DGCNN_cls``)

The edge convolution W . cat(x_j - x_i, x_i) is evaluated per POINT: with W = [W1 | W2], W . cat(x_j - x_i, x_i) = W1 x_j + (W2 - W1) x_i, so one
``K.linear`` onto [B*N, 2*out] gives P = x W1^T and Q = x (W2 - W1)^T (1/k of the per-edge FLOPs), and ``K.edge_conv_bn`` forms P[idx] + Q, the
statistics, the activation and the max without an edge tensor.  ``state_dict`` has upstream's keys and shapes (``bn1`` .. ``bn7``, ``conv1`` ..
``conv5`` as Sequential(conv, bn, LeakyReLU) sharing the ``bnX`` modules, ``linear1`` .. ``linear3``), so an upstream checkpoint loads with
``strict=True``; the forward calls the kernels, never the Sequentials.  Everything random or discrete is injectable: the four neighbour lists go
through ``draws`` keys ``knn.1`` .. ``knn.4``, the dropout masks through ``head.dp1`` / ``head.dp2``.
"""
import torch
import torch.nn as nn

from .. import kernels as K
from .build import MODELS
from .pointnet2_nets import _dropout, _load

SLOPE = 0.2


def _no_sync(bn, who):
    if K._sync_group(bn) is not None:
        raise NotImplementedError(f"{who}: SyncBatchNorm across ranks is not implemented for the EdgeConv BatchNorm")


def edge_conv(x, idx, conv, bn, k, training, validate=True):
    """x [B,N,C], idx int [B,N,k] -> [B,N,out] with the weights of ``conv`` (Conv2d(2C, out, 1, bias=False), columns (x_j - x_i | x_i)) and ``bn``"""
    B, N, C = x.shape
    out = conv.weight.shape[0]
    if conv.weight.shape[1] != 2 * C:
        raise ValueError(f"edge_conv: the convolution takes {conv.weight.shape[1]} = 2 * {conv.weight.shape[1] // 2} channels, x has {C}")
    _no_sync(bn, "edge_conv")
    W = conv.weight.view(out, 2 * C)
    Wpq = torch.cat((W[:, :C], W[:, C:] - W[:, :C]), dim=0)                      # [2*out, C]: rows of P, then rows of Q
    pq = K.linear(x.reshape(B * N, C), Wpq)
    return K.edge_conv_bn(pq, out, idx, B, N, k, out, bn, training, slope=SLOPE, validate=validate).view(B, N, out)


class EdgeConv(nn.Module):
    def __init__(self, in_channel, out_channel, k):
        super().__init__()
        self.k = int(k)
        self.conv = nn.Conv2d(2 * in_channel, out_channel, kernel_size=1, bias=False)
        self.bn = nn.BatchNorm2d(out_channel)

    def forward(self, x, idx=None):
        made = idx is None
        if made:
            idx = K.knn_features(x, self.k)
        return edge_conv(x, idx, self.conv, self.bn, idx.shape[2], self.training, validate=not made)


class dgcnn_cls(nn.Module):
    def __init__(self, cls_dim=40, k=20, emb_dims=1024, dropout=0.5, widths=(64, 64, 128, 256)):
        super().__init__()
        widths = tuple(int(w) for w in widths)
        if len(widths) != 4 or any(w < 4 or w % 4 for w in widths):
            raise ValueError(f"dgcnn_cls: widths must be four multiples of 4, got {widths}")
        self.cls_dim, self.k, self.emb_dims, self.widths = cls_dim, int(k), int(emb_dims), widths
        self.bn1, self.bn2, self.bn3, self.bn4 = (nn.BatchNorm2d(w) for w in widths)
        self.bn5 = nn.BatchNorm1d(emb_dims)
        cin = (3,) + widths[:3]
        act = lambda: nn.LeakyReLU(negative_slope=SLOPE)
        self.conv1 = nn.Sequential(nn.Conv2d(2 * cin[0], widths[0], kernel_size=1, bias=False), self.bn1, act())
        self.conv2 = nn.Sequential(nn.Conv2d(2 * cin[1], widths[1], kernel_size=1, bias=False), self.bn2, act())
        self.conv3 = nn.Sequential(nn.Conv2d(2 * cin[2], widths[2], kernel_size=1, bias=False), self.bn3, act())
        self.conv4 = nn.Sequential(nn.Conv2d(2 * cin[3], widths[3], kernel_size=1, bias=False), self.bn4, act())
        self.conv5 = nn.Sequential(nn.Conv1d(sum(widths), emb_dims, kernel_size=1, bias=False), self.bn5, act())
        self.linear1 = nn.Linear(2 * emb_dims, 512, bias=False)
        self.bn6 = nn.BatchNorm1d(512)
        self.dp1 = nn.Dropout(p=dropout)
        self.linear2 = nn.Linear(512, 256)
        self.bn7 = nn.BatchNorm1d(256)
        self.dp2 = nn.Dropout(p=dropout)
        self.linear3 = nn.Linear(256, cls_dim)

    def forward_features(self, pts, draws=None):
        """-> (logits, the [B, 2*emb_dims] global feature cat(max, mean) the head reads)"""
        if pts.dim() != 3 or pts.shape[2] != 3:
            raise ValueError(f"dgcnn_cls: pts: expected [B, N, 3], got {list(pts.shape)}")
        B, N, _ = pts.shape
        x, feats = pts.contiguous(), []
        for i, seq in enumerate((self.conv1, self.conv2, self.conv3, self.conv4), 1):
            make = lambda x=x: K.knn_features(x, self.k)
            idx = draws.get(f"knn.{i}", make) if draws is not None else make()
            x = edge_conv(x, idx.to(pts.device), seq[0], seq[1], self.k, self.training, validate=False)
            feats.append(x)
        rows = torch.cat(feats, dim=2).reshape(B * N, sum(self.widths))
        w5 = self.conv5[0].weight
        h = K.batch_norm_act(K.linear(rows, w5.view(w5.shape[0], w5.shape[1])), self.bn5, self.training, slope=SLOPE)
        f = torch.cat((K.group_max(h, N), K.group_mean(h, N)), dim=1)
        h = K.batch_norm_act(K.linear(f, self.linear1.weight), self.bn6, self.training, slope=SLOPE)
        h = _dropout(h, self.dp1, self.training, draws, "head.dp1")
        h = K.batch_norm_act(K.linear(h, self.linear2.weight, self.linear2.bias), self.bn7, self.training, slope=SLOPE)
        h = _dropout(h, self.dp2, self.training, draws, "head.dp2")
        return K.linear(h, self.linear3.weight, self.linear3.bias), f

    def forward(self, pts, draws=None):
        return self.forward_features(pts, draws)[0]


@MODELS.register_module()
class DGCNN_cls(dgcnn_cls):
    """``dgcnn_cls`` behind the config interface of ``PointTransformer``: keys ``cls_dim``, ``k`` (20), ``emb_dims`` (1024), ``dropout`` (0.5)"""

    def __init__(self, config, **kwargs):
        super().__init__(config.cls_dim, config.get("k", 20), config.get("emb_dims", 1024), config.get("dropout", 0.5))
        self.config = config
        self.build_loss_func()

    def build_loss_func(self):
        self.loss_ce = nn.CrossEntropyLoss()          # kept for interface parity; get_loss_acc runs the HIP kernel

    def get_loss_acc(self, ret, gt):
        """-> (mean cross-entropy, top-1 accuracy in percent), both on the device, no host sync."""
        loss, acc = K.softmax_xent(ret, gt)
        return loss, acc * 100

    def load_model_from_ckpt(self, bert_ckpt_path, custom_loading=False):
        return _load(self, bert_ckpt_path, 'DGCNN_cls')
