"""The DGCNN networks (Wang et al. 2019; the layer tables of the widely used PyTorch port) on the HIP kernels of csrc/edgeconv.hip and
csrc/edge_mlp2.hip.

    EdgeConv   forward(x [B,N,C], idx=None)   -> [B,N,out]       one dynamic-graph layer: kNN in the layer's own features, edge convolution,
                                                                BatchNorm over all B*N*k edges, LeakyReLU(0.2), max over the k neighbours
    dgcnn_cls  forward(pts [B,N,3])           -> logits [B,cls_dim]                               (MODELS: ``DGCNN_cls``)
    dgcnn_partseg  forward(pts [B,3,N], onehot [B,16])  -> log-probabilities [B,N,seg_num_all]     (``runner_partseg --model dgcnn_partseg``)
    dgcnn_semseg   forward(pts [B,in_channel,N])        -> log-probabilities [B,N,num_classes]     (``runner_semseg --model dgcnn_semseg``)

The edge convolution W . cat(x_j - x_i, x_i) is evaluated per POINT: with W = [W1 | W2], W . cat(x_j - x_i, x_i) = W1 x_j + (W2 - W1) x_i, so one
``K.linear`` onto [B*N, 2*out] gives P = x W1^T and Q = x (W2 - W1)^T (1/k of the per-edge FLOPs), and ``K.edge_conv_bn`` forms P[idx] + Q, the
statistics, the activation and the max without an edge tensor.  ``state_dict`` has upstream's keys and shapes (``bn1`` .. ``bn7``, ``conv1`` ..
``conv5`` as Sequential(conv, bn, LeakyReLU) sharing the ``bnX`` modules, ``linear1`` .. ``linear3``), so an upstream checkpoint loads with
``strict=True``; the forward calls the kernels, never the Sequentials.  Everything random or discrete is injectable: the four neighbour lists go
through ``draws`` keys ``knn.1`` .. ``knn.4``, the dropout masks through ``head.dp1`` / ``head.dp2``.

The segmentation networks and the part network's spatial transformer put TWO convolutions ahead of the max over the neighbours.  The first still
collapses to P[idx] + Q; the second is a per-edge product, which ``K.edge_mlp2_bn`` forms tile by tile on the matrix cores (``edge_conv2``).  The
convolution that follows the global max-pool reads cat(repeat(global feature), x1, x2, x3): its repeated columns are evaluated once per cloud and
added in the GEMM epilogue (``K.linear_group_add``).  Their lists are ``knn.t`` (the transformer's graph, part network only) and ``knn.1`` ..
``knn.3``.
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


# ---- the segmentation networks --------------------------------------------------------------------------------------------------------------------------
def _pq_of(x, conv):
    """x [B,N,C], conv Conv2d(2C, out, 1, bias=False) on cat(x_j - x_i, x_i) -> pq [B*N, 2*out] = [P | Q]"""
    B, N, C = x.shape
    out = conv.weight.shape[0]
    if conv.weight.shape[1] != 2 * C:
        raise ValueError(f"edge_conv2: the convolution takes {conv.weight.shape[1]} = 2 * {conv.weight.shape[1] // 2} channels, x has {C}")
    W = conv.weight.view(out, 2 * C)
    return K.linear(x.reshape(B * N, C), torch.cat((W[:, :C], W[:, C:] - W[:, :C]), dim=0))


def edge_conv2(x, idx, conv_a, bn_a, conv_b, bn_b, k, training, validate=True):
    """x [B,N,C], idx int [B,N,k] -> [B,N,out]: conv_a (Conv2d(2C, mid)) / bn_a / LeakyReLU / conv_b (Conv2d(mid, out)) / bn_b / LeakyReLU / max over k"""
    B, N, _ = x.shape
    mid, out = conv_a.weight.shape[0], conv_b.weight.shape[0]
    return K.edge_mlp2_bn(_pq_of(x, conv_a), mid, idx, B, N, k, mid, bn_a, conv_b.weight.view(out, mid), bn_b, training, slope=SLOPE,
                          validate=validate).view(B, N, out)


def _seq2(cin, cout, bn):
    return nn.Sequential(nn.Conv2d(cin, cout, kernel_size=1, bias=False), bn, nn.LeakyReLU(negative_slope=SLOPE))


def _seq1(cin, cout, bn):
    return nn.Sequential(nn.Conv1d(cin, cout, kernel_size=1, bias=False), bn, nn.LeakyReLU(negative_slope=SLOPE))


def _rows_conv(rows, seq, training):
    """Sequential(Conv1d(cin, cout, 1, bias=False), BatchNorm1d, LeakyReLU) on rows [R, cin]"""
    w = seq[0].weight
    return K.batch_norm_act(K.linear(rows, w.view(w.shape[0], w.shape[1])), seq[1], training, slope=SLOPE)


def _widths(who, widths, n):
    widths = tuple(int(w) for w in widths)
    if len(widths) != n or any(w < 4 or w % 4 for w in widths):
        raise ValueError(f"{who}: widths must be {n} multiples of 4, got {widths}")
    return widths


def _knn(draws, key, x, k):
    make = lambda: K.knn_features(x, k)
    return (draws.get(key, make) if draws is not None else make()).to(x.device)


class Transform_Net(nn.Module):
    """the spatial transformer of the part network: graph feature of the raw xyz -> a 3x3 matrix per cloud.  ``bn3`` is BatchNorm1d(512): upstream
    assigns the attribute twice, so conv3's own BatchNorm1d(1024) is reachable only as ``conv3.1``."""

    def __init__(self, widths=(64, 128, 1024, 512, 256)):
        super().__init__()
        w = self.widths = _widths("Transform_Net", widths, 5)
        self.bn1, self.bn2 = nn.BatchNorm2d(w[0]), nn.BatchNorm2d(w[1])
        self.conv1, self.conv2 = _seq2(6, w[0], self.bn1), _seq2(w[0], w[1], self.bn2)
        self.conv3 = _seq1(w[1], w[2], nn.BatchNorm1d(w[2]))
        self.linear1 = nn.Linear(w[2], w[3], bias=False)
        self.bn3 = nn.BatchNorm1d(w[3])
        self.linear2 = nn.Linear(w[3], w[4], bias=False)
        self.bn4 = nn.BatchNorm1d(w[4])
        self.transform = nn.Linear(w[4], 9)
        nn.init.constant_(self.transform.weight, 0)
        nn.init.eye_(self.transform.bias.view(3, 3))

    def forward(self, x, idx):
        """x [B,N,3], idx [B,N,k] -> T [B,3,3]"""
        B, N, _ = x.shape
        h = edge_conv2(x, idx, self.conv1[0], self.bn1, self.conv2[0], self.bn2, idx.shape[2], self.training, validate=False)
        g = K.group_max(_rows_conv(h.reshape(B * N, -1), self.conv3, self.training), N)
        h = K.batch_norm_act(K.linear(g, self.linear1.weight), self.bn3, self.training, slope=SLOPE)
        h = K.batch_norm_act(K.linear(h, self.linear2.weight), self.bn4, self.training, slope=SLOPE)
        return K.linear(h, self.transform.weight, self.transform.bias).view(B, 3, 3)


class _DgcnnSeg(nn.Module):
    def _trunk(self, x, draws, first_graph=None):
        """x [B,N,C] -> (x1, x2, x3 [B,N,w], the global max [B,emb]) through conv1 .. conv6"""
        B, N, _ = x.shape
        k, tr = self.k, self.training
        idx = _knn(draws, "knn.1", x if first_graph is None else first_graph, k)
        x1 = edge_conv2(x, idx, self.conv1[0], self.bn1, self.conv2[0], self.bn2, k, tr, validate=False)
        x2 = edge_conv2(x1, _knn(draws, "knn.2", x1, k), self.conv3[0], self.bn3, self.conv4[0], self.bn4, k, tr, validate=False)
        x3 = edge_conv(x2, _knn(draws, "knn.3", x2, k), self.conv5[0], self.bn5, k, tr, validate=False)
        rows = torch.cat((x1, x2, x3), dim=2).reshape(B * N, -1)
        return rows, K.group_max(_rows_conv(rows, self.conv6, tr), N)

    def _fused_cat_conv(self, g, rows, seq, N):
        """seq on cat(repeat(g [B,G]), rows [B*N,W]): the G repeated columns once per cloud, added in the epilogue of the per-point product"""
        w = seq[0].weight.view(seq[0].weight.shape[0], -1)
        G = g.shape[1]
        per_cloud = K.linear(g, w[:, :G].contiguous())
        return K.batch_norm_act(K.linear_group_add(rows, w[:, G:].contiguous(), per_cloud, N), seq[1], self.training, slope=SLOPE)

    def load_model_from_ckpt(self, ckpt_path, custom_loading=False):
        return _load(self, ckpt_path, type(self).__name__)


class dgcnn_partseg(_DgcnnSeg):
    """``widths``: conv1 .. conv5; ``head``: conv8, conv9, conv10; ``tnet``: the widths of Transform_Net (tiny variants for the tests)"""

    def __init__(self, seg_num_all=50, k=40, emb_dims=1024, dropout=0.5, widths=(64, 64, 64, 64, 64), head=(256, 256, 128), tnet=(64, 128, 1024, 512, 256)):
        super().__init__()
        w, hd = _widths("dgcnn_partseg", widths, 5), _widths("dgcnn_partseg", head, 3)
        self.seg_num_all, self.k, self.emb_dims, self.widths = seg_num_all, int(k), int(emb_dims), w
        self.transform_net = Transform_Net(tnet)
        self.bn1, self.bn2, self.bn3, self.bn4, self.bn5 = (nn.BatchNorm2d(c) for c in w)
        self.bn6, self.bn7 = nn.BatchNorm1d(emb_dims), nn.BatchNorm1d(64)
        self.bn8, self.bn9, self.bn10 = (nn.BatchNorm1d(c) for c in hd)
        self.conv1, self.conv2 = _seq2(6, w[0], self.bn1), _seq2(w[0], w[1], self.bn2)
        self.conv3, self.conv4 = _seq2(2 * w[1], w[2], self.bn3), _seq2(w[2], w[3], self.bn4)
        self.conv5 = _seq2(2 * w[3], w[4], self.bn5)
        self.conv6 = _seq1(w[1] + w[3] + w[4], emb_dims, self.bn6)
        self.conv7 = _seq1(16, 64, self.bn7)
        self.conv8 = _seq1(emb_dims + 64 + w[1] + w[3] + w[4], hd[0], self.bn8)
        self.dp1 = nn.Dropout(p=dropout)
        self.conv9 = _seq1(hd[0], hd[1], self.bn9)
        self.dp2 = nn.Dropout(p=dropout)
        self.conv10 = _seq1(hd[1], hd[2], self.bn10)
        self.conv11 = nn.Conv1d(hd[2], seg_num_all, kernel_size=1, bias=False)

    def forward(self, pts, onehot, draws=None):
        """pts [B,3,N], onehot [B,16] or [B,1,16] (the category) -> log-probabilities [B,N,seg_num_all]"""
        if pts.dim() != 3 or pts.shape[1] != 3:
            raise ValueError(f"dgcnn_partseg: pts: expected [B, 3, N], got {list(pts.shape)}")
        B, _, N = pts.shape
        tr = self.training
        x0 = pts.transpose(1, 2).contiguous()
        T = self.transform_net(x0, _knn(draws, "knn.t", x0, self.k))
        x = K.cloud_transform3(x0, T)
        rows, g = self._trunk(x, draws)
        lab = K.label_branch(onehot.reshape(B, 16).to(torch.float32), self.conv7[0], self.bn7, self.conv7[2], tr)
        h = self._fused_cat_conv(torch.cat((g, lab), dim=1), rows, self.conv8, N)
        h = _rows_conv(_dropout(h, self.dp1, tr, draws, "head.dp1"), self.conv9, tr)
        h = _rows_conv(_dropout(h, self.dp2, tr, draws, "head.dp2"), self.conv10, tr)
        w = self.conv11.weight
        return K.log_softmax(K.linear(h, w.view(w.shape[0], w.shape[1]))).view(B, N, self.seg_num_all)


class dgcnn_semseg(_DgcnnSeg):
    """``widths``: conv1 .. conv5; ``head``: conv7, conv8.  The first graph is searched on the last three channels when ``in_channel`` is 9 (the
    room-normalised xyz of the S3DIS blocks, upstream's rule), otherwise on all channels."""

    def __init__(self, num_classes=13, in_channel=9, k=20, emb_dims=1024, dropout=0.5, widths=(64, 64, 64, 64, 64), head=(512, 256)):
        super().__init__()
        w, hd = _widths("dgcnn_semseg", widths, 5), _widths("dgcnn_semseg", head, 2)
        if in_channel < 1:
            raise ValueError(f"dgcnn_semseg: in_channel must be >= 1, got {in_channel}")
        self.num_classes, self.in_channel, self.k, self.emb_dims, self.widths = num_classes, int(in_channel), int(k), int(emb_dims), w
        self.bn1, self.bn2, self.bn3, self.bn4, self.bn5 = (nn.BatchNorm2d(c) for c in w)
        self.bn6 = nn.BatchNorm1d(emb_dims)
        self.bn7, self.bn8 = (nn.BatchNorm1d(c) for c in hd)
        self.conv1, self.conv2 = _seq2(2 * in_channel, w[0], self.bn1), _seq2(w[0], w[1], self.bn2)
        self.conv3, self.conv4 = _seq2(2 * w[1], w[2], self.bn3), _seq2(w[2], w[3], self.bn4)
        self.conv5 = _seq2(2 * w[3], w[4], self.bn5)
        self.conv6 = _seq1(w[1] + w[3] + w[4], emb_dims, self.bn6)
        self.conv7 = _seq1(emb_dims + w[1] + w[3] + w[4], hd[0], self.bn7)
        self.conv8 = _seq1(hd[0], hd[1], self.bn8)
        self.dp1 = nn.Dropout(p=dropout)
        self.conv9 = nn.Conv1d(hd[1], num_classes, kernel_size=1, bias=False)

    def forward(self, pts, draws=None):
        """pts [B,in_channel,N] -> log-probabilities [B,N,num_classes]"""
        if pts.dim() != 3 or pts.shape[1] != self.in_channel:
            raise ValueError(f"dgcnn_semseg: pts: expected [B, {self.in_channel}, N], got {list(pts.shape)}")
        B, _, N = pts.shape
        tr = self.training
        x = pts.transpose(1, 2).contiguous()
        rows, g = self._trunk(x, draws, first_graph=x[:, :, 6:].contiguous() if self.in_channel == 9 else None)
        h = _rows_conv(self._fused_cat_conv(g, rows, self.conv7, N), self.conv8, tr)
        w = self.conv9.weight
        return K.log_softmax(K.linear(_dropout(h, self.dp1, tr, draws, "head.dp1"), w.view(w.shape[0], w.shape[1]))).view(B, N, self.num_classes)
