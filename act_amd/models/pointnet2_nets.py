"""The three standard PointNet++ networks on the HIP kernels, composed of models/pointnet2.py: the SSG classifier, the MSG part-segmentation
network and the SSG semantic-segmentation network (Qi et al. 2017; the layer tables of the widely used PyTorch port).

    pointnet2_cls_ssg      forward(pts [B,N,3|6])                  -> logits [B,cls_dim]              (MODELS: ``PointNet2_SSG``)
    pointnet2_part_seg_msg forward(pts [B,3|6,N], cls_label [B,16]) -> log-probabilities [B,N,num_part]
    pointnet2_sem_seg      forward(pts [B,in_channel,N])           -> log-probabilities [B,N,num_classes]

The two segmentation networks return what ``partseg.get_model`` / ``semseg.get_model`` return, so the runners' losses and evaluation take them
unchanged (``runner_partseg --model pointnet2_part_seg_msg``, ``runner_semseg --model pointnet2_sem_seg``).  Widths are fixed; the
``npoint`` / ``radius`` / ``nsample`` of every set-abstraction level can be overridden by keyword (``sa1=(npoint, radius, nsample)``; for the
MSG levels ``(npoint, radius_list, nsample_list)``).  ``state_dict`` names are the attribute names.  FPS starts at index 0; dropout masks come
from ``draws`` (keys ``head.drop1`` / ``head.drop2``) as in ``PointTransformer._head``.
"""
import torch
import torch.nn as nn

from .. import kernels as K
from ..utils.logger import print_log
from .build import MODELS
from .pointnet2 import PointNetSetAbstraction, PointNetSetAbstractionMsg, PointNetFeaturePropagationAny, _w2d

CLS_SA = dict(sa1=(512, 0.2, 32), sa2=(128, 0.4, 64))
PART_SA = dict(sa1=(512, [0.1, 0.2, 0.4], [32, 64, 128]), sa2=(128, [0.4, 0.8], [64, 128]))
SEM_SA = dict(sa1=(1024, 0.1, 32), sa2=(256, 0.2, 32), sa3=(64, 0.4, 32), sa4=(16, 0.8, 32))
NUM_CATEGORIES = 16


def _levels(name, default, over):
    unknown = sorted(set(over) - set(default))
    if unknown:
        raise ValueError(f"{name}: unknown keyword(s) {unknown}; the set-abstraction levels are {sorted(default)}")
    return {k: tuple(over.get(k, v)) for k, v in default.items()}


def _dropout(x, drop, training, draws, key):
    if not training or drop.p == 0:
        return x
    mk = lambda: (torch.rand_like(x) >= drop.p).to(x.dtype)
    keep = draws.get(key, mk) if draws is not None else mk()
    return x * (keep.to(x.device) / (1.0 - drop.p))


def _rows(x):
    """[B,C,N] -> rows [B*N,C]"""
    B, C, N = x.shape
    return x.transpose(1, 2).reshape(B * N, C)


def _load(model, path, logger):
    """a checkpoint of this model ({'model_state_dict' | 'base_model' | 'state_dict': ...} or a bare state_dict), loaded non-strictly"""
    if path is None:
        print_log('Training from scratch!!!', logger=logger)
        return None
    ckpt = torch.load(path, map_location='cpu')
    for key in ('model_state_dict', 'base_model', 'state_dict'):
        if isinstance(ckpt, dict) and key in ckpt:
            ckpt = ckpt[key]
            break
    incompatible = model.load_state_dict({k.replace('module.', ''): v for k, v in ckpt.items()}, strict=False)
    if incompatible.missing_keys:
        print_log(f'missing_keys: {incompatible.missing_keys}', logger=logger)
    if incompatible.unexpected_keys:
        print_log(f'unexpected_keys: {incompatible.unexpected_keys}', logger=logger)
    print_log(f'[{logger}] Successful Loading the ckpt from {path}', logger=logger)
    return incompatible


class pointnet2_cls_ssg(nn.Module):
    def __init__(self, cls_dim=40, normal_channel=False, **sa):
        super().__init__()
        lv = _levels("pointnet2_cls_ssg", CLS_SA, sa)
        self.cls_dim, self.normal_channel = cls_dim, bool(normal_channel)
        self.sa1 = PointNetSetAbstraction(*lv["sa1"], (3 if normal_channel else 0) + 3, [64, 64, 128], False)
        self.sa2 = PointNetSetAbstraction(*lv["sa2"], 128 + 3, [128, 128, 256], False)
        self.sa3 = PointNetSetAbstraction(None, None, None, 256 + 3, [256, 512, 1024], True)
        self.fc1, self.bn1, self.drop1 = nn.Linear(1024, 512), nn.BatchNorm1d(512), nn.Dropout(0.4)
        self.fc2, self.bn2, self.drop2 = nn.Linear(512, 256), nn.BatchNorm1d(256), nn.Dropout(0.4)
        self.fc3 = nn.Linear(256, cls_dim)

    def forward_features(self, pts, draws=None):
        """-> (logits, the [B,1024] global feature the head reads)"""
        want = 6 if self.normal_channel else 3
        if pts.dim() != 3 or pts.shape[2] != want:
            raise ValueError(f"pointnet2_cls_ssg: pts: expected [B, N, {want}], got {list(pts.shape)}")
        x = pts.transpose(1, 2)
        xyz, norm = x[:, :3], (x[:, 3:] if self.normal_channel else None)
        l1x, l1p = self.sa1(xyz, norm)
        l2x, l2p = self.sa2(l1x, l1p)
        _, l3p = self.sa3(l2x, l2p)
        f = l3p.reshape(pts.shape[0], 1024)
        h = K.batch_norm_act(K.linear(f, self.fc1.weight, self.fc1.bias), self.bn1, self.training, relu=True)
        h = _dropout(h, self.drop1, self.training, draws, "head.drop1")
        h = K.batch_norm_act(K.linear(h, self.fc2.weight, self.fc2.bias), self.bn2, self.training, relu=True)
        h = _dropout(h, self.drop2, self.training, draws, "head.drop2")
        return K.linear(h, self.fc3.weight, self.fc3.bias), f

    def forward(self, pts, draws=None):
        return self.forward_features(pts, draws)[0]


@MODELS.register_module()
class PointNet2_SSG(pointnet2_cls_ssg):
    """``pointnet2_cls_ssg`` behind the config interface of ``PointTransformer``: keys ``cls_dim``, ``normal_channel`` (default False) and the
    optional level overrides ``sa1`` / ``sa2`` = [npoint, radius, nsample]"""

    def __init__(self, config, **kwargs):
        sa = {k: tuple(config.get(k)) for k in CLS_SA if config.get(k) is not None}
        super().__init__(config.cls_dim, config.get("normal_channel", False), **sa)
        self.config = config
        self.build_loss_func()

    def build_loss_func(self):
        self.loss_ce = nn.CrossEntropyLoss()          # kept for interface parity; get_loss_acc runs the HIP kernel

    def get_loss_acc(self, ret, gt):
        """-> (mean cross-entropy, top-1 accuracy in percent), both on the device, no host sync."""
        loss, acc = K.softmax_xent(ret, gt)
        return loss, acc * 100

    def load_model_from_ckpt(self, bert_ckpt_path, custom_loading=False):
        return _load(self, bert_ckpt_path, 'PointNet2_SSG')


class _SegHead(nn.Module):
    """conv1 -> bn1 -> ReLU -> drop1 -> conv2 -> log-softmax over the classes, on rows"""

    def _seg_head(self, l0p, draws):
        B, _, N = l0p.shape
        h = K.batch_norm_act(K.linear(_rows(l0p), _w2d(self.conv1), self.conv1.bias), self.bn1, self.training, relu=True)
        h = _dropout(h, self.drop1, self.training, draws, "head.drop1")
        z = K.linear(h, _w2d(self.conv2), self.conv2.bias)
        return K.log_softmax(z).view(B, N, -1)

    def load_model_from_ckpt(self, path):
        return _load(self, path, type(self).__name__)


class pointnet2_part_seg_msg(_SegHead):
    def __init__(self, num_part=50, normal_channel=False, **sa):
        super().__init__()
        lv = _levels("pointnet2_part_seg_msg", PART_SA, sa)
        extra = 3 if normal_channel else 0
        self.num_part, self.normal_channel = num_part, bool(normal_channel)
        self.sa1 = PointNetSetAbstractionMsg(*lv["sa1"], 3 + extra, [[32, 32, 64], [64, 64, 128], [64, 96, 128]])
        self.sa2 = PointNetSetAbstractionMsg(*lv["sa2"], 128 + 128 + 64, [[128, 128, 256], [128, 196, 256]])
        self.sa3 = PointNetSetAbstraction(None, None, None, 512 + 3, [256, 512, 1024], True)
        self.fp3 = PointNetFeaturePropagationAny(1536, [256, 256])
        self.fp2 = PointNetFeaturePropagationAny(576, [256, 128])
        self.fp1 = PointNetFeaturePropagationAny(150 + extra, [128, 128])
        self.conv1, self.bn1, self.drop1 = nn.Conv1d(128, 128, 1), nn.BatchNorm1d(128), nn.Dropout(0.5)
        self.conv2 = nn.Conv1d(128, num_part, 1)

    def forward(self, pts, cls_label, draws=None):
        """pts [B,3|6,N], cls_label [B,16] or [B,1,16] (one-hot category) -> log-probabilities [B,N,num_part]"""
        want = 6 if self.normal_channel else 3
        if pts.dim() != 3 or pts.shape[1] != want:
            raise ValueError(f"pointnet2_part_seg_msg: pts: expected [B, {want}, N], got {list(pts.shape)}")
        B, _, N = pts.shape
        l0p, l0x = pts, pts[:, :3]
        l1x, l1p = self.sa1(l0x, l0p)
        l2x, l2p = self.sa2(l1x, l1p)
        l3x, l3p = self.sa3(l2x, l2p)
        l2p = self.fp3(l2x, l3x, l2p, l3p)
        l1p = self.fp2(l1x, l2x, l1p, l2p)
        onehot = cls_label.reshape(B, NUM_CATEGORIES, 1).to(torch.float32).expand(B, NUM_CATEGORIES, N)
        l0p = self.fp1(l0x, l1x, torch.cat((onehot, l0x, l0p), dim=1), l1p)
        return self._seg_head(l0p, draws)


class pointnet2_sem_seg(_SegHead):
    """``in_channel`` (default 9: xyz, rgb, room-normalised xyz) is the number of input channels, the first three of which are xyz; the project's
    S3DIS blocks carry xyz only, so ``runner_semseg`` builds the network with ``in_channel=3``."""

    def __init__(self, num_classes=13, in_channel=9, **sa):
        super().__init__()
        lv = _levels("pointnet2_sem_seg", SEM_SA, sa)
        if in_channel < 3:
            raise ValueError(f"pointnet2_sem_seg: in_channel must be >= 3 (xyz first), got {in_channel}")
        self.num_classes, self.in_channel = num_classes, in_channel
        self.sa1 = PointNetSetAbstraction(*lv["sa1"], in_channel + 3, [32, 32, 64], False)
        self.sa2 = PointNetSetAbstraction(*lv["sa2"], 64 + 3, [64, 64, 128], False)
        self.sa3 = PointNetSetAbstraction(*lv["sa3"], 128 + 3, [128, 128, 256], False)
        self.sa4 = PointNetSetAbstraction(*lv["sa4"], 256 + 3, [256, 256, 512], False)
        self.fp4 = PointNetFeaturePropagationAny(768, [256, 256])
        self.fp3 = PointNetFeaturePropagationAny(384, [256, 256])
        self.fp2 = PointNetFeaturePropagationAny(320, [256, 128])
        self.fp1 = PointNetFeaturePropagationAny(128, [128, 128, 128])
        self.conv1, self.bn1, self.drop1 = nn.Conv1d(128, 128, 1), nn.BatchNorm1d(128), nn.Dropout(0.5)
        self.conv2 = nn.Conv1d(128, num_classes, 1)

    def forward(self, pts, draws=None):
        """pts [B,in_channel,N] -> log-probabilities [B,N,num_classes]"""
        if pts.dim() != 3 or pts.shape[1] != self.in_channel:
            raise ValueError(f"pointnet2_sem_seg: pts: expected [B, {self.in_channel}, N], got {list(pts.shape)}")
        l0p, l0x = pts, pts[:, :3]
        l1x, l1p = self.sa1(l0x, l0p)
        l2x, l2p = self.sa2(l1x, l1p)
        l3x, l3p = self.sa3(l2x, l2p)
        l4x, l4p = self.sa4(l3x, l3p)
        l3p = self.fp4(l3x, l4x, l3p, l4p)
        l2p = self.fp3(l2x, l3x, l2p, l3p)
        l1p = self.fp2(l1x, l2x, l1p, l2p)
        l0p = self.fp1(l0x, l1x, None, l1p)
        return self._seg_head(l0p, draws)
