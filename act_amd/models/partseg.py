"""ShapeNetPart part segmentation on the ACT encoder (reference: part_segmentation/models/pt.py).

``part_segmentation/models/pt.py`` is the semantic-segmentation model plus a category label branch, so this module is ``semseg.get_model`` with
``LABEL_DIM = 16``: the same features (Group -> mini-PointNet -> blocks 3, 7, 11 -> LayerNorm), the same three-NN feature propagation and the same
head, with

  label_conv_cls = Sequential(Conv1d(16, 64, 1, bias=False), BatchNorm1d(64), LeakyReLU(0.2)) on the category rows [B, 16] -- one HIP launch
  (kernels.label_branch); its BatchNorm takes batch statistics over the B clouds, as the reference's does on [B, 16, 1] before the repeat over N
  -> global feature cat(max, mean, label feature) [B, 2368], so convs1_cls is Conv1d(3392, 512, 1) and its 2,368 per-cloud columns run once per
  cloud, added in the GEMM epilogue of the 1,024 per-point columns.

The ``state_dict`` keys, shapes and order are the reference's (label_conv_cls between norm and propagation_0_cls).  ACT_SEG_FP_PERGROUP selects the
form of the first propagation conv here as in semseg.
"""
import torch
import torch.nn as nn

from .. import kernels as K
from . import semseg

NUM_CATEGORIES = 16


def to_categorical(y, num_classes):
    """1-hot rows of the category ids ``y`` (any shape) -> float32 [*y.shape, num_classes] on y's device (main.py to_categorical, without the
    round trip through numpy)"""
    y = torch.as_tensor(y)
    return torch.eye(num_classes, dtype=torch.float32, device=y.device)[y.long()]


class get_model(semseg.get_model):
    LABEL_DIM = NUM_CATEGORIES
    LOGGER = "PartSeg"

    def __init__(self, cls_dim=50):
        super().__init__(cls_dim)

    def forward(self, pts, cls_label, draws=None, pergroup=None):
        """pts [B, 3, N] (the reference's layout), cls_label [B, 1, 16] (to_categorical of the category; any [B, 16] values) -> log-probabilities
        [B, N, cls_dim]"""
        B = pts.shape[0]
        xyz = pts.transpose(1, 2).contiguous()
        x, center = self.features(xyz, draws)
        lc = self.label_conv_cls
        lab = K.label_branch(cls_label.reshape(B, self.LABEL_DIM).to(torch.float32), lc[0], lc[1], lc[2], self.training)
        return self.head(xyz, x, center, (lab,), draws, pergroup)


class get_loss(nn.Module):
    """F.nll_loss(pred, target): unweighted mean of -logp[target] (deterministic device reduction)"""

    def forward(self, pred, target):
        C = pred.shape[-1]
        loss, _ = K.nll_weighted(pred.reshape(-1, C), target.reshape(-1), None)
        return loss

    @staticmethod
    def with_correct(pred, target):
        """-> (loss, number of points whose unmasked arg-max equals the target), both on the device"""
        C = pred.shape[-1]
        return K.nll_weighted(pred.reshape(-1, C), target.reshape(-1), None)
