"""S3DIS semantic segmentation on the ACT encoder (reference: semantic_segmentation/models/pt.py, models/pointnet2_utils.py:262-315).

Same public names (``get_model``, ``get_loss``, ``PointNetFeaturePropagation``) and the same ``state_dict`` keys and shapes as the reference, so
reference checkpoints and ACT pretraining checkpoints load unchanged.  Every layer runs on the HIP kernels:

  Group (FPS + kNN) -> mini-PointNet Encoder(384) -> 12 blocks (no cls token), the outputs of blocks 3, 7, 11 kept (one BlockStackFn per chunk
  of 4 blocks: each chunk's output IS a kept output) -> shared LayerNorm -> x [B*G, 1152]
  -> global feature cat(max over G, mean over G) [B, 2304]
  -> PointNetFeaturePropagation(1155, [1536, 1024]): three nearest centres (difference-form distances), inverse-distance weights,
     first conv on cat(xyz, interp(x)) + BN + ReLU, second conv + BN + ReLU
  -> convs1_cls on cat(f_level_0, global): the per-point 1024 columns through the GEMM, the per-cloud 2304 columns once per cloud and added in
     the GEMM epilogue -> BN, ReLU, Dropout(0.5) -> convs2_cls, BN, ReLU -> convs3_cls -> log_softmax, returned as [B, N, cls_dim].

First propagation conv, default (ACT_SEG_FP_PERGROUP=1): W_f . sum_k w_k x[idx_k] = sum_k w_k (W_f . x)[idx_k], so P = x . W_f^T is computed once
per centre (B*G rows) and interpolated with the xyz columns and the bias in one kernel -- 16x fewer FLOPs in the largest product of the head.
ACT_SEG_FP_PERGROUP=0 keeps the plain form (interpolate the 1152 features, then the 1155-wide GEMM) for A/B runs and the parity tests.
"""
import os

import torch
import torch.nn as nn

from .. import kernels as K
from ..utils.logger import print_log
from .act import TransformerEncoder, stack_gates
from .dvae import Group, Encoder, trunc_normal_

FP_PERGROUP = os.environ.get("ACT_SEG_FP_PERGROUP", "1") != "0"
FETCH = (3, 7, 11)              # blocks whose outputs the head reads (semantic_segmentation/models/pt.py TransformerEncoder.forward)


def _w2d(conv):
    w = conv.weight
    return w.view(w.shape[0], w.shape[1])


class PointNetFeaturePropagation(nn.Module):
    """pointnet2_utils.PointNetFeaturePropagation with the reference's parameters (mlp_convs / mlp_bns).  ``forward`` takes the row layout of
    this package: xyz [B,N,3] (the points, also points1), center [B,G,3], x [B*G,D] (points2 as rows) -> [B*N, mlp[-1]]."""

    def __init__(self, in_channel, mlp):
        super().__init__()
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last = in_channel
        for out in mlp:
            self.mlp_convs.append(nn.Conv1d(last, out, 1))
            self.mlp_bns.append(nn.BatchNorm1d(out))
            last = out

    def forward(self, xyz, center, x, nn3=None, pergroup=None):
        B, N, _ = xyz.shape
        G = center.shape[1]
        if nn3 is None:
            nn3 = K.three_nn(xyz, center, want_adj=torch.is_grad_enabled())    # the inverse adjacency serves the backward only
        pergroup = FP_PERGROUP if pergroup is None else pergroup
        xyz2 = xyz.reshape(B * N, 3).contiguous()
        c0 = self.mlp_convs[0]
        if pergroup:
            h = K.interp_conv(x, _w2d(c0), c0.bias, xyz2, nn3, B, N, G)
        else:
            h = K.linear(torch.cat((xyz2, K.interp_rows(x, nn3, B, N, G)), dim=1), _w2d(c0), c0.bias)
        h = K.batch_norm_act(h, self.mlp_bns[0], self.training, relu=True)
        for conv, bn in zip(list(self.mlp_convs)[1:], list(self.mlp_bns)[1:]):
            h = K.batch_norm_act(K.linear(h, _w2d(conv), conv.bias), bn, self.training, relu=True)
        return h


class get_model(nn.Module):
    LABEL_DIM = 0               # part segmentation (models/partseg.py) sets 16: the category label branch and its 64 per-cloud columns
    LOGGER = "SemSeg"

    def __init__(self, cls_dim):
        super().__init__()
        self.trans_dim = 384
        self.depth = 12
        self.drop_path_rate = 0.1
        self.cls_dim = cls_dim
        self.num_heads = 6
        self.group_size = 32
        self.num_group = 128
        self.group_divider = Group(num_group=self.num_group, group_size=self.group_size)
        self.encoder_dims = 384
        self.encoder = Encoder(encoder_channel=self.encoder_dims)
        self.pos_embed = nn.Sequential(nn.Linear(3, 128), nn.GELU(), nn.Linear(128, self.trans_dim))
        dpr = [x.item() for x in torch.linspace(0, self.drop_path_rate, self.depth)]
        self.blocks = TransformerEncoder(embed_dim=self.trans_dim, depth=self.depth, drop_path_rate=dpr, num_heads=self.num_heads)
        self.norm = nn.LayerNorm(self.trans_dim)
        if self.LABEL_DIM:                      # the reference registers it here: its state_dict keys sit between norm and propagation_0_cls
            self.label_conv_cls = nn.Sequential(nn.Conv1d(self.LABEL_DIM, 64, kernel_size=1, bias=False), nn.BatchNorm1d(64), nn.LeakyReLU(0.2))
        self.propagation_0_cls = PointNetFeaturePropagation(in_channel=1152 + 3, mlp=[self.trans_dim * 4, 1024])
        self.convs1_cls = nn.Conv1d(3328 + (64 if self.LABEL_DIM else 0), 512, 1)
        self.dp1 = nn.Dropout(0.5)
        self.convs2_cls = nn.Conv1d(512, 256, 1)
        self.convs3_cls = nn.Conv1d(256, self.cls_dim, 1)
        self.bns1_cls = nn.BatchNorm1d(512)
        self.bns2_cls = nn.BatchNorm1d(256)
        self.relu = nn.ReLU()
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, (nn.Linear, nn.Conv1d)):
            trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def _strip(self, sd, model_key):
        sd = {k.replace("module.", ""): v for k, v in sd.items()}
        for k in list(sd.keys()):
            if k.startswith(model_key + "."):
                sd[k[len(model_key) + 1:]] = sd.pop(k)
            elif k.startswith("base_model."):
                sd[k[len("base_model."):]] = sd.pop(k)
        return sd

    def _report(self, incompatible, path, mismatched=()):
        if mismatched:
            print_log(f"size mismatch, kept at their initial values: {list(mismatched)}", logger=self.LOGGER)
        if incompatible.missing_keys:
            print_log(f"missing_keys: {incompatible.missing_keys}", logger=self.LOGGER)
        if incompatible.unexpected_keys:
            print_log(f"unexpected_keys: {incompatible.unexpected_keys}", logger=self.LOGGER)
        print_log(f"[Transformer] Successful Loading the ckpt from {path}", logger=self.LOGGER)

    def load_model_from_ckpt(self, bert_ckpt_path, model_key="ACT_encoder"):
        """ACT pretraining checkpoint ({'base_model': state_dict}): strips ``module.``, ``<model_key>.`` and ``base_model.``, loads non-strictly"""
        if bert_ckpt_path is None:
            return None
        ckpt = torch.load(bert_ckpt_path, map_location="cpu")
        incompatible = self.load_state_dict(self._strip(ckpt["base_model"], model_key), strict=False)
        self._report(incompatible, bert_ckpt_path)
        return incompatible

    def load_model_from_ckpt_withrename(self, bert_ckpt_path):
        """checkpoint of this model or of its segmentation sibling ({'model_state_dict': ...}); keys without ``_cls`` map onto ``*_cls``.
        Entries whose shape differs from this model's (the other task's heads: convs1_cls, convs3_cls) are not loaded: they keep their
        initial values, are printed, and are returned among ``missing_keys``."""
        if bert_ckpt_path is None:
            return None
        ckpt = torch.load(bert_ckpt_path, map_location="cpu")["model_state_dict"]
        model_dict = self.state_dict()
        mismatched = []
        for k in list(model_dict.keys()):
            src = k if k in ckpt else (k.replace("_cls", "") if k.replace("_cls", "") in ckpt else None)
            if src is None:
                continue
            if ckpt[src].shape != model_dict[k].shape:
                mismatched.append(k)
            else:
                model_dict[k] = ckpt[src]
        incompatible = self.load_state_dict(model_dict, strict=False)
        self._report(incompatible, bert_ckpt_path, mismatched)
        if mismatched:
            incompatible = type(incompatible)(mismatched + list(incompatible.missing_keys), incompatible.unexpected_keys)
        return incompatible

    def _dropout(self, x, draws):
        p = self.dp1.p
        if not self.training or p == 0:
            return x
        mk = lambda: (torch.rand_like(x) >= p).to(x.dtype)
        keep = draws.get("head.drop1", mk) if draws is not None else mk()
        return x * (keep.to(x.device) / (1.0 - p))

    def features(self, xyz, draws=None):
        """xyz [B,N,3] -> (x [B*G,1152] normed block-3/7/11 tokens, center [B,G,3])"""
        neighborhood, center = self.group_divider(xyz)
        tokens = self.encoder(neighborhood)                                            # B G C
        pe = self.pos_embed
        pos = K.mlp(center, pe[0].weight, pe[0].bias, pe[2].weight, pe[2].bias)
        blocks = self.blocks.blocks
        gates = stack_gates(blocks, tokens.shape[0], tokens.device, draws, self.blocks.__dict__.setdefault("_keep_cache", {}))
        taps = K.block_stack(blocks, tokens, pos, gates, draws, "enc", chunk=4, taps=True)
        assert len(taps) == len(FETCH)
        B, G, D = tokens.shape
        x = torch.cat([K.layer_norm(t, self.norm.weight, self.norm.bias, self.norm.eps) for t in taps], dim=-1)
        return x.reshape(B * G, 3 * D), center

    def forward(self, pts, draws=None, pergroup=None):
        """pts [B, 3, N] (the reference's layout) -> log-probabilities [B, N, cls_dim]"""
        xyz = pts.transpose(1, 2).contiguous()
        x, center = self.features(xyz, draws)
        return self.head(xyz, x, center, (), draws, pergroup)

    def head(self, xyz, x, center, extra=(), draws=None, pergroup=None):
        """xyz [B,N,3], x [B*G,1152], center [B,G,3]; ``extra``: per-cloud blocks appended to the global feature (part segmentation: the
        label branch's [B,64]) -> log-probabilities [B, N, cls_dim]"""
        B, N, _ = xyz.shape
        G = center.shape[1]
        glob = torch.cat((K.group_max(x, G), K.group_mean(x, G)) + tuple(extra), dim=1)  # [B, 2304 (+ 64)]
        f0 = self.propagation_0_cls(xyz, center, x, pergroup=pergroup)                # [B*N, 1024]
        w1 = _w2d(self.convs1_cls)
        nf = f0.shape[1]
        g = K.linear(glob, w1[:, nf:], self.convs1_cls.bias)                            # per-cloud columns, once per cloud
        h = K.batch_norm_act(K.linear_group_add(f0, w1[:, :nf], g, N), self.bns1_cls, self.training, relu=True)
        h = self._dropout(h, draws)
        h = K.batch_norm_act(K.linear(h, _w2d(self.convs2_cls), self.convs2_cls.bias), self.bns2_cls, self.training, relu=True)
        z = K.linear(h, _w2d(self.convs3_cls), self.convs3_cls.bias)
        return K.log_softmax(z).view(B, N, self.cls_dim)


class get_loss(nn.Module):
    """F.nll_loss(pred, target, weight): weighted mean sum w[t] (-logp[t]) / sum w[t] (deterministic device reduction)"""

    def forward(self, pred, target, weight=None):
        C = pred.shape[-1]
        loss, _ = K.nll_weighted(pred.reshape(-1, C), target.reshape(-1), weight)
        return loss

    @staticmethod
    def with_correct(pred, target, weight=None):
        """-> (loss, number of rows whose arg-max equals the target), both on the device"""
        C = pred.shape[-1]
        return K.nll_weighted(pred.reshape(-1, C), target.reshape(-1), weight)
