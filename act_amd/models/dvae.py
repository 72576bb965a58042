"""Point-patch tokenizer and the frozen cross-modal teacher (reference: models/dvae.py).

Same class names, constructor arguments, forward signatures and ``state_dict`` keys as the reference
(``Group``, ``Encoder``, ``DGCNN``, ``Decoder``, ``ACTPromptedDiscreteVAEwithVIT``); the arithmetic runs in
the HIP kernels of libact_hip.so via act_amd.kernels / act_amd.knn_cuda / act_amd.pointnet2_ops.
GPU only: a CPU tensor raises (there is no fallback path).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import kernels as K
from .. import composite as CP
from ..knn_cuda import KNN, knn_group
from ..pointnet2_ops import pointnet2_utils
from ..extensions.chamfer_dist import ChamferDistanceL1, ChamferDistanceL2
from ..utils.draws import Draws
from .build import MODELS

knn = KNN(k=4, transpose_mode=False)          # module-level DGCNN graph operator, as in models/dvae.py:23


EMD_LOSS_DEFAULTS = dict(weight=1.0, eps=1.0e-12, eps_rel=2.0 ** -18, max_bids=100000)


def parse_emd_loss(value, group_size):
    """model key ``emd_loss``: absent / false -> None; ``True`` -> the defaults; a dict -> the defaults with its entries.  The term runs on the
    one-wave-per-pair solver of extensions/emd, so ``group_size`` must not exceed its limit (checked here, at construction)."""
    if not value:
        return None
    opts = dict(EMD_LOSS_DEFAULTS)
    if value is not True:
        if not isinstance(value, dict):
            raise ValueError(f"emd_loss: expected True or a dict of {sorted(EMD_LOSS_DEFAULTS)}, got {value!r}")
        unknown = sorted(set(value) - set(opts))
        if unknown:
            raise ValueError(f"emd_loss: unknown keys {unknown} (supported: {sorted(opts)})")
        opts.update(value)
    opts = dict(weight=float(opts["weight"]), eps=float(opts["eps"]), eps_rel=float(opts["eps_rel"]), max_bids=int(opts["max_bids"]))
    from ..extensions.emd import wave_max_points
    if group_size > wave_max_points():
        raise ValueError(f"emd_loss: group_size = {group_size}, but the matching of a group runs in one wavefront and takes at most "
                         f"{wave_max_points()} points")
    return opts


def trunc_normal_(tensor, mean=0.0, std=1.0, a=-2.0, b=2.0):
    return nn.init.trunc_normal_(tensor, mean=mean, std=std, a=a, b=b)


class Group(nn.Module):
    """FPS centres -> kNN neighbourhoods -> centred patches (models/dvae.py:154-183), two launches."""

    def __init__(self, num_group, group_size, skip_near_origin=None):
        super().__init__()
        self.num_group = num_group
        self.group_size = group_size
        # None: process default (ACT_FPS_SKIP_NEAR_ORIGIN); True reproduces upstream pointnet2_ops, which never selects a point with
        # |p|^2 <= 1e-3 (config key ``fps_skip_near_origin`` of the model / dvae_config sections, absent from the reference YAML)
        self.skip_near_origin = skip_near_origin
        self.knn = KNN(k=self.group_size, transpose_mode=True)

    def forward(self, xyz):
        """xyz [B,N,3] -> neighborhood [B,G,M,3] (centred), center [B,G,3]"""
        xyz = xyz.contiguous()
        with torch.no_grad():
            _, center = pointnet2_utils.furthest_point_sample_with_centers(xyz, self.num_group, self.skip_near_origin)
            _, neighborhood, _ = knn_group(xyz, center, self.group_size, want_nbr=True)
        return neighborhood, center


def _w2d(conv):
    """[out, in, 1(,1)] conv weight viewed as the [out, in] matrix of the equivalent Linear."""
    w = conv.weight
    return w.view(w.shape[0], w.shape[1])


class Encoder(nn.Module):
    """mini-PointNet patch embedding (models/dvae.py:185-215) on rows [B*G*n, C].

    second_conv[0] acts on cat(global.expand, local): W[:, :256] . global is identical for the n points of a
    group, so it is computed once per group and broadcast (exact in real arithmetic, 25% fewer FLOPs)."""

    def __init__(self, encoder_channel):
        super().__init__()
        self.encoder_channel = encoder_channel
        self.first_conv = nn.Sequential(nn.Conv1d(3, 128, 1), nn.BatchNorm1d(128), nn.ReLU(inplace=True),
                                        nn.Conv1d(128, 256, 1))
        self.second_conv = nn.Sequential(nn.Conv1d(512, 512, 1), nn.BatchNorm1d(512), nn.ReLU(inplace=True),
                                         nn.Conv1d(512, self.encoder_channel, 1))

    def forward(self, point_groups, need=None):
        """``need`` [B, k] (optional, no reference counterpart): the only groups per cloud whose tokens the caller reads -- MaskTransformer keeps the
        visible patches (models/act.py:269-275).  The last conv + max-pool then run on those groups alone and the other tokens come back as ZEROS; every
        layer in front still sees all groups (BatchNorm statistics are over all of them), so the wanted tokens and all gradients are unchanged."""
        if CP.ENABLED and not any(isinstance(m, nn.SyncBatchNorm) for m in (self.first_conv[1], self.second_conv[1])):
            return CP.pointnet_forward(self, point_groups, need)        # one host call per direction (csrc/composite.hip)
        bs, g, n, _ = point_groups.shape
        x = point_groups.reshape(bs * g * n, 3)
        c1, bn1, _, c2 = self.first_conv
        c3, bn2, _, c4 = self.second_conv
        h = K.linear(x, _w2d(c1), c1.bias)
        h = K.batch_norm_act(h, bn1, self.training, relu=True)
        h = K.linear(h, _w2d(c2), c2.bias)                               # [R,256]
        fg = K.group_max(h, n)                                           # [BG,256]
        w3 = _w2d(c3)
        gw = K.linear(fg, w3[:, :256], c3.bias)                          # per-group half of the 512->512 conv
        h = K.linear_group_add(h, w3[:, 256:], gw, n)                    # + per-point half, broadcast add in the epilogue
        h = K.batch_norm_act(h, bn2, self.training, relu=True)
        h = K.linear(h, _w2d(c4), c4.bias)
        return K.group_max(h, n).reshape(bs, g, self.encoder_channel)


class DGCNN(nn.Module):
    """4 x (kNN(k=4) graph feature -> 1x1 conv -> GroupNorm(4) -> LeakyReLU(0.2) -> max_k) + 1x1 conv head
    (models/dvae.py:26-117).

    conv(cat(x_j - x_i, x_i)) = Wa x_j + (Wb - Wa) x_i, so each edge-conv layer is ONE GEMM over the B*G points
    (not over the B*G*k edges) followed by a gather: 4x fewer FLOPs than the reference formulation."""

    def __init__(self, encoder_channel, output_channel):
        super().__init__()
        self.input_trans = nn.Conv1d(encoder_channel, 128, 1)

        def layer(cin, cout):
            return nn.Sequential(nn.Conv2d(cin, cout, kernel_size=1, bias=False), nn.GroupNorm(4, cout),
                                 nn.LeakyReLU(negative_slope=0.2))
        self.layer1 = layer(256, 256)
        self.layer2 = layer(512, 512)
        self.layer3 = layer(1024, 512)
        self.layer4 = layer(1024, 1024)
        self.layer5 = nn.Sequential(nn.Conv1d(2304, output_channel, kernel_size=1, bias=False),
                                    nn.GroupNorm(4, output_channel), nn.LeakyReLU(negative_slope=0.2))

    @staticmethod
    def graph_index(coor):
        """coor [B,G,3] -> idx int64 [B,k=4,G] (KNN(k=4, transpose_mode=False) layout)."""
        idx, _, _ = knn_group(coor.contiguous(), coor.contiguous(), 4, idx_kq=True)
        return idx

    @staticmethod
    def _stacked_weight(conv):
        w = _w2d(conv)
        cin = w.shape[1] // 2
        wa, wb = w[:, :cin], w[:, cin:]
        if torch.is_grad_enabled() and w.requires_grad:
            return torch.cat((wa, wb - wa), dim=0)                        # rows: [Wa ; Wb - Wa]
        # frozen / no-grad use (Stage-II teacher): the stacked matrix only changes when the weight does
        cache = conv.__dict__.get("_act_stacked")
        key = (conv.weight.data_ptr(), conv.weight._version, conv.weight.device)
        if cache is None or cache[0] != key:
            with torch.no_grad():
                cache = (key, torch.cat((wa, wb - wa), dim=0))
            conv.__dict__["_act_stacked"] = cache
        return cache[1]

    @staticmethod
    def _edge_layer(f, idx, layer, B, G, out=None, ooff=0):
        conv, gn, _ = layer
        cout = conv.weight.shape[0]
        yz = K.linear(f, DGCNN._stacked_weight(conv), None)               # [BG, 2*Cout] = [Y | Z]
        if not torch.is_grad_enabled():                                   # frozen teacher (Stage II): written into the cat buffer
            return K.edge_gn_lrelu_max(yz, cout, idx, B, G, idx.shape[1], cout, gn, out=out, ooff=ooff)
        return K.edge_gn_lrelu_max_train(yz, cout, idx, B, G, idx.shape[1], cout, gn)     # Stage I: same kernels + HIP backward

    def features(self, f, coor, idx=None):
        """everything up to (not including) layer5's GroupNorm: -> pre-norm head output rows [B*G, C']"""
        B, G, Cin = f.shape
        if idx is None:
            with torch.no_grad():
                idx = self.graph_index(coor)
        if CP.ENABLED and not torch.is_grad_enabled():                     # frozen teacher: the whole stack in one host call
            stacked = [self._stacked_weight(l[0]) for l in (self.layer1, self.layer2, self.layer3, self.layer4)]
            return CP.dgcnn_features(self, f, idx, stacked)
        x = K.linear(f.reshape(B * G, Cin), _w2d(self.input_trans), self.input_trans.bias)
        fused = not torch.is_grad_enabled()
        cat = torch.empty(B * G, 2304, dtype=torch.float32, device=f.device) if fused else None
        feats, off = [], 0
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            cout = layer[0].weight.shape[0]
            x = self._edge_layer(x, idx, layer, B, G, out=cat, ooff=off)
            if fused:
                x = cat[:, off:off + cout]                                # written in place: no torch.cat of the 4 outputs
            feats.append(x)
            off += cout
        h_in = cat if fused else torch.cat(feats, dim=1)
        return K.linear(h_in, _w2d(self.layer5[0]), None)                 # [BG, C']

    def forward(self, f, coor, idx=None):
        """f [B,G,C], coor [B,G,3] -> [B,G,C']"""
        B, G, _ = f.shape
        h = self.features(f, coor, idx)
        gn = self.layer5[1]
        if not torch.is_grad_enabled():
            return K.edge_gn_lrelu_max(h, -1, None, B, G, 1, h.shape[1], gn).view(B, G, -1)
        return K.edge_gn_lrelu_max_train(h, -1, None, B, G, 1, h.shape[1], gn).view(B, G, -1)


class Decoder(nn.Module):
    """FoldingNet decoder (models/dvae.py:217-275)."""

    def __init__(self, encoder_channel, num_fine):
        super().__init__()
        self.num_fine = num_fine
        self.grid_size = 2
        self.num_coarse = self.num_fine // 4
        assert num_fine % 4 == 0
        self.mlp = nn.Sequential(nn.Linear(encoder_channel, 1024), nn.ReLU(inplace=True), nn.Linear(1024, 1024),
                                 nn.ReLU(inplace=True), nn.Linear(1024, 3 * self.num_coarse))
        self.final_conv = nn.Sequential(nn.Conv1d(encoder_channel + 3 + 2, 512, 1), nn.BatchNorm1d(512), nn.ReLU(inplace=True),
                                        nn.Conv1d(512, 512, 1), nn.BatchNorm1d(512), nn.ReLU(inplace=True), nn.Conv1d(512, 3, 1))
        lin = torch.linspace(-0.05, 0.05, steps=self.grid_size, dtype=torch.float)
        a = lin.view(1, self.grid_size).expand(self.grid_size, self.grid_size).reshape(1, -1)
        b = lin.view(self.grid_size, 1).expand(self.grid_size, self.grid_size).reshape(1, -1)
        # non-persistent buffer: follows .to(device) (a CPU attribute would cost a blocking H2D copy per step), not in the state_dict
        self.register_buffer("folding_seed", torch.cat([a, b], dim=0).view(1, 2, self.grid_size ** 2), persistent=False)

    def forward(self, feature_global):
        """feature_global [B,G,C] -> coarse [B,G,M/4,3], fine [B,G,M,3]"""
        bs, g, c = feature_global.shape
        fgl = feature_global.reshape(bs * g, c)
        m = self.mlp
        coarse = K.mlp_relu3(fgl, m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias).reshape(bs * g, self.num_coarse, 3)
        S = self.grid_size ** 2
        rep = coarse.unsqueeze(2).expand(-1, -1, S, -1).reshape(bs * g * self.num_fine, 3)      # rows (group, point)
        seed = self.folding_seed.to(fgl.device).view(2, S).t()                                   # [S,2]
        seed = seed.unsqueeze(0).expand(bs * g * self.num_coarse, -1, -1).reshape(bs * g * self.num_fine, 2)
        c1, bn1, _, c2, bn2, _, c3 = self.final_conv
        w1 = _w2d(c1)
        # conv over cat(feature_global, seed, point): the feature_global part is constant per group
        gw = K.linear(fgl, w1[:, :c], c1.bias)                                                  # [BG,512]
        h = K.linear_group_add(torch.cat((seed, rep), dim=1), w1[:, c:], gw, self.num_fine)
        h = K.batch_norm_act(h, bn1, self.training, relu=True)
        h = K.batch_norm_act(K.linear(h, _w2d(c2), c2.bias), bn2, self.training, relu=True)
        fine = K.linear(h, _w2d(c3), c3.bias) + rep
        return coarse.reshape(bs, g, self.num_coarse, 3), fine.reshape(bs, g, self.num_fine, 3)


class _FrozenBlock(nn.Module):
    """parameter container with the timm ViT block key names (norm1, attn.qkv/proj, norm2, mlp.fc1/fc2)."""

    def __init__(self, dim, heads, qkv_bias=True, eps=1e-6):
        super().__init__()
        self.num_heads, self.eps = heads, eps
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = nn.Module()
        self.attn.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn.proj = nn.Linear(dim, dim)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = nn.Module()
        self.mlp.fc1 = nn.Linear(dim, dim * 4)
        self.mlp.fc2 = nn.Linear(dim * 4, dim)

    def forward(self, x, pos=None, gate1=None, gate2=None, train_w=False):
        a, m = self.attn, self.mlp
        return K.BlockFn.apply(x, pos, gate1, gate2, self.norm1.weight, self.norm1.bias, a.qkv.weight, a.qkv.bias,
                               a.proj.weight, a.proj.bias, self.norm2.weight, self.norm2.bias, m.fc1.weight, m.fc1.bias,
                               m.fc2.weight, m.fc2.bias, self.num_heads, self.eps, train_w)


class _ClipAttnParams(nn.Module):
    """``nn.MultiheadAttention``'s parameters under its key names: in_proj_weight [3D, D] (q, k, v stacked, heads major inside each), in_proj_bias, out_proj"""

    def __init__(self, dim):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * dim, dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * dim))
        self.out_proj = nn.Linear(dim, dim)
        nn.init.xavier_uniform_(self.in_proj_weight)


class _ClipBlock(nn.Module):
    """parameter container of one CLIP ``ResidualAttentionBlock``, its key names and order (attn.{in_proj_weight,in_proj_bias,out_proj}, ln_1,
    mlp.{c_fc,c_proj}, ln_2); the arithmetic is K.clip_block."""

    def __init__(self, dim, heads, eps=1e-5):
        super().__init__()
        self.num_heads, self.eps = heads, eps
        self.attn = _ClipAttnParams(dim)
        self.ln_1 = nn.LayerNorm(dim, eps=eps)
        self.mlp = nn.Module()
        self.mlp.c_fc = nn.Linear(dim, dim * 4)
        self.mlp.c_proj = nn.Linear(dim * 4, dim)
        self.ln_2 = nn.LayerNorm(dim, eps=eps)

    def forward(self, x, pos=None):
        a, m = self.attn, self.mlp
        return K.clip_block(x, pos, self.ln_1.weight, self.ln_1.bias, a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias,
                            self.ln_2.weight, self.ln_2.bias, m.c_fc.weight, m.c_fc.bias, m.c_proj.weight, m.c_proj.bias, self.num_heads, self.eps)


_CLIP_GEOMETRY = {"vit-b/16": (12, 12), "vit-b/32": (12, 12), "vit-l/14": (24, 16)}      # clip:<name> -> (layers, heads) of the visual tower; head dimension 64

_VIT_GEOMETRY = {            # timm names -> (depth, heads); width must equal config.visual_embed_dim
    "vit_base_patch16_384": (12, 12), "vit_base_patch16_224": (12, 12), "vit_small_patch16_384": (12, 6),
    "vit_small_patch16_224": (12, 6), "deit_base_distilled_patch16_384": (12, 12),
}


@MODELS.register_module()
class DiscreteVAE(nn.Module):
    """The plain Point-BERT tokenizer / autoencoder (models/dvae.py:278-358, recipe cfgs/autoencoder/pointbert_dvae.yaml):
    Group -> mini-PointNet -> DGCNN -> gumbel-softmax over the codebook -> DGCNN -> FoldingNet; everything trainable.
    ``forward(inp, temperature, hard)`` -> the 6-tuple, ``get_loss(ret, gt)`` -> (loss_recon, loss_klv)."""

    def __init__(self, config, **kwargs):
        super().__init__()
        self.group_size = config.group_size
        self.num_group = config.num_group
        self.encoder_dims = config.encoder_dims
        self.tokens_dims = config.tokens_dims
        self.decoder_dims = config.decoder_dims
        self.num_tokens = config.num_tokens
        self.group_divider = Group(num_group=self.num_group, group_size=self.group_size, skip_near_origin=config.get("fps_skip_near_origin", None))
        self.encoder = Encoder(encoder_channel=self.encoder_dims)
        self.dgcnn_1 = DGCNN(encoder_channel=self.encoder_dims, output_channel=self.num_tokens)
        self.codebook = nn.Parameter(torch.randn(self.num_tokens, self.tokens_dims))
        self.dgcnn_2 = DGCNN(encoder_channel=self.tokens_dims, output_channel=self.decoder_dims)
        self.decoder = Decoder(encoder_channel=self.decoder_dims, num_fine=self.group_size)
        self.build_loss_func()
        self.build_emd_loss(config)

    def build_loss_func(self):
        self.loss_func_cdl1 = ChamferDistanceL1()
        self.loss_func_cdl2 = ChamferDistanceL2()

    def build_emd_loss(self, config):
        """optional model key ``emd_loss`` (``parse_emd_loss``): the line ``# self.loss_func_emd = emd().cuda()`` of models/dvae.py:302,701.
        ``emd_last_info``: the ``info`` tensor of the last solve; ``emd_capped``: int64 device scalar, += the pairs whose solve hit
        ``max_bids``.  Neither is read on the host by a training step (the runner reads ``emd_capped`` once per epoch)."""
        self.emd_loss = parse_emd_loss(config.get("emd_loss", None), self.group_size)
        if self.emd_loss is not None:
            self.emd_last_info = None
            self.register_buffer("emd_capped", torch.zeros((), dtype=torch.int64), persistent=False)      # state_dict keys stay the reference's

    # ---- losses (Stage I) ------------------------------------------------------------------------
    def recon_loss(self, ret, gt):
        """CDL1(coarse, group_gt) + CDL1(fine, group_gt), per group.  With ``emd_loss``: + weight * mean over all B*G*group_size points of
        sqrt(dist), dist the squared distances of the one-to-one matching of (fine, group_gt) per group; differentiable in ``fine`` with the
        matching held fixed.  (The square root has no finite slope at 0: a point that coincides with its match gives a NaN gradient, as in
        ChamferDistanceL1.)  ``coarse`` has group_size / 4 points and gets no such term."""
        whole_coarse, whole_fine, coarse, fine, group_gt, _ = ret
        bs, g, _, _ = coarse.shape
        coarse = coarse.reshape(bs * g, -1, 3).contiguous()
        fine = fine.reshape(bs * g, -1, 3).contiguous()
        group_gt = group_gt.reshape(bs * g, -1, 3).contiguous()
        loss = self.loss_func_cdl1(coarse, group_gt) + self.loss_func_cdl1(fine, group_gt)
        if self.emd_loss is None:
            return loss
        from ..extensions.emd import EMDFunction
        o, info = self.emd_loss, []
        dist, _ = EMDFunction.apply(fine, group_gt, o["eps"], o["max_bids"], info, "wave", o["eps_rel"])
        self.emd_last_info = info[0]
        self.emd_capped += (info[0] < 0).sum()
        return loss + o["weight"] * torch.mean(torch.sqrt(dist))

    def get_loss(self, ret, gt):
        loss_recon = self.recon_loss(ret, gt)
        loss_klv = K.kl_to_uniform(ret[-1])        # KL(mean_g softmax(logits) || uniform), 'batchmean' (models/dvae.py:470-476)
        return loss_recon, loss_klv

    def visual_embedding(self, input, center, draws=None, rng=None):
        return input                               # the plain tokenizer feeds the codebook vectors straight to dgcnn_2 (:340, :350)

    def _rng(self, device):
        """(base seed, device-resident step counter) of the in-kernel Philox draws of the frozen-teacher path.  The counter lives
        in HBM and is bumped by a device op per teacher forward, so a captured hipGraph of that forward draws fresh noise on
        every replay and eager / replayed executions produce the same sequence."""
        st = self.__dict__.get("_rng_state")
        if st is None or st[1].device != device:
            st = (int(torch.randint(0, 2 ** 62, (1,)).item()), torch.zeros(1, dtype=torch.int64, device=device))
            self.__dict__["_rng_state"] = st
        return st

    # ---- tokenizer ----------------------------------------------------------------------------------
    def _gumbel_codes(self, logits, tau, hard, draws):
        g = None
        if draws is not None and (draws.has("gumbel") or draws.record):
            g = draws.get("gumbel", lambda: -torch.empty_like(logits).exponential_().log())
        if hard:
            if g is None:
                g = -torch.empty_like(logits).exponential_().log()
            index = ((logits + g) / tau).argmax(dim=-1)    # one-hot x codebook == row gather (models/dvae.py:587-588)
            codes = F.embedding(index, self.codebook)
            if torch.is_grad_enabled() and logits.requires_grad:
                # straight-through estimator of F.gumbel_softmax(hard=True): y = y_hard - y_soft.detach() + y_soft, so the value is the
                # codebook row while the gradient reaches the logits through y_soft (and the codebook only through the selected rows)
                soft = K.gumbel_softmax(logits, tau, noise=g)
                through = K.linear(soft, self.codebook.detach().t().contiguous(), None)
                codes = codes + (through - through.detach())
            return codes
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if g is None else 0       # host RNG (no device sync)
        y = K.gumbel_softmax(logits, tau, noise=g, seed=seed)                       # soft one-hot [B,G,N], noise from Philox in-kernel
        return K.linear(y, self.codebook.t().contiguous(), None)

    def forward_tokenizer(self, neighborhood, center):
        gt_logits = self.dgcnn_1(self.encoder(neighborhood), center)
        return gt_logits.argmax(-1).long()

    def forward_tokenizer_features(self, neighborhood, center, return_global=True, draws=None):
        with torch.no_grad():
            idx = DGCNN.graph_index(center)                # the k=4 graph is identical for all 8 edge-conv layers
        if not torch.is_grad_enabled():
            # frozen teacher: head GroupNorm + LeakyReLU + hard gumbel + codebook lookup in one pass over the logits
            B, G, _ = center.shape
            h = self.dgcnn_1.features(self.encoder(neighborhood), center, idx)
            noise = None
            if draws is not None and (draws.has("gumbel") or draws.record):
                noise = draws.get("gumbel", lambda: -torch.empty(B, G, h.shape[1], device=h.device).exponential_().log())
            rng = self._rng(h.device)
            sampled, _, _ = K.gn_gumbel_argmax_gather(h, B, G, self.dgcnn_1.layer5[1], self.codebook, noise=noise,
                                                      seed=rng[0] ^ 0x5bd1e995, seed_dev=rng[1])
            feature = self.visual_embedding(sampled, center, draws, rng)
            if return_global:
                feature = self.dgcnn_2(feature, center, idx)
            rng[1].add_(1)                                 # next teacher forward draws a fresh Philox stream
            return feature
        logits = self.dgcnn_1(self.encoder(neighborhood), center, idx)
        sampled = self._gumbel_codes(logits, 1.0, True, draws)
        feature = self.visual_embedding(sampled, center, draws)
        if return_global:
            feature = self.dgcnn_2(feature, center, idx)
        return feature

    def forward(self, inp, temperature=1., hard=False, draws=None, **kwargs):
        neighborhood, center = self.group_divider(inp)
        with torch.no_grad():
            idx = DGCNN.graph_index(center)
        logits = self.dgcnn_1(self.encoder(neighborhood), center, idx)
        sampled = self._gumbel_codes(logits, temperature, hard, draws)
        sampled = self.visual_embedding(sampled, center, draws)
        feature = self.dgcnn_2(sampled, center, idx)
        coarse, fine = self.decoder(feature)
        with torch.no_grad():
            whole_fine = (fine + center.unsqueeze(2)).reshape(inp.size(0), -1, 3)
            whole_coarse = (coarse + center.unsqueeze(2)).reshape(inp.size(0), -1, 3)
        assert fine.size(2) == self.group_size
        return (whole_coarse, whole_fine, coarse, fine, neighborhood, logits)


@MODELS.register_module()
class ACTPromptedDiscreteVAEwithVIT(DiscreteVAE):
    """Stage-I autoencoder / Stage-II frozen teacher (models/dvae.py:360-615): DiscreteVAE with the prompt-tuned image Transformer
    between the codebook lookup and dgcnn_2.

    The pretrained image Transformer is represented by its ``blocks`` + ``norm`` (what the reference keeps,
    :405-410) with timm's key names; weights come from the dVAE checkpoint (``ckpt``), never from the network.
    Optional config keys (absent from the reference YAML): ``visual_embed_depth`` / ``visual_embed_heads``
    override the geometry implied by ``visual_embed_type``.

    ``visual_embed_type: clip:ViT-B/16`` (any name with 'clip' in it, :394-403) is CLIP's visual tower instead: ``visual_embed = Sequential(ln_pre, resblocks,
    ln_post)`` with CLIP's key names, QuickGELU, LayerNorm eps 1e-5; its length of 3 is how the forward tells the two apart (:501).  The ``clip`` package is never
    imported and nothing is fetched: the weights come from the dVAE checkpoint or from the optional local ``visual_embed_ckpt``, else they are random and the
    class says so.  Shallow prompts only: ``use_deep_prompt: True`` raises ValueError (the reference's deep path hands a batch-first tensor to a sequence-first
    attention) and ``freeze_visual_embed: False`` raises NotImplementedError.  The CLIP teacher always runs in fp32 (ACT_TEACHER_BF16X3 does not reach it)."""

    def __init__(self, config, **kwargs):
        super().__init__(config)
        self.visual_embed_type = config.visual_embed_type
        self.visual_embed_dim = config.visual_embed_dim
        self.freeze_visual_embed = config.freeze_visual_embed
        self.num_prompt_token = config.num_prompt_token
        self.use_deep_prompt = config.use_deep_prompt
        if self.use_deep_prompt and (self.visual_embed_dim == 'none' or self.num_prompt_token <= 0):
            raise ValueError("use_deep_prompt needs an image Transformer and num_prompt_token > 0 (the reference fails on this combination too)")
        self.build_visual_embedding(config)

    def build_visual_embedding(self, config):
        """models/dvae.py:390-444.  Configurations: deep prompts (the ACT recipe, `use_deep_prompt`), shallow prompts (prepended once), no
        prompts (`num_prompt_token` 0), no image Transformer (`visual_embed_dim: none`)."""
        if self.visual_embed_dim == 'none':
            self.visual_embed = None
            return
        D = self.visual_embed_dim
        self.is_clip = 'clip' in str(self.visual_embed_type).lower()
        if self.is_clip:
            depth, heads = self._clip_geometry(config)
            self.visual_embed = nn.Sequential(nn.LayerNorm(D, eps=1e-5), nn.Sequential(*[_ClipBlock(D, heads) for _ in range(depth)]),
                                              nn.LayerNorm(D, eps=1e-5))
        else:
            depth, heads = _VIT_GEOMETRY.get(self.visual_embed_type, (12, 12))
            depth = int(config.get("visual_embed_depth", depth))
            heads = int(config.get("visual_embed_heads", heads))
            blocks = nn.Sequential(*[_FrozenBlock(D, heads) for _ in range(depth)])
            self.visual_embed = nn.Sequential(blocks, nn.LayerNorm(D, eps=1e-6))
        self.visual_embed_depth = depth
        self.proj_pre = nn.Linear(self.tokens_dims, D)
        self.visual_pos_embed = nn.Sequential(nn.Linear(3, 128), nn.GELU(), nn.Linear(128, D))
        self.proj_post = nn.Linear(D, self.tokens_dims)
        Pn = self.num_prompt_token
        if Pn > 0:
            self.visual_prompt_proj = nn.Identity()
            self.prompt_dropout = nn.Dropout(0.1)
            self.visual_prompt_token = nn.Parameter(torch.zeros(1, Pn, D))
            self.visual_prompt_pos = nn.Parameter(torch.randn(1, Pn, D))
            trunc_normal_(self.visual_prompt_token, std=.02)
            trunc_normal_(self.visual_prompt_pos, std=.02)
            if self.use_deep_prompt:
                self.deep_prompt_tokens = nn.Parameter(torch.zeros(depth - 1, Pn, D))
                self.deep_prompt_pos = nn.Parameter(torch.randn(depth - 1, Pn, D))
                trunc_normal_(self.deep_prompt_tokens, std=.02)
                trunc_normal_(self.deep_prompt_pos, std=.02)
        else:
            self.visual_prompt_token = None
        if self.is_clip:
            ckpt = config.get("visual_embed_ckpt", None)
            if ckpt and str(ckpt).lower() not in ("none", "random", ""):
                self.load_clip_visual(ckpt)
            else:
                import warnings
                warnings.warn("ACTPromptedDiscreteVAEwithVIT: no visual_embed_ckpt -- the CLIP visual Transformer is RANDOMLY INITIALISED unless a dVAE "
                              "checkpoint that contains it is loaded afterwards.  Real Stage-I training must point visual_embed_ckpt at a local CLIP file of "
                              + str(self.visual_embed_type) + " (its state_dict or its TorchScript archive); nothing is ever downloaded.", stacklevel=2)
        if self.freeze_visual_embed:
            for param in self.visual_embed.parameters():
                param.requires_grad = False

    def _clip_geometry(self, config):
        """the refusals and the (layers, heads) of a CLIP teacher"""
        if self.use_deep_prompt:
            raise ValueError("use_deep_prompt: True is not built for a CLIP teacher: in the reference's visual_embedding_deep_prompt the permute(0, 1, 2) calls "
                             "are identities, so the batch-first tensor enters nn.MultiheadAttention, which reads dimension 0 as the sequence, and attention "
                             "runs across the clouds of a batch.  Neither that nor the presumably intended per-cloud attention is computed; use "
                             "use_deep_prompt: False (shallow prompts)")
        if not self.freeze_visual_embed:
            raise NotImplementedError("freeze_visual_embed: False -- training CLIP's own weights is not built (ACT's recipe never trains the teacher "
                                      "Transformer; only prompts and projections learn)")
        name = str(self.visual_embed_type).split(":", 1)[-1].strip().lower()
        has = lambda k: config.get(k, None) is not None       # noqa: E731
        if name not in _CLIP_GEOMETRY and not (has("visual_embed_depth") and has("visual_embed_heads")):
            raise ValueError(f"visual_embed_type {self.visual_embed_type!r}: the CLIP visual Transformers are {sorted('clip:' + k for k in _CLIP_GEOMETRY)} "
                             "(the ResNet towers have no Transformer blocks); any other needs visual_embed_depth and visual_embed_heads")
        depth, heads = _CLIP_GEOMETRY.get(name, (0, 0))
        depth = int(config.get("visual_embed_depth")) if has("visual_embed_depth") else depth
        heads = int(config.get("visual_embed_heads")) if has("visual_embed_heads") else heads
        D = self.visual_embed_dim
        if depth < 1 or heads < 1 or D % heads or D // heads not in (32, 64):
            raise ValueError(f"visual_embed_dim {D} / visual_embed_heads {heads} / visual_embed_depth {depth}: the attention kernels take head dimensions "
                             "32 and 64")
        return depth, heads

    def load_clip_visual(self, path):
        """``path``: a local file of CLIP -- a ``state_dict`` (``torch.save``) or the TorchScript archive CLIP distributes -- either the whole model's
        (``visual.ln_pre.*``, ``visual.transformer.resblocks.{i}.*``, ``visual.ln_post.*``) or one already in this class's ``visual_embed.*`` form.
        fp16 is cast to fp32; a missing or mis-shaped key raises and names it."""
        try:
            sd = torch.load(path, map_location='cpu')
        except Exception:
            sd = torch.jit.load(path, map_location='cpu')
        if hasattr(sd, "state_dict"):
            sd = sd.state_dict()
        sd = sd.get("state_dict", sd)
        forms = (("visual.ln_pre.", "visual_embed.0."), ("visual.transformer.resblocks.", "visual_embed.1."), ("visual.ln_post.", "visual_embed.2."),
                 ("visual_embed.", "visual_embed."))
        got = {}
        for k, v in sd.items():
            k = k[7:] if k.startswith("module.") else k
            for src, dst in forms:
                if k.startswith(src):
                    got[dst + k[len(src):]] = v
                    break
        with torch.no_grad():
            for name, p in self.visual_embed.state_dict().items():
                key = "visual_embed." + name
                if key not in got:
                    raise KeyError(f"{path}: {key} is missing (CLIP form: {self._clip_form(key)})")
                v = got[key]
                if tuple(v.shape) != tuple(p.shape):
                    raise ValueError(f"{path}: {key} has shape {tuple(v.shape)}, the model's is {tuple(p.shape)}")
                p.copy_(v.to(torch.float32))

    @staticmethod
    def _clip_form(key):
        for src, dst in (("visual.ln_pre.", "visual_embed.0."), ("visual.transformer.resblocks.", "visual_embed.1."), ("visual.ln_post.", "visual_embed.2.")):
            if key.startswith(dst):
                return src + key[len(dst):]
        return key

    # ---- prompt-tuned frozen Transformer ---------------------------------------------------------
    def _drop(self, t, draws, key):
        p = self.prompt_dropout.p
        if not self.training or p == 0:
            return t
        if draws is not None and draws.has(key):
            return t * draws.get(key, None).to(t.dtype) / (1.0 - p)
        if draws is not None and draws.record:
            keep = draws.get(key, lambda: (torch.rand_like(t) >= p).to(t.dtype))
            return t * keep / (1.0 - p)
        return F.dropout(t, p, True)

    def _prompt_rows(self, tok, ppos, B, draws, key):
        """dropout(tok) + ppos for every cloud, [B*Pn, D], one HIP launch per direction (K.prompt_rows): injected / recorded keep masks
        when the parity tests ask for them, in-kernel Philox otherwise."""
        p = self.prompt_dropout.p if self.training else 0.0
        mask = None
        if p > 0 and draws is not None and (draws.has(key) or draws.record):
            shape = (B,) + tuple(tok.shape)
            mask = draws.get(key, lambda: (torch.rand(shape, device=tok.device) >= p).to(tok.dtype))
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if (p > 0 and mask is None) else 0       # host RNG: no device sync
        return K.prompt_rows(tok, ppos, B, p, seed, mask)

    def visual_embedding(self, input, center, draws=None, rng=None):
        if self.visual_embed is None:
            return input
        if self.use_deep_prompt:
            return self.visual_embedding_deep_prompt(input, center, draws=draws, rng=rng)
        return self._visual_embedding_shallow(input, center, draws)

    def _visual_embedding_shallow(self, input, center, draws=None):
        """models/dvae.py:517-534: the Transformer applied as `x = blk(x + pos)` (forward_visual_feature :500-511), either on the patch
        tokens alone -- under no_grad when it is frozen (:522-524), so nothing upstream receives a gradient through it -- or behind prompts
        that are prepended ONCE (incorporate_prompt :485-498) and whose outputs flow through all blocks before being dropped."""
        B = input.shape[0]
        Pn = self.num_prompt_token
        vp = self.visual_pos_embed
        pos = K.mlp(center, vp[0].weight, vp[0].bias, vp[2].weight, vp[2].bias)
        hidden = K.linear(input, self.proj_pre.weight, self.proj_pre.bias)
        train_w = not self.freeze_visual_embed
        nrm = self.visual_embed[-1]
        if len(self.visual_embed) == 3:                    # CLIP (:501-507): ln_pre on the prompted rows (pos is not normalised), then x = blk(x + pos)
            pre = self.visual_embed[0]

            def stack(h, p):
                h = K.layer_norm(h, pre.weight, pre.bias, pre.eps)
                for blk in self.visual_embed[1]:
                    h = blk(h, p)
                return h
        else:
            def stack(h, p):
                for blk in self.visual_embed[0]:
                    h = blk(h, p, None, None, train_w)
                return h
        if self.visual_prompt_token is None:
            if self.freeze_visual_embed:
                with torch.no_grad():
                    hidden = stack(hidden, pos)
            else:
                hidden = stack(hidden, pos)
        else:
            hidden = torch.cat((self._drop(self.visual_prompt_token.expand(B, -1, -1), draws, "prompt.0"), hidden), dim=1)
            pos = torch.cat((self.visual_prompt_pos.expand(B, -1, -1), pos), dim=1)
            hidden = stack(hidden, pos)[:, Pn:].contiguous()
        return K.linear(K.layer_norm(hidden, nrm.weight, nrm.bias, nrm.eps), self.proj_post.weight, self.proj_post.bias)

    def _visual_embedding_prefix(self, input, center, draws=None, rng=None):
        """Inference form of visual_embedding_deep_prompt.  Every layer REPLACES the prompt rows of its input
        (models/dvae.py:556-566) and the final output drops them (:574), so prompt tokens only ever act as keys/values:
        queries, projection and MLP are evaluated for the G patch tokens only (58 % of the FLOPs, identical outputs)."""
        B, G, _ = input.shape
        Pn, D = self.num_prompt_token, self.visual_embed_dim
        drop_p = self.prompt_dropout.p if self.training else 0.0
        fused = draws is None or not (draws.record or any(draws.has(f"prompt.{i}") for i in range(self.visual_embed_depth)))
        base, ctr = rng if rng is not None else self._rng(input.device)
        if fused and CP.ENABLED:                                         # the whole 12-layer stack in one host call (~125 launches)
            return CP.prefix_vit_forward(self, input, center, drop_p, base, ctr)
        vp = self.visual_pos_embed
        pos = K.mlp(center, vp[0].weight, vp[0].bias, vp[2].weight, vp[2].bias).reshape(B * G, D)
        x = K.linear(input, self.proj_pre.weight, self.proj_pre.bias).reshape(B * G, D)
        blocks = self.visual_embed[0]
        for i in range(self.visual_embed_depth):
            tok = self.visual_prompt_token[0] if i == 0 else self.deep_prompt_tokens[i - 1]
            ppos = self.visual_prompt_pos[0] if i == 0 else self.deep_prompt_pos[i - 1]
            blk = blocks[i]
            a, m = blk.attn, blk.mlp
            prm = kvp = None
            if fused:       # dropout (in-kernel Philox) + prompt position + LayerNorm + the K,V rows of the qkv Linear: the entry the composite stack calls
                kvp = K.prompt_kv(tok, ppos, B, drop_p, (base + 7919 * (i + 1)) & (2 ** 62 - 1), blk.norm1.weight, blk.norm1.bias, blk.eps,
                                  a.qkv.weight[D:], a.qkv.bias[D:] if a.qkv.bias is not None else None, seed_dev=ctr)
            else:           # injected / recorded dropout masks (parity tests)
                prm = (self._drop(tok.unsqueeze(0).expand(B, -1, -1), draws, f"prompt.{i}") + ppos).reshape(B * Pn, D)
            x = K.block_forward_prefix(x, pos, prm, B, Pn, G, blk.norm1.weight, blk.norm1.bias, a.qkv.weight, a.qkv.bias,
                                       a.proj.weight, a.proj.bias, blk.norm2.weight, blk.norm2.bias, m.fc1.weight, m.fc1.bias,
                                       m.fc2.weight, m.fc2.bias, blk.num_heads, blk.eps, kvp=kvp)
        nrm = self.visual_embed[1]
        feature = K.layer_norm(x, nrm.weight, nrm.bias, nrm.eps)
        return K.linear(feature, self.proj_post.weight, self.proj_post.bias).reshape(B, G, -1)

    def _visual_embedding_prefix_train(self, input, center, draws=None):
        """Stage-I training form of the same restructuring (frozen block weights, learnable prompts / projections): gradients
        reach the prompts through their keys/values only, exactly as in the reference graph."""
        B, G, _ = input.shape
        Pn, D = self.num_prompt_token, self.visual_embed_dim
        vp = self.visual_pos_embed
        pos = K.mlp(center, vp[0].weight, vp[0].bias, vp[2].weight, vp[2].bias).reshape(B * G, D)
        x = K.linear(input, self.proj_pre.weight, self.proj_pre.bias).reshape(B * G, D)
        blocks = self.visual_embed[0]
        for i in range(self.visual_embed_depth):
            tok = self.visual_prompt_token[0] if i == 0 else self.deep_prompt_tokens[i - 1]
            ppos = self.visual_prompt_pos[0] if i == 0 else self.deep_prompt_pos[i - 1]
            prm = self._prompt_rows(tok, ppos, B, draws, f"prompt.{i}")
            blk = blocks[i]
            a, m = blk.attn, blk.mlp
            x = K.PrefixBlockFn.apply(x, pos, prm, B, Pn, G, blk.norm1.weight, blk.norm1.bias, a.qkv.weight, a.qkv.bias,
                                      a.proj.weight, a.proj.bias, blk.norm2.weight, blk.norm2.bias, m.fc1.weight, m.fc1.bias,
                                      m.fc2.weight, m.fc2.bias, blk.num_heads, blk.eps)
        nrm = self.visual_embed[1]
        feature = K.layer_norm(x, nrm.weight, nrm.bias, nrm.eps)
        return K.linear(feature, self.proj_post.weight, self.proj_post.bias).reshape(B, G, -1)

    def visual_embedding_deep_prompt(self, input, center, permute_feature=False, draws=None, rng=None):
        """models/dvae.py:536-576 (+ incorporate_prompt :485-498): prompts replaced (not appended) at layers 1..L-1."""
        if not torch.is_grad_enabled():
            return self._visual_embedding_prefix(input, center, draws, rng)
        if self.freeze_visual_embed:
            return self._visual_embedding_prefix_train(input, center, draws)
        B, G, _ = input.shape
        Pn = self.num_prompt_token
        vp = self.visual_pos_embed
        pos_tok = K.mlp(center, vp[0].weight, vp[0].bias, vp[2].weight, vp[2].bias)                 # [B,G,D]
        feature = K.linear(input, self.proj_pre.weight, self.proj_pre.bias)
        train_w = not self.freeze_visual_embed
        hidden = torch.cat((self._drop(self.visual_prompt_token.expand(B, -1, -1), draws, "prompt.0"), feature), dim=1)
        pos = torch.cat((self.visual_prompt_pos.expand(B, -1, -1), pos_tok), dim=1)
        blocks = self.visual_embed[0]
        for i in range(self.visual_embed_depth):
            if i > 0:
                prm = self._drop(self.deep_prompt_tokens[i - 1].expand(B, -1, -1), draws, f"prompt.{i}")
                hidden = torch.cat((prm, hidden[:, Pn:, :]), dim=1)
                pos = torch.cat((self.deep_prompt_pos[i - 1].expand(B, -1, -1), pos_tok), dim=1)
            hidden = blocks[i](hidden, pos, None, None, train_w)
        nrm = self.visual_embed[1]
        feature = K.layer_norm(hidden[:, Pn:].contiguous(), nrm.weight, nrm.bias, nrm.eps)
        return K.linear(feature, self.proj_post.weight, self.proj_post.bias)


class _BertLayerParams(nn.Module):
    """parameter container of one transformers ``BertLayer``, its key names and order (attention.self.{query,key,value}, attention.output.{dense,
    LayerNorm}, intermediate.dense, output.{dense,LayerNorm}); the arithmetic is K.bert_layer."""

    def __init__(self, dim, heads, intermediate, eps=1e-12, p_attn=0.1, p_hidden=0.1):
        super().__init__()
        self.num_heads, self.eps, self.p_attn, self.p_hidden = heads, eps, p_attn, p_hidden
        self.attention = nn.Module()
        setattr(self.attention, "self", nn.Module())
        att = getattr(self.attention, "self")
        att.query, att.key, att.value = nn.Linear(dim, dim), nn.Linear(dim, dim), nn.Linear(dim, dim)
        self.attention.output = nn.Module()
        self.attention.output.dense = nn.Linear(dim, dim)
        self.attention.output.LayerNorm = nn.LayerNorm(dim, eps=eps)
        self.intermediate = nn.Module()
        self.intermediate.dense = nn.Linear(dim, intermediate)
        self.output = nn.Module()
        self.output.dense = nn.Linear(intermediate, dim)
        self.output.LayerNorm = nn.LayerNorm(dim, eps=eps)

    def qkv(self):
        """the concatenated [3D, D] weight and [3D] bias of the packed q/k/v product, built once and rebuilt only when a weight changes"""
        att = getattr(self.attention, "self")
        ps = (att.query.weight, att.key.weight, att.value.weight, att.query.bias, att.key.bias, att.value.bias)
        key = tuple((p.data_ptr(), p._version, p.device) for p in ps)
        cache = self.__dict__.get("_act_qkv")
        if cache is None or cache[0] != key:
            with torch.no_grad():
                cache = (key, torch.cat(ps[:3], dim=0).contiguous(), torch.cat(ps[3:], dim=0).contiguous())
            self.__dict__["_act_qkv"] = cache
        return cache[1], cache[2]

    def forward(self, x, p_attn, p_hidden, seeds, masks, seed_dev):
        wqkv, bqkv = self.qkv()
        ao, o = self.attention.output, self.output
        return K.bert_layer(x, wqkv, bqkv, ao.dense.weight, ao.dense.bias, ao.LayerNorm.weight, ao.LayerNorm.bias, self.intermediate.dense.weight,
                            self.intermediate.dense.bias, o.dense.weight, o.dense.bias, o.LayerNorm.weight, o.LayerNorm.bias, self.num_heads, self.eps,
                            p_attn, p_hidden, seeds, masks, seed_dev)


class _BertEncoderParams(nn.Module):
    """``BertModel.encoder``: ``layer.{i}``"""

    def __init__(self, dim, heads, intermediate, depth):
        super().__init__()
        self.layer = nn.ModuleList([_BertLayerParams(dim, heads, intermediate) for _ in range(depth)])


_BERT_GEOMETRY = {"bert-base-uncased": (12, 12, 3072), "bert-base-cased": (12, 12, 3072), "bert-large-uncased": (24, 16, 4096)}     # depth, heads, intermediate


@MODELS.register_module()
class ACTPromptedDiscreteVAEwithBERT(DiscreteVAE):
    """The language teacher (models/dvae.py:617-857): DiscreteVAE with a prompt-tuned, FROZEN BERT encoder between the codebook lookup and dgcnn_2.

    ``visual_embed = nn.Sequential(BertModel.encoder)`` is represented by a parameter container with transformers' key names
    (``visual_embed.0.layer.{i}.…``), so a reference checkpoint loads with ``strict=True``; ``transformers`` is never imported and nothing is ever
    fetched: the weights come from the dVAE checkpoint or from the optional local ``visual_embed_ckpt`` (a ``BertModel``'s or its encoder's
    ``state_dict``), else they are random and the class says so.  What the reference computes, and this class with it:
      * shallow prompts only -- ``pos`` is added ONCE before the first layer, prompts are prepended once, flow through all layers as full tokens and are
        cut off at the end; there is no final norm.  ``use_deep_prompt: True`` crashes in the reference; here the deep parameters are created (they are
        part of the ``state_dict``) and the forward raises ValueError;
      * a BERT layer is post-LayerNorm with two dropouts (attention probabilities, hidden states; 0.1 each) that follow ``module.training``: live in
        Stage-I training and in the Stage-II teacher forward (no_grad, train mode), off under ``.eval()``;
      * ``forward_tokenizer_features`` defaults to ``return_global=False``.
    ACT never trains the teacher: ``freeze_visual_embed: False`` raises NotImplementedError.  Config keys beyond the reference's:
    ``visual_embed_depth`` / ``visual_embed_heads`` / ``visual_embed_intermediate`` (geometry; bert-base by default) and ``visual_embed_ckpt``."""

    def __init__(self, config, **kwargs):
        super().__init__(config)
        self.visual_embed_type = config.visual_embed_type
        self.visual_embed_dim = config.visual_embed_dim
        self.freeze_visual_embed = config.freeze_visual_embed
        self.num_prompt_token = config.num_prompt_token
        self.use_deep_prompt = config.use_deep_prompt
        if self.visual_embed_dim != 'none' and not self.freeze_visual_embed:
            raise NotImplementedError("freeze_visual_embed: False -- training the language model's own weights is not built (ACT's recipe never trains "
                                      "the teacher Transformer; only prompts and projections learn)")
        self.build_visual_embedding(config)

    def build_visual_embedding(self, config):
        if self.visual_embed_dim == 'none':
            self.visual_embed = None
            return
        depth, heads, inter = _BERT_GEOMETRY.get(self.visual_embed_type, (12, 12, 3072))
        depth = int(config.get("visual_embed_depth", depth))
        heads = int(config.get("visual_embed_heads", heads))
        inter = int(config.get("visual_embed_intermediate", inter))
        D = self.visual_embed_dim
        if D % heads or D // heads not in (32, 64):
            raise ValueError(f"visual_embed_dim {D} / visual_embed_heads {heads}: the attention kernels take head dimensions 32 and 64")
        self.visual_embed = nn.Sequential(_BertEncoderParams(D, heads, inter, depth))
        self.visual_embed_depth = depth
        self.proj_pre = nn.Linear(self.tokens_dims, D)
        self.visual_pos_embed = nn.Sequential(nn.Linear(3, 128), nn.GELU(), nn.Linear(128, D))
        self.proj_post = nn.Linear(D, self.tokens_dims)
        Pn = self.num_prompt_token
        if Pn > 0:
            self.visual_prompt_proj = nn.Identity()
            self.prompt_dropout = nn.Dropout(0.1)
            self.visual_prompt_token = nn.Parameter(torch.zeros(1, Pn, D))
            self.visual_prompt_pos = nn.Parameter(torch.randn(1, Pn, D))
            trunc_normal_(self.visual_prompt_token, std=.02)
            trunc_normal_(self.visual_prompt_pos, std=.02)
            if self.use_deep_prompt:                                   # created as the reference does (:682-689); no forward uses them
                self.deep_prompt_tokens = nn.Parameter(torch.zeros(depth - 1, Pn, D))
                self.deep_prompt_pos = nn.Parameter(torch.randn(depth - 1, Pn, D))
                trunc_normal_(self.deep_prompt_tokens, std=.02)
                trunc_normal_(self.deep_prompt_pos, std=.02)
        else:
            self.visual_prompt_token = None
        ckpt = config.get("visual_embed_ckpt", None)
        if ckpt and str(ckpt).lower() not in ("none", "random", ""):
            self.load_language_model(ckpt)
        else:
            import warnings
            warnings.warn("ACTPromptedDiscreteVAEwithBERT: no visual_embed_ckpt -- the language model is RANDOMLY INITIALISED unless a dVAE checkpoint "
                          "that contains it is loaded afterwards.  Real Stage-I training must point visual_embed_ckpt at a local BertModel (or "
                          "BertModel.encoder) state_dict of " + str(self.visual_embed_type) + "; nothing is ever downloaded.", stacklevel=2)
        for param in self.visual_embed.parameters():
            param.requires_grad = False

    def load_language_model(self, path):
        """``path``: a local ``state_dict`` file of a ``BertModel`` (``encoder.layer.*``, possibly behind ``bert.``) or of its encoder (``layer.*``)"""
        sd = torch.load(path, map_location='cpu')
        sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
        enc = {}
        for k, v in sd.items():
            i = k.find("layer.")
            if i >= 0 and (i == 0 or k[:i] in ("encoder.", "bert.encoder.")):
                enc[k[i:]] = v
        self.visual_embed[0].load_state_dict(enc, strict=True)

    # ---- random draws ------------------------------------------------------------------------------
    def _layer_draws(self, i, B, S, D, H, p_attn, p_hidden, draws, device):
        """-> (masks or None, seeds) of layer i: injected / recorded keep masks when ``draws`` carries or records them, host-drawn Philox seeds else"""
        keys = (f"bert.{i}.attn", f"bert.{i}.hidden1", f"bert.{i}.hidden2")
        if draws is not None and (draws.record or any(draws.has(k) for k in keys)):
            shapes, ps = ((B, H, S, S), (B, S, D), (B, S, D)), (p_attn, p_hidden, p_hidden)
            ms = [draws.get(k, lambda s=s, p=p: (torch.rand(s, device=device) >= p)) if p > 0 else None for k, s, p in zip(keys, shapes, ps)]
            return (ms[0].to(torch.uint8) if ms[0] is not None else None, ms[1].to(torch.float32) if ms[1] is not None else None,
                    ms[2].to(torch.float32) if ms[2] is not None else None), (0, 0, 0)
        return None, None

    def _encode(self, x, draws=None, rng=None):
        """the BertEncoder on x [B,S,D] (already x + pos): every layer one K.BertLayerFn"""
        B, S, D = x.shape
        layers = self.visual_embed[0].layer
        frozen_path = rng is not None                                   # the no_grad teacher forward (forward_tokenizer_features) hands its stream down
        seeds_host = None
        base, ctr = rng if frozen_path else (None, None)
        for i, lyr in enumerate(layers):
            p_attn = lyr.p_attn if self.training else 0.0
            p_hidden = lyr.p_hidden if self.training else 0.0
            masks, seeds = (None, (0, 0, 0))
            seed_dev = None
            if p_attn > 0 or p_hidden > 0:
                masks, seeds = self._layer_draws(i, B, S, D, lyr.num_heads, p_attn, p_hidden, draws, x.device)
                if seeds is None:
                    if frozen_path:                                    # teacher forward: base seed + device counter (fresh masks per captured replay)
                        seeds = tuple((base + 7919 * (3 * i + j + 1) + 0x3c6ef372) & (2 ** 62 - 1) for j in range(3))
                        seed_dev = ctr
                    else:
                        if seeds_host is None:                         # host RNG, one draw for the stack: no device sync
                            seeds_host = torch.randint(0, 2 ** 62, (3 * len(layers),)).tolist()
                        seeds = tuple(seeds_host[3 * i:3 * i + 3])
            x = lyr(x, p_attn, p_hidden, seeds, masks, seed_dev)
        return x

    def _prompt_rows(self, B, draws):
        """dropout(prompt tokens) + prompt positions for every cloud, [B, Pn, D] (incorporate_prompt :738-751), one HIP launch per direction"""
        tok, ppos = self.visual_prompt_token[0], self.visual_prompt_pos[0]
        p = self.prompt_dropout.p if self.training else 0.0
        mask = None
        if p > 0 and draws is not None and (draws.has("prompt.0") or draws.record):
            shape = (B,) + tuple(tok.shape)
            mask = draws.get("prompt.0", lambda: (torch.rand(shape, device=tok.device) >= p)).to(tok.dtype)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if (p > 0 and mask is None) else 0       # host RNG: no device sync
        return K.prompt_rows(tok, ppos, B, p, seed, mask).view(B, tok.shape[0], tok.shape[1])

    def visual_embedding(self, input, center, draws=None, rng=None):
        """models/dvae.py:756-777"""
        if self.use_deep_prompt:
            raise ValueError("use_deep_prompt: True has no forward with a BERT teacher (the reference fails on it too: 'BertEncoder' object is not "
                             "subscriptable); only the shallow prompt form exists")
        if self.visual_embed is None:
            return input
        vp = self.visual_pos_embed
        pos = K.mlp(center, vp[0].weight, vp[0].bias, vp[2].weight, vp[2].bias)
        feature = K.linear(input, self.proj_pre.weight, self.proj_pre.bias)
        if self.visual_prompt_token is None:
            with torch.no_grad():                                      # frozen and promptless: nothing upstream receives a gradient (:766-768)
                feature = self._encode(feature + pos, draws, rng)
        else:
            Pn = self.num_prompt_token
            x = torch.cat((self._prompt_rows(input.shape[0], draws), feature + pos), dim=1)
            feature = self._encode(x, draws, rng)[:, Pn:].contiguous()
        return K.linear(feature, self.proj_post.weight, self.proj_post.bias)

    def forward_tokenizer_features(self, neighborhood, center, return_global=False, draws=None):
        return super().forward_tokenizer_features(neighborhood, center, return_global=return_global, draws=draws)
