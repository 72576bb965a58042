"""Torch restatements for PCT (Guo et al., CVM 2021): the offset-attention operator of act_amd/csrc/offset_attn.hip with its hand-written backward,
and the classifier network of act_amd/models/pct.py with the attribute names of the widely used PyTorch port, run through its own Conv1d / bmm /
softmax lines.  Everything runs in the dtype it is handed (float64 as the reference, float32 as the yardstick of rounding).

The upstream repository is not available to these tests: ``layer_table`` restates the port's layer table (names and shapes of every parameter and
buffer) by hand, independently of the modules below, and the tests hold both the restatement and the device network to it."""
import copy

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.pointmlp_ref import fps_from_zero, index_points, knn_of, own, rel          # noqa: F401  (rel / own: the project's two measures)

NORM_EPS = 1e-9

# (B, N, Dq, C): N = 1, small, ragged N, ragged with B > 1, ragged at the smallest widths, the shipped widths, one row past 256, the N limit
OP_SHAPES = [(1, 1, 4, 4), (2, 5, 4, 8), (1, 33, 8, 12), (3, 70, 16, 36), (1, 130, 4, 4), (1, 64, 64, 256), (2, 257, 64, 256), (1, 1024, 32, 64)]


# ---- the operator --------------------------------------------------------------------------------------------------------------------------------------
def offset_attention(q, k, v, x=None):
    """q, k [B,N,Dq], v, x [B,N,C] -> (out [B,N,C], lse [B,N], colsum [B,N]); the port's lines on rows: bmm, softmax over the keys, the division by
    1e-9 + the sum over the queries, bmm"""
    energy = torch.bmm(q, k.transpose(1, 2))
    attention = torch.softmax(energy, dim=-1)
    colsum = attention.sum(dim=1, keepdim=True)
    attention = attention / (NORM_EPS + colsum)
    x_r = torch.bmm(attention.transpose(1, 2), v)
    return (x_r if x is None else x - x_r), torch.logsumexp(energy, dim=-1), colsum.squeeze(1)


def offset_attention_backward(q, k, v, dout, fused):
    """the backward the kernels implement, formula by formula -> (dq, dk, dv, dx or None)"""
    E = torch.bmm(q, k.transpose(1, 2))
    P = torch.softmax(E, dim=-1)
    s = 1.0 / (NORM_EPS + P.sum(dim=1))                                   # [B,N] over j
    x_r = s.unsqueeze(-1) * torch.bmm(P.transpose(1, 2), v)
    g = -dout if fused else dout
    D = (g * x_r).sum(dim=-1)                                             # [B,N] over j
    dP = s.unsqueeze(1) * (torch.bmm(v, g.transpose(1, 2)) - D.unsqueeze(1))
    R = (P * dP).sum(dim=-1, keepdim=True)
    dE = P * (dP - R)
    dq = torch.bmm(dE, k)
    dk = torch.bmm(dE.transpose(1, 2), q)
    dv = torch.bmm(P, s.unsqueeze(-1) * g)
    return dq, dk, dv, (dout if fused else None)


def op_case(B, N, Dq, C, family="plain", seed=0):
    """float64 q, k, v, x and a cotangent, every value a float32.  Families: ``plain`` (gaussian rows, energies of unit spread), ``large`` (q = k with
    rows of norm 12: E_ii = 144, exp overflows without the row maximum), ``unattended`` (every q_i within 0.05 of a unit vector u and k_3 = -30 u: the
    sum of column 3 is about 1e-13, far below the 1e-9 of the normaliser)"""
    rs = np.random.default_rng(1000 * seed + 7 * B + 11 * N + 13 * Dq + 17 * C)
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).double()
    q, k = rs.standard_normal((B, N, Dq)) * Dq ** -0.25, rs.standard_normal((B, N, Dq)) * Dq ** -0.25
    if family == "large":
        q = 12.0 * q / np.linalg.norm(q, axis=-1, keepdims=True)
        k = q
    elif family == "unattended":
        u = np.zeros(Dq); u[0] = 1.0
        q = u + 0.05 * rs.standard_normal((B, N, Dq)) / np.sqrt(Dq)
        k = 0.5 * rs.standard_normal((B, N, Dq)) / np.sqrt(Dq)
        k[:, 3] = -30.0 * u
    q, k = f(q), (f(q) if family == "large" else f(k))
    return dict(q=q, k=k, v=f(rs.standard_normal((B, N, C))), x=f(rs.standard_normal((B, N, C))), dout=f(rs.standard_normal((B, N, C))),
                tied=family == "large")


def op_run(c, dtype, fused=False, tied=False):
    """autograd through the restatement in ``dtype`` -> dict(out, lse, colsum, dq, dk, dv[, dx]); ``tied``: one tensor is both q and k, dq holds
    the sum of both gradients and dk is absent"""
    q = c["q"].to(dtype).clone().requires_grad_(True)
    k = q if tied else c["k"].to(dtype).clone().requires_grad_(True)
    v = c["v"].to(dtype).clone().requires_grad_(True)
    x = c["x"].to(dtype).clone().requires_grad_(True) if fused else None
    out, lse, colsum = offset_attention(q, k, v, x)
    out.backward(c["dout"].to(dtype))
    r = dict(out=out.detach(), lse=lse.detach(), colsum=colsum.detach(), dq=q.grad, dv=v.grad)
    if not tied:
        r["dk"] = k.grad
    if fused:
        r["dx"] = x.grad
    return r


# ---- the network ---------------------------------------------------------------------------------------------------------------------------------------
PCT = dict(points=1024, npoint=(512, 256), nsample=32, width=64, fuse=1024, head=(512, 256))
TINY = dict(points=64, npoint=(32, 16), nsample=8, width=8, fuse=64, head=(512, 256))
RAGGED = dict(TINY, points=70, npoint=(33, 17))
TINY_B, TINY_CLS = 8, 4
# Of seeds 0..19, those whose float32 restatement stays within 2.5e-5 of float64 everywhere (19 and 18 of 20), and among them the one whose SMALLEST
# own-scale gradient error is largest (2.2e-6 both; the head's last two biases, sums of a few terms, aside).  The second bar of the GPU test is four
# times that error tensor by tensor: at the seed with the smallest worst error (ragged 18) one tensor's float32 run happened to land 5.5e-7 from
# float64, a fifth of its neighbours, and four times luck is no bar for a kernel.  tests/test_pct_host.py holds both properties.
TINY_SEED = {"tiny": 1, "ragged": 17}
FEW_TERMS = ("grad:bn7.bias", "grad:linear3.bias")
TINY_CFG = {"tiny": TINY, "ragged": RAGGED}
PCT_PARAMETERS = 2876136


def layer_table(cfg, classes):
    """{state_dict key: shape} of the port's Pct for this configuration, written out from its layer table"""
    t = {}

    def conv(name, cin, cout, bias=False):
        t[name + ".weight"] = (cout, cin, 1)
        if bias:
            t[name + ".bias"] = (cout,)

    def bn(name, c):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            t[f"{name}.{leaf}"] = (c,)
        t[name + ".num_batches_tracked"] = ()

    def pair(prefix, cin, cout):
        conv(prefix + "conv1", cin, cout); conv(prefix + "conv2", cout, cout); bn(prefix + "bn1", cout); bn(prefix + "bn2", cout)

    w = cfg["width"]
    pair("", 3, w)
    pair("gather_local_0.", 2 * w, 2 * w)
    pair("gather_local_1.", 4 * w, 4 * w)
    c = 4 * w
    pair("pt_last.", c, c)
    for i in (1, 2, 3, 4):
        sa = f"pt_last.sa{i}."
        conv(sa + "q_conv", c, c // 4); conv(sa + "k_conv", c, c // 4)
        conv(sa + "v_conv", c, c, bias=True); conv(sa + "trans_conv", c, c, bias=True); bn(sa + "after_norm", c)
    conv("conv_fuse.0", 5 * c, cfg["fuse"]); bn("conv_fuse.1", cfg["fuse"])
    h1, h2 = cfg["head"]
    t["linear1.weight"] = (h1, cfg["fuse"]); bn("bn6", h1)
    t["linear2.weight"], t["linear2.bias"] = (h2, h1), (h2,); bn("bn7", h2)
    t["linear3.weight"], t["linear3.bias"] = (classes, h2), (classes,)
    return t


class Local_op(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = nn.Conv1d(in_channels, out_channels, kernel_size=1, bias=False)
        self.conv2 = nn.Conv1d(out_channels, out_channels, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm1d(out_channels)
        self.bn2 = nn.BatchNorm1d(out_channels)

    def forward(self, x):
        b, n, s, d = x.size()
        x = x.permute(0, 1, 3, 2).reshape(-1, d, s)
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.relu(self.bn2(self.conv2(x)))
        x = F.adaptive_max_pool1d(x, 1).view(b * n, -1)
        return x.reshape(b, n, -1).permute(0, 2, 1)


class SA_Layer(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.q_conv = nn.Conv1d(channels, channels // 4, 1, bias=False)
        self.k_conv = nn.Conv1d(channels, channels // 4, 1, bias=False)
        self.q_conv.weight = self.k_conv.weight
        self.v_conv = nn.Conv1d(channels, channels, 1)
        self.trans_conv = nn.Conv1d(channels, channels, 1)
        self.after_norm = nn.BatchNorm1d(channels)
        self.act = nn.ReLU()
        self.softmax = nn.Softmax(dim=-1)

    def forward(self, x):
        x_q = self.q_conv(x).permute(0, 2, 1)
        x_k = self.k_conv(x)
        x_v = self.v_conv(x)
        energy = torch.bmm(x_q, x_k)
        attention = self.softmax(energy)
        attention = attention / (NORM_EPS + attention.sum(dim=1, keepdim=True))
        x_r = torch.bmm(x_v, attention)
        x_r = self.act(self.after_norm(self.trans_conv(x - x_r)))
        return x + x_r


class Point_Transformer_Last(nn.Module):
    def __init__(self, channels=256):
        super().__init__()
        self.conv1 = nn.Conv1d(channels, channels, kernel_size=1, bias=False)
        self.conv2 = nn.Conv1d(channels, channels, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm1d(channels)
        self.bn2 = nn.BatchNorm1d(channels)
        self.sa1, self.sa2, self.sa3, self.sa4 = SA_Layer(channels), SA_Layer(channels), SA_Layer(channels), SA_Layer(channels)

    def forward(self, x):
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.relu(self.bn2(self.conv2(x)))
        x1 = self.sa1(x)
        x2 = self.sa2(x1)
        x3 = self.sa3(x2)
        x4 = self.sa4(x3)
        return torch.cat((x1, x2, x3, x4), dim=1)


def sample_and_group(xyz, points, fps_idx, idx):
    """the port's sample_and_group with the choices handed in: rows cat(x_j - x_i, x_i) -> (new_xyz [B,S,3], [B,S,k,2D])"""
    new_xyz, new_points = index_points(xyz, fps_idx), index_points(points, fps_idx)
    grouped = index_points(points, idx)
    norm = grouped - new_points.unsqueeze(2)
    return new_xyz, torch.cat([norm, new_points.unsqueeze(2).repeat(1, 1, idx.shape[2], 1)], dim=-1)


class Pct(nn.Module):
    """forward(pts [B,N,3], draws): draws["fps.i"] [B,S_i] and draws["knn.i"] [B,S_i,k] for i = 1, 2 and the keep-masks ["head.dp1"] / ["head.dp2"]
    in train mode; a missing choice is made here (``fps_from_zero``, ``knn_of``) and stored in ``draws``"""

    def __init__(self, output_channels, points, npoint, nsample, width, fuse, head, dropout=0.5):
        super().__init__()
        self.npoint, self.nsample = tuple(npoint), nsample
        self.conv1 = nn.Conv1d(3, width, kernel_size=1, bias=False)
        self.conv2 = nn.Conv1d(width, width, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm1d(width)
        self.bn2 = nn.BatchNorm1d(width)
        self.gather_local_0 = Local_op(2 * width, 2 * width)
        self.gather_local_1 = Local_op(4 * width, 4 * width)
        self.pt_last = Point_Transformer_Last(4 * width)
        self.conv_fuse = nn.Sequential(nn.Conv1d(20 * width, fuse, kernel_size=1, bias=False), nn.BatchNorm1d(fuse), nn.LeakyReLU(negative_slope=0.2))
        self.linear1 = nn.Linear(fuse, head[0], bias=False)
        self.bn6 = nn.BatchNorm1d(head[0])
        self.dp1 = nn.Dropout(p=dropout)
        self.linear2 = nn.Linear(head[0], head[1])
        self.bn7 = nn.BatchNorm1d(head[1])
        self.dp2 = nn.Dropout(p=dropout)
        self.linear3 = nn.Linear(head[1], output_channels)

    def _group(self, xyz, points, stage, draws):
        if f"fps.{stage}" not in draws:
            draws[f"fps.{stage}"] = fps_from_zero(xyz.detach(), self.npoint[stage - 1])
        fps_idx = draws[f"fps.{stage}"].long()
        if f"knn.{stage}" not in draws:
            draws[f"knn.{stage}"] = knn_of(xyz.detach(), index_points(xyz.detach(), fps_idx), self.nsample)
        return sample_and_group(xyz, points, fps_idx, draws[f"knn.{stage}"].long())

    def forward(self, pts, draws):
        xyz = pts
        batch_size = pts.shape[0]
        x = pts.permute(0, 2, 1)
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.relu(self.bn2(self.conv2(x)))
        x = x.permute(0, 2, 1)
        new_xyz, new_feature = self._group(xyz, x, 1, draws)
        feature_0 = self.gather_local_0(new_feature)
        feature = feature_0.permute(0, 2, 1)
        new_xyz, new_feature = self._group(new_xyz, feature, 2, draws)
        feature_1 = self.gather_local_1(new_feature)
        x = self.pt_last(feature_1)
        x = torch.cat([x, feature_1], dim=1)
        x = self.conv_fuse(x)
        x = F.adaptive_max_pool1d(x, 1).view(batch_size, -1)
        x = F.leaky_relu(self.bn6(self.linear1(x)), negative_slope=0.2)
        if self.training:
            x = x * (draws["head.dp1"].to(x.dtype) / (1.0 - self.dp1.p))
        x = F.leaky_relu(self.bn7(self.linear2(x)), negative_slope=0.2)
        if self.training:
            x = x * (draws["head.dp2"].to(x.dtype) / (1.0 - self.dp2.p))
        return self.linear3(x)


def tiny_net(which, seed=None):
    """the float64 tiny network of the tests with every BatchNorm gain in [0.5, 1.5] and every bias and running statistic off its default"""
    cfg = TINY_CFG[which]
    torch.manual_seed(100 + (TINY_SEED[which] if seed is None else seed))
    m = Pct(TINY_CLS, **cfg).double()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(".weight") and p.dim() == 1:
                p.copy_(0.5 + torch.rand_like(p))
            elif name.endswith(".bias"):
                p.copy_(0.1 * torch.randn_like(p))
        for name, b in m.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.1 * torch.randn_like(b))
            elif name.endswith("running_var"):
                b.copy_(1.0 + 0.2 * torch.rand_like(b))
    return m, cfg


def tiny_inputs(which, seed=None):
    cfg = TINY_CFG[which]
    s = TINY_SEED[which] if seed is None else seed
    rs = np.random.default_rng(500 + s)
    pts = torch.from_numpy(rs.uniform(-1, 1, (TINY_B, cfg["points"], 3)).astype(np.float32)).double()
    masks = {"head.dp1": torch.from_numpy((rs.random((TINY_B, cfg["head"][0])) >= 0.5).astype(np.float64)),
             "head.dp2": torch.from_numpy((rs.random((TINY_B, cfg["head"][1])) >= 0.5).astype(np.float64))}
    z, labels = torch.from_numpy(rs.standard_normal((TINY_B, TINY_CLS))), torch.from_numpy(rs.integers(0, TINY_CLS, TINY_B))
    cot = (torch.softmax(z, dim=1) - F.one_hot(labels, TINY_CLS)) / TINY_B          # the cotangent of a mean cross-entropy, as in training
    return pts, masks, cot


def net_run(model, pts, draws, cot, dtype):
    """train-mode forward and backward of a copy of ``model`` in ``dtype`` -> {"logits": .., "grad:<name>": .., "stat:<buffer>": ..}; the tied
    q_conv / k_conv weight is listed once (``named_parameters``), under q_conv"""
    m = copy.deepcopy(model).to(dtype).train()
    logits = m(pts.to(dtype), draws)
    logits.backward(cot.to(dtype))
    out = {"logits": logits.detach()}
    out.update({"grad:" + n: p.grad for n, p in m.named_parameters()})
    out.update({"stat:" + n: b.detach() for n, b in m.named_buffers() if "running" in n})
    return out
