"""Restatement of the feature-propagation kernels (act_amd/csrc/sa.hip: general three-NN, inverse adjacency, interpolation with skipped slots)
in numpy, and of ``PointNetFeaturePropagationAny`` and the three PointNet++ networks in plain torch at any dtype.  Test infrastructure only.

numpy part: the search is written out operation by operation in float32 (tests/sa_ref.sqdist), so ``idx``, ``d2`` and the weights are expected
bit for bit; the interpolation is float64 (or int64 in the tests that use dyadic weights).

torch part: ``FPRef`` / ``SARef`` / ``MsgRef`` and the networks hold torch's own Conv / BatchNorm modules under the attribute names of the
device classes, so one ``fill_module`` call gives both sides the same weights; ``.double()`` makes the float64 oracle, ``.float()`` the run that
the seed checks compare it with.  Every set-abstraction level appends (fps indices, ball-query lists, max-pool arg-max points, margins) to
``trace``."""
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn

from tests import sa_ref as SR
from tests import seg_ref as GR

F = np.float32


# ---- kernels, numpy ------------------------------------------------------------------------------------------------------------------------------
def three_nn(unknown, known):
    """unknown [B,n,3], known [B,m,3] -> (idx int32 [B,n,3], w float32 [B,n,3], d2 float32 [B,n,3]): the first three of a stable sort by
    float32 difference-form distance (equal distances: lower index first).  Slots past m: idx 0, d2 +inf, and r = 1 / (inf + 1e-8) = 0 makes
    their weight exactly 0.  r = 1 / (d2 + 1e-8f), w = r / ((r0 + r1) + r2), every operation rounded to float32."""
    unknown, known = np.asarray(unknown, F), np.asarray(known, F)
    B, n, _ = unknown.shape
    m = known.shape[1]
    k = min(m, 3)
    idx = np.zeros((B, n, 3), np.int32)
    d2 = np.full((B, n, 3), np.inf, F)
    for b in range(B):
        d = SR.sqdist(unknown[b], known[b])
        o = np.argsort(d, axis=-1, kind="stable")[:, :k]
        idx[b, :, :k] = o
        d2[b, :, :k] = np.take_along_axis(d, o, -1)
    r = (F(1.0) / (d2 + F(1e-8))).astype(F)
    s = ((r[..., 0] + r[..., 1]).astype(F) + r[..., 2]).astype(F)
    w = (r / s[..., None]).astype(F)
    return idx, w, d2


def adjacency(idx, m):
    """idx [B,n,3] -> (off int32 [B,m+1], ent int32 [B,3n]): every known point lists the entries 3 * unknown + slot that name it, ascending.
    The slots of weight 0 (m < 3) name point 0 and are listed; the backward skips them."""
    return GR.adjacency(np.asarray(idx), m)


def interp_fwd(feat, idx, w, dtype=np.float64):
    """feat [B,m,C], idx [B,n,3], w [B,n,3] -> [B,n,C]: slots of weight 0 are skipped, never read"""
    feat, w = np.asarray(feat).astype(dtype), np.asarray(w).astype(dtype)
    B, n, _ = idx.shape
    out = np.zeros((B, n, feat.shape[2]), dtype)
    for b in range(B):
        for k in range(3):
            live = w[b, :, k] != 0
            out[b, live] += w[b, live, k, None] * feat[b, idx[b, live, k]]
    return out


def interp_bwd(dout, idx, w, m, dtype=np.float64):
    """dout [B,n,C] -> dfeat [B,m,C], the adjoint of interp_fwd in ``feat``"""
    dout, w = np.asarray(dout).astype(dtype), np.asarray(w).astype(dtype)
    B, n, _ = idx.shape
    out = np.zeros((B, m, dout.shape[2]), dtype)
    for b in range(B):
        for k in range(3):
            live = w[b, :, k] != 0
            np.add.at(out[b], idx[b, live, k], w[b, live, k, None] * dout[b, live])
    return out


def lattice_pair(rs, B, n, m, half=1.0):
    """unknown / known clouds on the 1/8 lattice in [-half, half]: every squared distance is exact in float32"""
    return SR.lattice_cloud(rs, B, n, -half, half), SR.lattice_cloud(rs, B, m, -half, half)


def third_fourth_tie(unknown, known):
    """bool [B,n]: the third and the fourth smallest float32 distances are equal (the reference's torch.sort fixes no order there)"""
    B, n, _ = unknown.shape
    out = np.zeros((B, n), bool)
    if known.shape[1] > 3:
        for b in range(B):
            d = np.sort(SR.sqdist(unknown[b], known[b]), axis=-1)
            out[b] = d[:, 2] == d[:, 3]
    return out


# ---- modules, torch at any dtype -------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy()


def _sqd(a, b):
    """a [S,3], b [N,3] numpy of one dtype -> [S,N], the difference form in that dtype"""
    d = a[:, None, :] - b[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def fps(x, npoint):
    """x numpy [B,N,3] -> int64 [B,npoint]: start at index 0, running minimum of difference-form distances in x's dtype, first arg-max"""
    B, N, _ = x.shape
    out = np.zeros((B, npoint), np.int64)
    for b in range(B):
        temp = np.full(N, 1e10, x.dtype)
        old = 0
        for j in range(1, npoint):
            temp = np.minimum(temp, _sqd(x[b], x[b, old][None])[:, 0])
            old = int(np.argmax(temp))
            out[b, j] = old
    return out


def ball(x, q, radius, nsample):
    """inclusive radius search in x's dtype: the lowest nsample indices with d2 <= r * r, the rest of the row the first hit"""
    B, S = q.shape[:2]
    r = x.dtype.type(radius)
    r2 = r * r
    idx = np.zeros((B, S, nsample), np.int64)
    for b in range(B):
        hit = _sqd(q[b], x[b]) <= r2
        for s in range(S):
            h = np.flatnonzero(hit[s])[:nsample]
            assert len(h), "a centre is a cloud point: it reaches itself"
            idx[b, s, :len(h)] = h
            idx[b, s, len(h):] = h[0]
    return idx


def _pool(v, pid, trace, fps_idx, bq):
    """v [B,C,ns,S] after ReLU, pid int64 [B,S,ns] = the point every row holds -> max over ns [B,C,S]; records the arg-max POINT and the margin to
    the best row of another point (repeated rows of one point are one candidate; an all-zero column, whose gradient is zero, has margin inf)"""
    mx, arg = v.max(dim=2)                                               # [B,C,S]
    p = torch.from_numpy(pid).permute(0, 2, 1).unsqueeze(1).expand_as(v)  # [B,C,ns,S]
    win = torch.gather(p, 2, arg.unsqueeze(2))                           # [B,C,1,S]
    other = torch.where(p == win, torch.full_like(v, -float("inf")), v).max(dim=2)[0]
    margin = torch.where(mx > 0, mx - other, torch.full_like(mx, float("inf")))     # no other point in the group: inf
    trace.append(dict(fps=fps_idx, bq=bq, arg=_np(win.squeeze(2)), live=_np(mx > 0), margin=float(margin.min().detach())))
    return mx


def _bidx(B):
    return torch.arange(B)[:, None, None]


class SARef(nn.Module):
    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all):
        super().__init__()
        self.npoint, self.radius, self.nsample, self.group_all = npoint, radius, nsample, group_all
        self.mlp_convs, self.mlp_bns = nn.ModuleList(), nn.ModuleList()
        last = in_channel
        for out in mlp:
            self.mlp_convs.append(nn.Conv2d(last, out, 1))
            self.mlp_bns.append(nn.BatchNorm2d(out))
            last = out

    def forward(self, xyz, points, trace):
        x = xyz.transpose(1, 2)
        p = None if points is None else points.transpose(1, 2)
        B, N, _ = x.shape
        if self.group_all:
            new_xyz = torch.zeros(B, 1, 3, dtype=x.dtype)
            g = (x if p is None else torch.cat((x, p), dim=-1)).unsqueeze(1)              # [B,1,N,3+D]
            pid, fi, bq = np.broadcast_to(np.arange(N), (B, 1, N)).copy(), None, None
        else:
            fi = fps(_np(x), self.npoint)
            new_xyz = x[torch.arange(B)[:, None], torch.from_numpy(fi)]
            pid = bq = ball(_np(x), _np(new_xyz), self.radius, self.nsample)
            t = torch.from_numpy(pid)
            g = x[_bidx(B), t] - new_xyz[:, :, None, :]
            if p is not None:
                g = torch.cat((g, p[_bidx(B), t]), dim=-1)
        v = g.permute(0, 3, 2, 1)                                          # [B,C,ns,S]
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            v = Fn.relu(bn(conv(v)))
        return new_xyz.transpose(1, 2), _pool(v, pid, trace, fi, bq)


class MsgRef(nn.Module):
    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list):
        super().__init__()
        self.npoint, self.radius_list, self.nsample_list = npoint, radius_list, nsample_list
        self.conv_blocks, self.bn_blocks = nn.ModuleList(), nn.ModuleList()
        for mlp in mlp_list:
            convs, bns = nn.ModuleList(), nn.ModuleList()
            last = in_channel + 3
            for out in mlp:
                convs.append(nn.Conv2d(last, out, 1))
                bns.append(nn.BatchNorm2d(out))
                last = out
            self.conv_blocks.append(convs)
            self.bn_blocks.append(bns)

    def forward(self, xyz, points, trace):
        x = xyz.transpose(1, 2)
        p = None if points is None else points.transpose(1, 2)
        B = x.shape[0]
        fi = fps(_np(x), self.npoint)
        new_xyz = x[torch.arange(B)[:, None], torch.from_numpy(fi)]
        outs = []
        for k, radius in enumerate(self.radius_list):
            pid = ball(_np(x), _np(new_xyz), radius, self.nsample_list[k])
            t = torch.from_numpy(pid)
            g = x[_bidx(B), t] - new_xyz[:, :, None, :]
            if p is not None:
                g = torch.cat((p[_bidx(B), t], g), dim=-1)                  # (features, xyz): the reference's order in this class
            v = g.permute(0, 3, 2, 1)
            for conv, bn in zip(self.conv_blocks[k], self.bn_blocks[k]):
                v = Fn.relu(bn(conv(v)))
            outs.append(_pool(v, pid, trace, fi, pid))
        return new_xyz.transpose(1, 2), torch.cat(outs, dim=1)


class FPRef(nn.Module):
    """the reference's PointNetFeaturePropagation with the project's rules: difference-form distances, stable (distance, index) order, the
    weights normalised over min(S, 3) columns (the reference's S == 1 branch is the one-column case: weight 1)"""

    def __init__(self, in_channel, mlp):
        super().__init__()
        self.mlp_convs, self.mlp_bns = nn.ModuleList(), nn.ModuleList()
        last = in_channel
        for out in mlp:
            self.mlp_convs.append(nn.Conv1d(last, out, 1))
            self.mlp_bns.append(nn.BatchNorm1d(out))
            last = out

    def forward(self, xyz1, xyz2, points1, points2, trace=None):
        x1, x2, p2 = xyz1.transpose(1, 2), xyz2.transpose(1, 2), points2.transpose(1, 2)
        B, N, _ = x1.shape
        S = x2.shape[1]
        k = min(S, 3)
        a, b = _np(x1), _np(x2)
        d = np.stack([_sqd(a[i], b[i]) for i in range(B)])                 # [B,N,S] in the module's dtype
        o = np.argsort(d, axis=-1, kind="stable")[:, :, :k]
        if trace is not None:
            trace.append(dict(nn=np.sort(o, axis=-1)))                   # the neighbour SETS: an order change inside them only reorders a sum
        d3 = torch.from_numpy(np.take_along_axis(d, o, -1))
        r = 1.0 / (d3 + 1e-8)
        w = r / r.sum(dim=2, keepdim=True)
        interp = (p2[_bidx(B), torch.from_numpy(o)] * w.unsqueeze(-1)).sum(dim=2)         # [B,N,D2]
        v = interp if points1 is None else torch.cat((points1.transpose(1, 2), interp), dim=-1)
        v = v.transpose(1, 2)
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            v = Fn.relu(bn(conv(v)))
        return v


def _drop(x, p, training, draws, key):
    if not training or p == 0:
        return x
    return x * (draws[key].to(x.dtype) / (1.0 - p))


# the SA levels of the three networks at their published sizes; the tests override npoint / radius / nsample
CLS_SA = dict(sa1=(512, 0.2, 32), sa2=(128, 0.4, 64))
PART_SA = dict(sa1=(512, [0.1, 0.2, 0.4], [32, 64, 128]), sa2=(128, [0.4, 0.8], [64, 128]))
SEM_SA = dict(sa1=(1024, 0.1, 32), sa2=(256, 0.2, 32), sa3=(64, 0.4, 32), sa4=(16, 0.8, 32))


class ClsSSGRef(nn.Module):
    def __init__(self, cls_dim, normal_channel=False, **sa):
        super().__init__()
        lv = {**CLS_SA, **sa}
        self.normal_channel = normal_channel
        self.sa1 = SARef(*lv["sa1"], (3 if normal_channel else 0) + 3, [64, 64, 128], False)
        self.sa2 = SARef(*lv["sa2"], 128 + 3, [128, 128, 256], False)
        self.sa3 = SARef(None, None, None, 256 + 3, [256, 512, 1024], True)
        self.fc1, self.bn1, self.drop1 = nn.Linear(1024, 512), nn.BatchNorm1d(512), nn.Dropout(0.4)
        self.fc2, self.bn2, self.drop2 = nn.Linear(512, 256), nn.BatchNorm1d(256), nn.Dropout(0.4)
        self.fc3 = nn.Linear(256, cls_dim)

    def forward(self, pts, draws=None, trace=None, gaps=None):
        """pts [B,N,3|6] -> logits [B,cls_dim]; ``gaps`` collects the two pre-BatchNorm activations of the head"""
        trace = [] if trace is None else trace
        x = pts.transpose(1, 2)
        xyz, norm = x[:, :3], (x[:, 3:] if self.normal_channel else None)
        l1x, l1p = self.sa1(xyz, norm, trace)
        l2x, l2p = self.sa2(l1x, l1p, trace)
        _, l3p = self.sa3(l2x, l2p, trace)
        h = l3p.reshape(pts.shape[0], 1024)
        a1 = self.fc1(h)
        h = _drop(Fn.relu(self.bn1(a1)), 0.4, self.training, draws, "head.drop1")
        a2 = self.fc2(h)
        h = _drop(Fn.relu(self.bn2(a2)), 0.4, self.training, draws, "head.drop2")
        if gaps is not None:
            gaps += [a1.detach(), a2.detach()]
        return self.fc3(h)


class PartSegMsgRef(nn.Module):
    def __init__(self, num_part, normal_channel=False, **sa):
        super().__init__()
        lv = {**PART_SA, **sa}
        extra = 3 if normal_channel else 0
        self.normal_channel = normal_channel
        self.sa1 = MsgRef(*lv["sa1"], 3 + extra, [[32, 32, 64], [64, 64, 128], [64, 96, 128]])
        self.sa2 = MsgRef(*lv["sa2"], 128 + 128 + 64, [[128, 128, 256], [128, 196, 256]])
        self.sa3 = SARef(None, None, None, 512 + 3, [256, 512, 1024], True)
        self.fp3 = FPRef(1536, [256, 256])
        self.fp2 = FPRef(576, [256, 128])
        self.fp1 = FPRef(150 + extra, [128, 128])
        self.conv1, self.bn1, self.drop1 = nn.Conv1d(128, 128, 1), nn.BatchNorm1d(128), nn.Dropout(0.5)
        self.conv2 = nn.Conv1d(128, num_part, 1)

    def forward(self, pts, cls_label, draws=None, trace=None):
        """pts [B,3|6,N], cls_label [B,16] one-hot -> log-probabilities [B,N,num_part]"""
        trace = [] if trace is None else trace
        B, _, N = pts.shape
        l0p, l0x = pts, pts[:, :3]
        l1x, l1p = self.sa1(l0x, l0p, trace)
        l2x, l2p = self.sa2(l1x, l1p, trace)
        l3x, l3p = self.sa3(l2x, l2p, trace)
        l2p = self.fp3(l2x, l3x, l2p, l3p, trace)
        l1p = self.fp2(l1x, l2x, l1p, l2p, trace)
        onehot = cls_label.to(pts.dtype).view(B, 16, 1).expand(B, 16, N)
        l0p = self.fp1(l0x, l1x, torch.cat((onehot, l0x, l0p), dim=1), l1p, trace)
        h = _drop(Fn.relu(self.bn1(self.conv1(l0p))), 0.5, self.training, draws, "head.drop1")
        return Fn.log_softmax(self.conv2(h), dim=1).transpose(1, 2)


class SemSegRef(nn.Module):
    def __init__(self, num_classes, **sa):
        super().__init__()
        lv = {**SEM_SA, **sa}
        self.sa1 = SARef(*lv["sa1"], 9 + 3, [32, 32, 64], False)
        self.sa2 = SARef(*lv["sa2"], 64 + 3, [64, 64, 128], False)
        self.sa3 = SARef(*lv["sa3"], 128 + 3, [128, 128, 256], False)
        self.sa4 = SARef(*lv["sa4"], 256 + 3, [256, 256, 512], False)
        self.fp4 = FPRef(768, [256, 256])
        self.fp3 = FPRef(384, [256, 256])
        self.fp2 = FPRef(320, [256, 128])
        self.fp1 = FPRef(128, [128, 128, 128])
        self.conv1, self.bn1, self.drop1 = nn.Conv1d(128, 128, 1), nn.BatchNorm1d(128), nn.Dropout(0.5)
        self.conv2 = nn.Conv1d(128, num_classes, 1)

    def forward(self, pts, draws=None, trace=None):
        """pts [B,9,N] -> log-probabilities [B,N,num_classes]"""
        trace = [] if trace is None else trace
        l0p, l0x = pts, pts[:, :3]
        l1x, l1p = self.sa1(l0x, l0p, trace)
        l2x, l2p = self.sa2(l1x, l1p, trace)
        l3x, l3p = self.sa3(l2x, l2p, trace)
        l4x, l4p = self.sa4(l3x, l3p, trace)
        l3p = self.fp4(l3x, l4x, l3p, l4p, trace)
        l2p = self.fp3(l2x, l3x, l2p, l3p, trace)
        l1p = self.fp2(l1x, l2x, l1p, l2p, trace)
        l0p = self.fp1(l0x, l1x, None, l1p, trace)
        h = _drop(Fn.relu(self.bn1(self.conv1(l0p))), 0.5, self.training, draws, "head.drop1")
        return Fn.log_softmax(self.conv2(h), dim=1).transpose(1, 2)


def traces_agree(t32, t64):
    """every FPS index, ball-query list, live max-pool arg-max point and three-NN neighbour set of two runs agree"""
    assert len(t32) == len(t64) > 0
    for a, b in zip(t32, t64):
        if "nn" in a:
            if not np.array_equal(a["nn"], b["nn"]):
                return False
            continue
        for k in ("fps", "bq"):
            if a[k] is not None and not np.array_equal(a[k], b[k]):
                return False
        if not np.array_equal(a["live"], b["live"]) or not np.array_equal(a["arg"][a["live"]], b["arg"][b["live"]]):
            return False
    return True


# ---- the tiny network cases shared by the host test (which checks the seeds) and the GPU test -------------------------------------------------------
TINY_B, TINY_N = 2, 128
TINY = {
    "cls": dict(ref=ClsSSGRef, args=(10,), sa=dict(sa1=(32, 0.3, 8), sa2=(8, 0.6, 8)), channels=3, drops={"head.drop1": 512, "head.drop2": 256},
                p=0.4),
    "part": dict(ref=PartSegMsgRef, args=(50,), sa=dict(sa1=(32, [0.2, 0.3, 0.5], [8, 8, 8]), sa2=(8, [0.5, 0.8], [8, 8])), channels=3,
                 drops={"head.drop1": 128}, p=0.5),
    "sem": dict(ref=SemSegRef, args=(13,), sa=dict(sa1=(32, 0.3, 8), sa2=(16, 0.5, 8), sa3=(8, 0.8, 8), sa4=(4, 1.2, 8)), channels=9,
                drops={"head.drop1": 128}, p=0.5),
}
TINY_SEEDS = {"cls": 1, "part": 13, "sem": 37}          # checked by tests/test_fp_host.py::test_network_seeds_leave_no_decision_near_a_tie
CLS_GAP = 0.1


def _condition_cls_masks(seed, pts, keep):
    """The classifier's head runs train-mode BatchNorm over B = 2 rows: a channel's output is d / sqrt(d * d + eps) with d half the difference of
    its two rows, whose slope at d = 0 is 1 / sqrt(eps) = 316 -- a float32 rounding of 1e-6 ahead of it becomes 3e-4 behind it, in torch's own
    float32 run as much as in any kernel's.  The injected dropout masks therefore also drop, in both rows, every channel with |d| < CLS_GAP in the
    float64 restatement (slope <= eps / CLS_GAP^3 = 0.01), which keeps the forward well conditioned.  The price: the two saturated layers
    attenuate everything behind them, so the gradients of fc1 and of the whole backbone are 1e-7 ... 2e-5 in magnitude, and the backward of a
    saturated two-row BatchNorm cancels terms of order |g| to a result of order |g| * eps / d^2, which leaves them a relative float32 error of
    about 1e-3.  An absolute bar says nothing about such tensors: they are compared on their own scale (``own_scale_errors``, OWN_SCALE_BAR)."""
    for i, key in enumerate(("head.drop1", "head.drop2")):
        gaps = []
        with torch.no_grad():
            tiny_ref("cls", seed, torch.float64)(pts.double(), draws=keep, gaps=gaps)
        a = gaps[i]
        keep[key] = keep[key] * ((a[0] - a[1]).abs() / 2 >= CLS_GAP).float()[None]
    return keep


@functools.lru_cache(maxsize=None)
def tiny_inputs(name, seed):
    """-> (pts float32 in the network's layout, extra positional inputs, dropout keep-masks {key: float32 0/1 rows}, cotangent).  The cotangent
    is N(0, 1) divided by the number of rows, the scale of a mean loss: the parameter gradients of the two segmentation networks are then
    between 2e-2 and order 1 (the classifier's: see _condition_cls_masks), and the conv biases ahead of a train-mode BatchNorm, whose exact
    gradient is zero, carry float32 rounding noise far below the tests' bar."""
    from tests.golden.fill import clouds, fill_tensor
    c = TINY[name]
    xyz = torch.from_numpy(clouds(1000 + seed, TINY_B, TINY_N))
    rest = fill_tensor(f"fp.tiny.{name}.{seed}.rest", (TINY_B, TINY_N, c["channels"] - 3), "code") if c["channels"] > 3 else None
    pts = xyz if rest is None else torch.cat((xyz, rest), dim=-1)
    rows = TINY_B if name == "cls" else TINY_B * TINY_N
    keep = {k: (fill_tensor(f"fp.tiny.{name}.{seed}.{k}", (rows, w), "code") > -0.2).float() for k, w in c["drops"].items()}
    if name == "cls":
        keep = _condition_cls_masks(seed, pts, keep)
        extra, cot = (), fill_tensor(f"fp.tiny.{name}.{seed}.cot", (TINY_B, c["args"][0]), "code") / TINY_B
    else:
        pts = pts.transpose(1, 2).contiguous()
        cot = fill_tensor(f"fp.tiny.{name}.{seed}.cot", (TINY_B, TINY_N, c["args"][0]), "code") / (TINY_B * TINY_N)
        extra = (Fn.one_hot(torch.tensor([3, 11]), 16).float(),) if name == "part" else ()
    return pts, extra, keep, cot


def tiny_ref(name, seed, dtype):
    """the restated network with fill.py's weights -> (model in train mode, keep-masks shaped for its head)"""
    from tests.golden.fill import fill_module
    c = TINY[name]
    return fill_module(c["ref"](*c["args"], **c["sa"]), f"fp.tiny.{name}.{seed}.").to(dtype).train()


def tiny_run(name, seed, dtype):
    """train-mode forward + backward of the restatement -> (out, {parameter name: grad}, trace)"""
    pts, extra, keep, cot = tiny_inputs(name, seed)
    model = tiny_ref(name, seed, dtype)
    draws = {k: (v if name == "cls" else v.view(TINY_B, TINY_N, -1).transpose(1, 2)) for k, v in keep.items()}
    trace = []
    out = model(pts.to(dtype), *extra, draws=draws, trace=trace)
    (out * cot.to(dtype)).sum().backward()
    return out.detach(), {n: p.grad for n, p in model.named_parameters()}, trace


# ---- gradients on their own scale --------------------------------------------------------------------------------------------------------------------
# max |got - ref| / max |ref| per tensor: a measure under which a backward that returns zeros, or one that is off by a few per cent, fails whatever
# the tensor's magnitude.  OWN_SCALE_REF is what the restatement's own float32 run may differ from its float64 run at the seeds (asserted on the
# host; measured 2.4e-3 / 1.2e-5 / 2.4e-5, the classifier's being the cancellation described in _condition_cls_masks); the device, whose
# summation orders differ from torch's float32 as torch's float32 differs from float64, gets four times that.
OWN_SCALE_REF = {"cls": 5e-3, "part": 5e-5, "sem": 5e-5}
OWN_SCALE_BAR = {k: 4 * v for k, v in OWN_SCALE_REF.items()}
GRAD_FLOOR = 1e-8               # every gradient with a non-zero exact value is at least this large at the seeds (asserted on the host)


def exact_zero_gradient(name):
    """a conv / fc bias directly ahead of a train-mode BatchNorm: its exact gradient is zero, so it has no scale of its own"""
    return name.endswith(".bias") and not ("bns." in name or "bn_blocks." in name or name.split(".")[-2] in ("bn1", "bn2", "fc3", "conv2"))


def own_scale_errors(got, ref):
    """{name: max |got - ref| / max |ref|} over the parameters whose exact gradient is not zero"""
    out = {}
    for n, r in ref.items():
        if not exact_zero_gradient(n):
            r = r.detach().double().cpu()
            out[n] = float((got[n].detach().double().cpu() - r).abs().max() / r.abs().max())
    return out
