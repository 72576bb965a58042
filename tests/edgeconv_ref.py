"""Restatement of the DGCNN classifier's kernels (act_amd/csrc/edgeconv.hip) and of the network (act_amd/models/dgcnn_nets.py) in numpy and
torch-CPU.  Test infrastructure only.

  knn / knn_f64      the feature-space search: float32 arithmetic in the kernel's order (expected bit for bit), and a float64 brute-force ranking
  edge_conv          the MATERIALISED EdgeConv at any dtype: gather, cat(x_j - x_i, x_i), 1x1 conv, BatchNorm over all B*N*k edges, LeakyReLU,
                     max over k; differentiable by autograd
  edge_tail          the same from P, Q (v = P[idx] + Q materialised), with the selected j and sum_j v the kernel also returns
  DgcnnRef           the whole network of torch's own modules under upstream's attribute names, neighbour lists and dropout masks injected
"""
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn

F = np.float32
SLOPE = 0.2


# ---- the search -------------------------------------------------------------------------------------------------------------------------------------
def sqdist_feat(x):
    """x float32 [N,C] -> d float32 [N,N], d[i,j] = sum_c (x_ic - x_jc)^2: channels ascending, every subtraction, product and sum rounded to
    float32 (numpy's float32 ufuncs round once per operation and never contract)"""
    x = np.asarray(x, F)
    d = np.zeros((x.shape[0], x.shape[0]), F)
    for c in range(x.shape[1]):
        diff = (x[:, None, c] - x[None, :, c]).astype(F)
        d = (d + (diff * diff).astype(F)).astype(F)
    return d


def _first_k(d, k):
    """stable sort on (d, index), NaN after everything else (numpy sorts NaN last and keeps equal keys in index order)"""
    o = np.argsort(d, axis=-1, kind="stable")[:, :k]
    return o.astype(np.int32), np.take_along_axis(d, o, -1)


def knn(x, k):
    """x [B,N,C] -> (idx int32 [B,N,k], d2 float32 [B,N,k]) as the kernel computes them"""
    x = np.asarray(x, F)
    out = [_first_k(sqdist_feat(xb), k) for xb in x]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def sqdist_f64(x):
    x = np.asarray(x, np.float64)
    return ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)


def knn_f64(x, k):
    """the float64 brute-force ranking with the same tie rule -> (idx, d2 float64, gap): gap [B,N] = (d_(k+1) - d_(k)) / d_(k+1), the relative
    lead of the k-th neighbour over the first one left out (inf when k == N)"""
    idx, d2, gap = [], [], []
    for xb in np.asarray(x, np.float64):
        d = sqdist_f64(xb)
        o = np.argsort(d, axis=-1, kind="stable")
        s = np.take_along_axis(d, o, -1)
        idx.append(o[:, :k].astype(np.int32)); d2.append(s[:, :k])
        with np.errstate(divide="ignore", invalid="ignore"):
            gap.append((s[:, k] - s[:, k - 1]) / s[:, k] if k < d.shape[0] else np.full(d.shape[0], np.inf))
    return np.stack(idx), np.stack(d2), np.stack(gap)


def lattice(rs, shape, half=2.0):
    """multiples of 1/8 in [-half, half]: every difference, square and sum of a few hundred of them is exact in float32, and ties abound"""
    return (rs.integers(-int(half * 8), int(half * 8) + 1, size=shape) / 8.0).astype(F)


# ---- the EdgeConv, materialised ------------------------------------------------------------------------------------------------------------------------
def _bidx(B, dev=None):
    return torch.arange(B, device=dev)[:, None, None]


def bn_lrelu_max(v, gamma, beta, running_mean, running_var, training, momentum, eps, slope):
    """v [B,N,k,C] -> dict(out [B,N,C], z [B,N,k,C], mean, var (biased), new running_mean / running_var, scale).  train: statistics over all
    B*N*k values of a channel, running statistics moved by momentum with the unbiased variance (count 1: the biased one)"""
    M = v.shape[0] * v.shape[1] * v.shape[2]
    if training:
        mean = v.mean(dim=(0, 1, 2))
        var = ((v - mean) ** 2).mean(dim=(0, 1, 2))
        new_rm = new_rv = None
        if running_mean is not None:
            unb = var * (M / (M - 1)) if M > 1 else var
            new_rm = (1 - momentum) * running_mean + momentum * mean.detach()
            new_rv = (1 - momentum) * running_var + momentum * unb.detach()
    else:
        mean, var, new_rm, new_rv = running_mean, running_var, running_mean, running_var
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * rstd
    z = v * scale + (beta - mean * scale)
    h = torch.where(z > 0, z, slope * z)
    # the maximum is taken where the kernel takes it -- the first largest v (scale >= 0) or the first smallest -- which is a maximum of h by
    # monotonicity and gives ties (a zero gamma ties all k) one definite gradient route
    vn = v.detach().numpy()
    arg = torch.from_numpy(np.where((scale.detach().numpy() >= 0)[None, None, :], vn.argmax(axis=2), vn.argmin(axis=2)))
    return dict(out=torch.gather(h, 2, arg[:, :, None, :])[:, :, 0], h=h, mean=mean, var=var, rstd=rstd, scale=scale, running_mean=new_rm, running_var=new_rv)


def edge_conv(x, idx, W, gamma, beta, running_mean=None, running_var=None, training=True, momentum=0.1, eps=1e-5, slope=SLOPE):
    """x [B,N,C], idx int [B,N,k], W [out, 2C] with columns (x_j - x_i | x_i) -> the dict of bn_lrelu_max; the edge tensor IS formed"""
    B, N, C = x.shape
    xj = x[_bidx(B), idx.long()]                                        # [B,N,k,C]
    xi = x[:, :, None, :].expand_as(xj)
    v = torch.cat((xj - xi, xi), dim=-1) @ W.t()                        # [B,N,k,out]
    r = bn_lrelu_max(v, gamma, beta, running_mean, running_var, training, momentum, eps, slope)
    r["v"] = v
    return r


def edge_tail(P, Q, idx, gamma, beta, running_mean=None, running_var=None, training=True, momentum=0.1, eps=1e-5, slope=SLOPE):
    """P, Q [B,N,C], idx [B,N,k] -> the dict of bn_lrelu_max plus v = P[idx] + Q [B,N,k,C], vsum = sum_j v in ascending j and arg [B,N,C], the
    first j that attains the largest v where scale >= 0 and the smallest v elsewhere"""
    B = P.shape[0]
    v = P[_bidx(B), idx.long()] + Q[:, :, None, :]
    r = bn_lrelu_max(v, gamma, beta, running_mean, running_var, training, momentum, eps, slope)
    vn = v.detach().numpy()
    vs = vn[:, :, 0].copy()
    for j in range(1, vn.shape[2]):
        vs = (vs + vn[:, :, j]).astype(vn.dtype)
    up = (r["scale"].detach().numpy() >= 0)[None, None, :]
    r.update(v=v, vsum=vs, arg=np.where(up, vn.argmax(axis=2), vn.argmin(axis=2)).astype(np.int32))
    return r


def bn_lrelu_rows(x, gamma, beta, running_mean, running_var, training, momentum, eps, slope):
    """BatchNorm1d + LeakyReLU on rows [R,C] -> (y, new running_mean, new running_var)"""
    r = bn_lrelu_max(x[None, :, None, :], gamma, beta, running_mean, running_var, training, momentum, eps, slope)
    return r["out"][0], r["running_mean"], r["running_var"]


def rel(got, ref):
    """the project's measure: max |err| / max(1, max |ref|)"""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / max(1.0, float(ref.abs().max())))


ZERO_GRAD = 1e-12        # a float64 gradient whose largest entry is below this is an exact zero plus rounding: it has no scale of its own


def own(got, ref):
    """max |err| / max |ref|: a tensor against its own largest magnitude (nan when the reference is all zero)"""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    top = float(ref.abs().max())
    return float((got - ref).abs().max()) / top if top > ZERO_GRAD else float("nan")


# ---- the network ------------------------------------------------------------------------------------------------------------------------------------------
class DgcnnRef(nn.Module):
    """upstream's DGCNN classifier, attribute for attribute, run through its own Sequentials on the materialised graph feature [B, 2C, N, k].
    ``draws``: {"knn.1" .. "knn.4": idx [B,N,k], "head.dp1" / "head.dp2": keep-masks}; a missing knn entry is searched here (``knn``, float32
    arithmetic on the float32 cast of the features).  ``trace`` receives, per max (four EdgeConvs, the global max-pool), the smallest
    (lead of the maximum over its runner-up) / max(1, |maximum|); ``gaps`` the per-channel batch standard deviations ahead of bn6 and bn7."""

    def __init__(self, cls_dim=40, k=20, emb_dims=1024, dropout=0.5, widths=(64, 64, 128, 256)):
        super().__init__()
        self.k, self.p = k, dropout
        self.bn1, self.bn2, self.bn3, self.bn4 = (nn.BatchNorm2d(w) for w in widths)
        self.bn5 = nn.BatchNorm1d(emb_dims)
        cin = (3,) + tuple(widths[:3])
        for i, (ci, co, bn) in enumerate(zip(cin, widths, (self.bn1, self.bn2, self.bn3, self.bn4)), 1):
            setattr(self, f"conv{i}", nn.Sequential(nn.Conv2d(2 * ci, co, kernel_size=1, bias=False), bn, nn.LeakyReLU(negative_slope=SLOPE)))
        self.conv5 = nn.Sequential(nn.Conv1d(sum(widths), emb_dims, kernel_size=1, bias=False), self.bn5, nn.LeakyReLU(negative_slope=SLOPE))
        self.linear1 = nn.Linear(2 * emb_dims, 512, bias=False)
        self.bn6 = nn.BatchNorm1d(512)
        self.dp1 = nn.Dropout(p=dropout)
        self.linear2 = nn.Linear(512, 256)
        self.bn7 = nn.BatchNorm1d(256)
        self.dp2 = nn.Dropout(p=dropout)
        self.linear3 = nn.Linear(256, cls_dim)

    @staticmethod
    def _lead(h, dim, trace):
        if trace is not None and h.shape[dim] > 1:
            top = h.detach().topk(2, dim=dim).values
            a, b = top.select(dim, 0), top.select(dim, 1)
            trace.append(float(((a - b) / a.abs().clamp_min(1.0)).min()))

    def _drop(self, h, key, draws):
        if not self.training or self.p == 0:
            return h
        return h * (draws[key].to(h.dtype) / (1.0 - self.p))

    def forward(self, pts, draws=None, trace=None, gaps=None, made=None):
        draws = draws or {}
        B, N, _ = pts.shape
        x, feats = pts.transpose(1, 2), []                                   # [B,C,N]
        for i in range(1, 5):
            if f"knn.{i}" in draws:
                idx = torch.as_tensor(draws[f"knn.{i}"]).long()
            else:
                idx = torch.from_numpy(knn(x.detach().transpose(1, 2).float().numpy(), self.k)[0]).long()
            if made is not None:
                made[f"knn.{i}"] = idx.int()
            xt = x.transpose(1, 2)                                           # [B,N,C]
            xj = xt[_bidx(B), idx]                                           # [B,N,k,C]
            xi = xt[:, :, None, :].expand_as(xj)
            feat = torch.cat((xj - xi, xi), dim=3).permute(0, 3, 1, 2)      # [B,2C,N,k]
            h = getattr(self, f"conv{i}")(feat)
            self._lead(h, 3, trace)
            x = h.max(dim=-1).values
            feats.append(x)
        h = self.conv5(torch.cat(feats, dim=1))                              # [B,emb,N]
        self._lead(h, 2, trace)
        f = torch.cat((h.max(dim=-1).values, h.mean(dim=-1)), dim=1)
        a = self.linear1(f)
        if gaps is not None:
            gaps.append(a.detach().std(dim=0, unbiased=False))
        h = self._drop(Fn.leaky_relu(self.bn6(a), SLOPE), "head.dp1", draws)
        a = self.linear2(h)
        if gaps is not None:
            gaps.append(a.detach().std(dim=0, unbiased=False))
        h = self._drop(Fn.leaky_relu(self.bn7(a), SLOPE), "head.dp2", draws)
        return self.linear3(h), f


# the tiny network of the tests: dgcnn_cls(10, k=8, emb_dims=64, widths=(16, 16, 32, 64)) at B = 4, N = 64
TINY = dict(cls_dim=10, k=8, emb_dims=64, dropout=0.5, widths=(16, 16, 32, 64))
TINY_B, TINY_N = 4, 64
TINY_SEED = 4            # tests/test_edgeconv_host.py::test_tiny_network_seed_leaves_no_maximum_near_a_tie
LEAD = 1e-6              # every selected maximum leads its runner-up by more than LEAD * max(1, |maximum|) in float64
HEAD_GAP = 0.1           # head channels whose four rows have a batch standard deviation below this are dropped by the injected masks


def tiny_ref(seed, dtype):
    from tests.golden.fill import fill_module
    with torch.no_grad():
        m = fill_module(DgcnnRef(**TINY), f"edgeconv.tiny.{seed}.")
    return m.to(dtype).train()


def tiny_inputs(seed):
    """-> (pts float32 [B,N,3], raw keep-masks {key: float32 0/1 [B, width]}, cotangent [B, cls_dim])"""
    from tests.golden.fill import clouds, fill_tensor
    pts = torch.from_numpy(clouds(2000 + seed, TINY_B, TINY_N))
    keep = {k: (fill_tensor(f"edgeconv.tiny.{seed}.{k}", (TINY_B, w), "code") > -0.2).float() for k, w in (("head.dp1", 512), ("head.dp2", 256))}
    cot = fill_tensor(f"edgeconv.tiny.{seed}.cot", (TINY_B, TINY["cls_dim"]), "code") / TINY_B
    return pts, keep, cot


def condition_masks(seed, pts, draws):
    """bn6 and bn7 normalise B = 4 rows in train mode: a channel whose four rows nearly coincide has rstd up to 1 / sqrt(eps) = 316 and turns a
    float32 rounding of 1e-6 ahead of it into 3e-4 behind it, in torch's own float32 run as in any kernel's.  As for the PointNet++ classifier
    (notebook/fp.md), the injected masks also drop every such channel (batch standard deviation below HEAD_GAP in the float64 restatement) in
    all rows; dp1 first, then dp2 behind the conditioned dp1."""
    draws = dict(draws)
    for i, key in enumerate(("head.dp1", "head.dp2")):
        gaps = []
        with torch.no_grad():
            tiny_ref(seed, torch.float64)(pts.double(), draws=draws, gaps=gaps)
        draws[key] = draws[key] * (gaps[i] >= HEAD_GAP).float()[None]
    return draws


def tiny_run(seed, dtype, draws, pts, cot):
    """train-mode forward + backward of the restatement -> (logits, {parameter name: grad}, trace, feature)"""
    model = tiny_ref(seed, dtype)
    trace = []
    out, f = model(pts.to(dtype), draws=draws, trace=trace)
    (out * cot.to(dtype)).sum().backward()
    return out.detach(), {n: p.grad for n, p in model.named_parameters()}, trace, f.detach()


@functools.lru_cache(maxsize=None)
def tiny_host(seed):
    """everything the host can say about the seed, with the neighbour lists searched by the restatement itself ->
    (draws with conditioned masks and the lists, float64 run, float32 run)"""
    pts, keep, cot = tiny_inputs(seed)
    made = {}
    with torch.no_grad():
        tiny_ref(seed, torch.float64)(pts.double(), draws=keep, made=made)
    draws = condition_masks(seed, pts, {**keep, **made})
    return draws, tiny_run(seed, torch.float64, draws, pts, cot), tiny_run(seed, torch.float32, draws, pts, cot)


# upstream's state_dict, key by key (dgcnn_cls() with the default arguments)
def upstream_state_dict_shapes(cls_dim=40, emb_dims=1024, widths=(64, 64, 128, 256)):
    def bn(name, c):
        return [(f"{name}.weight", (c,)), (f"{name}.bias", (c,)), (f"{name}.running_mean", (c,)), (f"{name}.running_var", (c,)),
                (f"{name}.num_batches_tracked", ())]
    cin = (3,) + tuple(widths[:3])
    out = []
    for i, w in enumerate(widths, 1):
        out += bn(f"bn{i}", w)
    out += bn("bn5", emb_dims)
    for i, (ci, co) in enumerate(zip(cin, widths), 1):
        out += [(f"conv{i}.0.weight", (co, 2 * ci, 1, 1))] + bn(f"conv{i}.1", co)
    out += [("conv5.0.weight", (emb_dims, sum(widths), 1))] + bn("conv5.1", emb_dims)
    out += [("linear1.weight", (512, 2 * emb_dims))] + bn("bn6", 512)
    out += [("linear2.weight", (256, 512)), ("linear2.bias", (256,))] + bn("bn7", 256)
    out += [("linear3.weight", (cls_dim, 256)), ("linear3.bias", (cls_dim,))]
    return out
