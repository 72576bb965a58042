"""GPU: S3DIS semantic segmentation (act_amd/models/semseg.py, csrc/seg.hip) -- three-NN, row interpolation, log-softmax / weighted NLL,
confusion matrix, the whole model against the reference's own module (g18) and against a float64 CPU restatement at full geometry,
checkpoints, and a short synthetic training run."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.conftest import golden, ROOT
from tests.golden.fill import fill_module

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _nn3_f64(xyz, ctr):
    """float64 distances of the float32 inputs, stable ascending order -> (order [B,N,G], d [B,N,G])"""
    d = ((xyz[:, :, None, :].astype(np.float64) - ctr[:, None, :, :].astype(np.float64)) ** 2).sum(-1)
    return np.argsort(d, axis=-1, kind="stable"), d


# ---- three-NN ---------------------------------------------------------------------------------------------------------------
def test_three_nn_order_weights_and_adjacency(dev):
    from act_amd import kernels as K
    rs = np.random.RandomState(0)
    B, N, G = 3, 2048, 128
    xyz = rs.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    xyz[:, :, 2] += 1.5
    ctr = np.stack([xyz[b, rs.choice(N, G, replace=False)] for b in range(B)])      # centres are cloud points (as FPS picks them)
    idx, w, off, ent = K.three_nn(torch.from_numpy(xyz).to(dev), torch.from_numpy(ctr).to(dev))
    idx, w, off, ent = idx.cpu().numpy(), w.cpu().numpy(), off.cpu().numpy(), ent.cpu().numpy()
    order, d = _nn3_f64(xyz, ctr)
    ds = np.take_along_axis(d, order[:, :, :4], -1)
    gap = np.diff(ds, axis=-1).min(-1)
    clear = gap > 1e-5 * (1 + ds[:, :, 3])                              # rows without near-ties among the 4 nearest
    assert clear.mean() > 0.99
    np.testing.assert_array_equal(idx[clear], order[:, :, :3][clear])
    # coincident points: every centre's own point picks it first, at distance 0, with weight ~1
    for b in range(B):
        for g in range(G):
            n = np.where((xyz[b] == ctr[b, g]).all(-1))[0][0]
            assert idx[b, n, 0] == g and w[b, n, 0] > 1 - 1e-5
    r = 1.0 / (np.take_along_axis(d, idx.astype(np.int64), -1) + 1e-8)
    np.testing.assert_allclose(w, r / r.sum(-1, keepdims=True), rtol=1e-6, atol=1e-12)
    # inverse adjacency: per cloud and centre, the entries 3n+k that chose it, in increasing order
    for b in range(B):
        flat = idx[b].reshape(-1)
        assert off[b, 0] == 0 and off[b, G] == 3 * N
        for g in range(G):
            np.testing.assert_array_equal(ent[b, off[b, g]:off[b, g + 1]], np.where(flat == g)[0])


def test_three_nn_ties_go_to_lower_index(dev):
    from act_amd import kernels as K
    ctr = np.array([[[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, 2], [0, -1, 0], [5, 5, 5]]], np.float32)
    xyz = np.array([[[0, 0, 0], [0, 0, 1], [5, 5, 5], [1, 0, 0]]], np.float32)
    idx, w, _, _ = K.three_nn(torch.from_numpy(xyz).to(dev), torch.from_numpy(ctr).to(dev))
    idx, w = idx.cpu().numpy()[0], w.cpu().numpy()[0]
    assert idx[0].tolist() == [0, 1, 2]                                 # four centres at distance 1: the three lowest indices
    np.testing.assert_allclose(w[0], [1 / 3] * 3, rtol=1e-6)
    assert idx[1].tolist() == [3, 0, 1]                                 # d = 1, then 2, 2, 2, 2: lower indices first
    assert idx[2][0] == 5 and idx[3][0] == 0                            # coincident points
    assert w[2][0] > 1 - 1e-6 and w[3][0] > 1 - 1e-6
    dup = np.array([[[0, 0, 0], [1, 1, 1], [0, 0, 0], [2, 2, 2]]], np.float32)          # duplicated centre coordinates
    idx2, _, _, _ = K.three_nn(torch.zeros(1, 1, 3, device=dev), torch.from_numpy(dup).to(dev))
    assert idx2.cpu().numpy()[0, 0].tolist() == [0, 2, 1]


# ---- interpolation ----------------------------------------------------------------------------------------------------------
def _nn3_case(dev, B=2, N=1024, G=128, seed=1):
    from act_amd import kernels as K
    rs = np.random.RandomState(seed)
    xyz = rs.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    ctr = np.stack([xyz[b, rs.choice(N, G, replace=False)] for b in range(B)])
    return xyz, K.three_nn(torch.from_numpy(xyz).to(dev), torch.from_numpy(ctr).to(dev))


def test_interp_rows_forward_backward(dev):
    from act_amd import kernels as K
    B, N, G, C = 2, 1024, 128, 1536
    xyz, nn3 = _nn3_case(dev, B, N, G)
    idx, w = nn3[0].cpu().long(), nn3[1].cpu().double()
    rs = np.random.RandomState(2)
    P = torch.from_numpy(rs.standard_normal((B * G, C)).astype(np.float32))
    dY = torch.from_numpy(rs.standard_normal((B * N, C)).astype(np.float32))
    rows = (idx + (torch.arange(B) * G).view(B, 1, 1)).reshape(B * N, 3)
    P64 = P.double().requires_grad_(True)
    ref = (P64[rows] * w.reshape(B * N, 3, 1)).sum(1)
    ref.backward(dY.double())
    Pd = P.to(dev).requires_grad_(True)
    Y = K.interp_rows(Pd, nn3, B, N, G)
    assert (Y.detach().cpu().double() - ref.detach()).abs().max().item() <= 1e-5
    Y.backward(dY.to(dev))
    assert (Pd.grad.cpu().double() - P64.grad).abs().max().item() <= 1e-5
    dP2 = K.interp_rows_bwd(dY.to(dev), nn3[2], nn3[3], nn3[1], B, N, G)
    assert torch.equal(dP2, Pd.grad)                                    # deterministic gather: bit-identical run to run
    # the xyz / bias epilogue of the per-group form
    wx = torch.from_numpy(rs.standard_normal((C, 3)).astype(np.float32))
    bias = torch.from_numpy(rs.standard_normal(C).astype(np.float32))
    Y2 = K.interp_rows_fwd(P.to(dev), nn3[0], nn3[1], B, N, G, xyz=torch.from_numpy(xyz).to(dev).reshape(B * N, 3), wxyz=wx.to(dev),
                           bias=bias.to(dev))
    ref2 = ref.detach() + torch.from_numpy(xyz).double().reshape(B * N, 3) @ wx.double().t() + bias.double()
    assert (Y2.cpu().double() - ref2).abs().max().item() <= 1e-5
    dwx, db = K.interp_xyz_grad(dY.to(dev), torch.from_numpy(xyz).to(dev).reshape(B * N, 3))
    rdw = dY.double().t() @ torch.from_numpy(xyz).double().reshape(B * N, 3)
    assert (dwx.cpu().double() - rdw).abs().max().item() <= 1e-5 * rdw.abs().max().item()
    assert (db.cpu().double() - dY.double().sum(0)).abs().max().item() <= 1e-5 * dY.double().sum(0).abs().max().item()


# ---- log-softmax, weighted NLL, confusion matrix ------------------------------------------------------------------------------
def test_log_softmax_weighted_nll(dev):
    from act_amd import kernels as K
    rs = np.random.RandomState(3)
    R, C = 5000, 13
    z = torch.from_numpy((3 * rs.standard_normal((R, C))).astype(np.float32))
    t = torch.from_numpy(rs.randint(0, C, size=R))
    wt = torch.from_numpy((0.5 + rs.rand(C)).astype(np.float32))
    z64 = z.double().requires_grad_(True)
    lp64 = F.log_softmax(z64, dim=1)
    loss64 = F.nll_loss(lp64, t, wt.double())
    loss64.backward()
    zd = z.to(dev).requires_grad_(True)
    lp = K.log_softmax(zd)
    loss, correct = K.nll_weighted(lp, t.to(dev), wt.to(dev))
    loss.backward()
    assert (lp.detach().cpu().double() - lp64.detach()).abs().max().item() <= 1e-5
    assert abs(loss.item() - loss64.item()) <= 1e-5
    assert (zd.grad.cpu().double() - z64.grad).abs().max().item() <= 1e-6
    assert correct.item() == int((z.argmax(1) == t).sum())
    loss_b, _ = K.nll_weighted(lp.detach(), t.to(dev), wt.to(dev))
    assert torch.equal(loss_b, loss.detach())                            # fixed-order reduction: bit-identical


def test_confusion_and_metrics(dev):
    from act_amd import kernels as K
    from act_amd.tools.runner_semseg import seg_metrics
    rs = np.random.RandomState(4)
    R, C = 20000, 13
    pred = rs.randint(0, 4, size=(R, C)).astype(np.float32)              # many ties: arg-max takes the lowest index, as torch / numpy
    lab = rs.randint(0, C, size=R)
    cm = K.confusion(torch.from_numpy(pred).to(dev), torch.from_numpy(lab).to(dev), C)
    K.confusion(torch.from_numpy(pred[:5000]).to(dev), torch.from_numpy(lab[:5000]).to(dev), C, out=cm)      # accumulates
    cm = cm.cpu().numpy()
    am = np.concatenate([pred.argmax(1), pred[:5000].argmax(1)])
    ll = np.concatenate([lab, lab[:5000]])
    ref = np.zeros((C, C), np.int64)
    np.add.at(ref, (ll, am), 1)
    np.testing.assert_array_equal(cm, ref)
    # main.py:243-300 restated on the label / prediction arrays
    m = seg_metrics(cm)
    seen = np.array([np.sum(ll == l) for l in range(C)], dtype=np.float64)
    corr = np.array([np.sum((am == l) & (ll == l)) for l in range(C)], dtype=np.float64)
    deno = np.array([np.sum((am == l) | (ll == l)) for l in range(C)], dtype=np.float64)
    assert m["miou"] == np.mean(corr / (deno + 1e-6))
    assert m["macc"] == np.mean(corr / (seen + 1e-6))
    assert m["oa"] == np.sum(am == ll) / float(ll.size)


# ---- whole model against the reference module (g18) -----------------------------------------------------------------------
def _g18_model(dev):
    from act_amd.models.semseg import get_model
    m = fill_module(get_model(13), "g18.").to(dev)
    m.dp1.p = 0.0
    for b in m.blocks.blocks:
        b.drop_prob = 0.0
    return m


def _run_g18(dev, pergroup):
    from act_amd.models.semseg import get_loss
    g = golden("g18_semseg")
    model = _g18_model(dev)
    pts = torch.from_numpy(g["pts"]).to(dev).transpose(1, 2)
    target = torch.from_numpy(g["labels"]).to(dev).reshape(-1)
    weight = torch.from_numpy(g["weight"]).to(dev)
    model.train()
    logp = model(pts, pergroup=pergroup)
    loss = get_loss()(logp, target, weight)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    model.eval()
    with torch.no_grad():
        logp_eval = model(pts, pergroup=pergroup)
    return g, logp.detach(), loss.detach(), grads, logp_eval


@pytest.mark.parametrize("pergroup", [True, False])
def test_model_vs_reference_golden(dev, pergroup):
    g, logp, loss, grads, logp_eval = _run_g18(dev, pergroup)
    # (b): the reference module with the difference-form square_distance (the project's convention): the 1e-4 bars
    assert np.abs(logp.cpu().numpy() - g["b_logp_train"]).max() <= 1e-4
    assert np.abs(logp_eval.cpu().numpy() - g["b_logp_eval"]).max() <= 1e-4
    assert abs(loss.item() - float(g["b_loss"])) <= 1e-4
    # gradient norms: the bar the project holds every fp32-reference golden's gradient norms to (test_gpu_finetune.py), rtol 2e-3 / atol 2e-5.
    # Measured: at most 2.1e-4 relative (blocks.0.mlp.fc2.weight, the end of the 12-block backward chain); a 1e-4 bar on the norms is not met.
    ref = dict(zip(g["b_grad_names"], g["b_grad_norms"]))
    assert set(ref) == set(grads)
    names = sorted(grads)
    np.testing.assert_allclose([grads[n].norm().item() for n in names], [ref[n] for n in names], rtol=2e-3, atol=2e-5)
    # (a): the unmodified module.  Its expansion-form distances (|p|^2 + |c|^2 - 2 p.c) give every centre's own point a distance of
    # +-1e-7..1e-6 instead of 0, so that point's weight 1/(d + 1e-8) is not ~1e8 and the interpolated feature is not the centre's own:
    # the two reference forms differ by ~8e-5 in the train-mode log-probs (BatchNorm batch statistics carry it to every row).  Bar: 1e-3.
    assert np.abs(logp.cpu().numpy() - g["a_logp_train"]).max() <= 1e-3
    assert np.abs(logp_eval.cpu().numpy() - g["a_logp_eval"]).max() <= 1e-3
    assert abs(loss.item() - float(g["a_loss"])) <= 1e-3


def test_pergroup_vs_plain_form(dev):
    _, lp1, loss1, gr1, ev1 = _run_g18(dev, True)
    _, lp2, loss2, gr2, ev2 = _run_g18(dev, False)
    # the two forms sum in different orders (W_f . sum_k w_k x_k against sum_k w_k (W_f . x)_k); train-mode BatchNorm over 1,024 rows carries the
    # fp32 rounding to every row.  Measured 2.8e-5 on the train-mode log-probs; the bar is the 1e-4 each form meets against the reference.
    assert (lp1 - lp2).abs().max().item() <= 1e-4
    assert (ev1 - ev2).abs().max().item() <= 1e-4
    assert abs(loss1.item() - loss2.item()) <= 1e-4
    # gradients: element-wise 1e-4 of max(1, |max|) where the two forms make the same discrete selections.  They do not everywhere: the ReLU
    # masks after the propagation convs and bns1_cls flip for activations within rounding of 0 (measured: 152 of 1,703,936 elements of
    # convs1_cls.weight beyond 1e-4), so the flip-tolerant rule applies, naming that selection.
    for n in gr1:
        _grad_close(gr1[n], gr2[n], n)


# ---- full geometry against a float64 CPU restatement ------------------------------------------------------------------------
class _RefSemSeg(nn.Module):
    """semantic_segmentation/models/pt.py restated on CPU with the oracle's layers; grouping and three-NN selections are made on the float32
    cloud in the difference form (the project's convention), everything after them in the module's dtype; draws replayed"""

    def __init__(self):
        super().__init__()
        from oracle import layers as OL
        from act_amd.models.semseg import PointNetFeaturePropagation
        self.encoder = OL.Encoder(384)
        self.pos_embed = nn.Sequential(nn.Linear(3, 128), nn.GELU(), nn.Linear(128, 384))
        self.blocks = OL.TransformerEncoder(384, 12, 6, [x.item() for x in torch.linspace(0, 0.1, 12)], tag="enc")
        self.norm = nn.LayerNorm(384)
        self.propagation_0_cls = PointNetFeaturePropagation(1155, [1536, 1024])         # parameters only (forward restated below)
        self.convs1_cls = nn.Conv1d(3328, 512, 1)
        self.convs2_cls = nn.Conv1d(512, 256, 1)
        self.convs3_cls = nn.Conv1d(256, 13, 1)
        self.bns1_cls = nn.BatchNorm1d(512)
        self.bns2_cls = nn.BatchNorm1d(256)

    def forward(self, xyz32, draws):
        from oracle import point_ops as OP
        B, N, _ = xyz32.shape
        nb, center, _, _ = OP.group_ref(xyz32, 128, 32)
        dt = self.norm.weight.dtype
        nb, center = torch.from_numpy(nb).to(dt), torch.from_numpy(center)
        x = self.encoder(nb)
        pos = self.pos_embed(center.to(dt))
        feats = []
        for i, blk in enumerate(self.blocks.blocks):
            x = blk(x + pos, draws)
            if i in (3, 7, 11):
                feats.append(self.norm(x))
        x = torch.cat(feats, dim=-1)                                    # B G 1152
        glob = torch.cat((x.max(1)[0], x.mean(1)), dim=-1)              # B 2304
        c32 = center
        x32 = torch.from_numpy(xyz32)
        dd = x32[:, :, None, :] - c32[:, None, :, :]
        d = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]
        d, idx = torch.sort(d, dim=-1, stable=True)
        d, idx = d[:, :, :3].to(dt), idx[:, :, :3]
        r = 1.0 / (d + 1e-8)
        wgt = r / r.sum(-1, keepdim=True)
        interp = (torch.stack([x[b][idx[b]] for b in range(B)]) * wgt.unsqueeze(-1)).sum(2)      # B N 1152
        h = torch.cat((x32.to(dt), interp), dim=-1).transpose(1, 2)     # B 1155 N
        fp = self.propagation_0_cls
        for conv, bn in zip(fp.mlp_convs, fp.mlp_bns):
            h = F.relu(bn(conv(h)))
        h = torch.cat((h, glob.unsqueeze(-1).expand(-1, -1, N)), dim=1)
        h = F.relu(self.bns1_cls(self.convs1_cls(h)))
        keep = draws.get("head.drop1", None)                            # [B*N, 512] rows of the HIP path
        h = h * (keep.to(dt).reshape(B, N, 512).transpose(1, 2) / 0.5)
        h = F.relu(self.bns2_cls(self.convs2_cls(h)))
        return F.log_softmax(self.convs3_cls(h), dim=1).permute(0, 2, 1)


def _grad_close(a, ref, name, tol=1e-4, frac=1e-3):
    """the project's gradient rule (test_gpu_model.py::_grad_close): element-wise tol of max(1, max |ref|); where that fails, at most a ``frac``
    fraction of the elements (flipped discrete selections) may exceed it and the gradient must agree to 5e-3 in the L2 sense"""
    a = torch.as_tensor(a).detach().double().cpu(); ref = torch.as_tensor(ref).detach().double().cpu()
    assert a.shape == ref.shape, (name, a.shape, ref.shape)
    scale = max(1.0, ref.abs().max().item())
    err = (a - ref).abs()
    if err.max().item() <= tol * scale:
        return
    flipped = int((err > tol * scale).sum())
    l2 = (err.norm() / ref.norm().clamp_min(1e-30)).item()
    assert flipped <= frac * err.numel() and l2 <= 5e-3, (name, "flipped elements", flipped, "of", err.numel(), "l2", l2)


def test_full_geometry_vs_cpu_restatement_with_draws(dev):
    """B = 8, N = 2048, G = 128, DropPath 0.1 and Dropout 0.5 with the HIP path's draws replayed.  The gradient bar is the flip-tolerant rule:
    FPS, kNN and three-NN make the same selections on both sides by construction (float32 cloud, difference form), but the max-pool arg-maxes
    (the two mini-PointNet pools and the global x_max) may pick another row where two fp32 values are within rounding of each other."""
    from act_amd.models.semseg import get_model, get_loss
    from act_amd.utils.draws import Draws
    from tests.golden.fill import clouds
    B, N = 8, 2048
    xyz = clouds(181, B, N)
    xyz[:, :, 2] += 1.5
    rs = np.random.RandomState(181)
    target = torch.from_numpy(rs.randint(0, 13, size=B * N))
    weight = torch.from_numpy((1 + rs.rand(13)).astype(np.float32))
    model = fill_module(get_model(13), "g18f.").to(dev).train()
    torch.manual_seed(181)                                              # the DropPath / Dropout draws: one fixed instance, replayed on the CPU
    draws = Draws(record=True)
    logp = model(torch.from_numpy(xyz).to(dev).transpose(1, 2), draws=draws)
    loss = get_loss()(logp, target.to(dev), weight.to(dev))
    loss.backward()
    ref = _RefSemSeg()
    missing, unexpected = ref.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()}, strict=False)
    assert not [k for k in missing if "num_batches" not in k], missing
    ref = ref.double().train()
    for bn in [m for m in ref.modules() if isinstance(m, nn.BatchNorm1d)]:
        bn.running_mean.zero_(); bn.running_var.fill_(1.0)
    from oracle.layers import Draws as ODraws
    rdraws = ODraws({k: v.cpu().double() for k, v in draws.table.items()})
    rlogp = ref(xyz, rdraws)
    rloss = F.nll_loss(rlogp.reshape(-1, 13), target, weight.double())
    rloss.backward()
    assert (logp.detach().cpu().double() - rlogp.detach()).abs().max().item() <= 1e-4
    assert abs(loss.item() - rloss.item()) <= 1e-4
    rp = dict(ref.named_parameters())
    for n, p in model.named_parameters():
        _grad_close(p.grad, rp[n].grad, n)


# ---- checkpoints -------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_act_pretrain_loading(dev, tmp_path):
    from act_amd.models.semseg import get_model
    from act_amd.models.act import VisableOnlyMaskTransformer
    from act_amd.utils.config import EasyDict
    m1 = fill_module(get_model(13), "ck1.").to(dev)
    opt = torch.optim.AdamW(m1.parameters(), lr=1e-3)
    path = tmp_path / "best_model.pth"
    torch.save({"epoch": 3, "class_avg_iou": 0.5, "model_state_dict": m1.state_dict(), "optimizer_state_dict": opt.state_dict()}, path)
    m2 = get_model(13).to(dev)
    inc = m2.load_model_from_ckpt_withrename(str(path))
    assert not inc.missing_keys and not inc.unexpected_keys
    for k, v in m1.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k
    # an ACT pretraining checkpoint: {'base_model': ACT_PointDistillation.state_dict()} -- the student lives under ACT_encoder.
    cfg = EasyDict(dict(transformer_config=dict(mask_ratio=0.8, mask_type="rand", embed_dim=384, depth=12, drop_path_rate=0.1, cls_dim=512,
                                                num_heads=6),
                        dvae_config=dict(encoder_dims=384, num_tokens=64)))
    enc = fill_module(VisableOnlyMaskTransformer(cfg), "ck2.")
    sd = {"module.ACT_encoder." + k: v for k, v in enc.state_dict().items()}
    sd["module.ACT_decoder.norm.weight"] = torch.ones(384)
    ppath = tmp_path / "ckpt-last.pth"
    torch.save({"base_model": sd}, ppath)
    m3 = get_model(13)
    inc = m3.load_model_from_ckpt(str(ppath))
    esd = enc.state_dict()
    loaded = [k for k in m3.state_dict() if k in esd]
    assert any(k.startswith("blocks.blocks.11.") for k in loaded) and "encoder.second_conv.3.weight" in loaded and "norm.weight" in loaded
    for k in loaded:
        assert torch.equal(m3.state_dict()[k], esd[k]), k
    assert all(k.startswith(("propagation_0_cls", "convs", "bns")) for k in inc.missing_keys)


# ---- short synthetic training run --------------------------------------------------------------------------------------------
def test_runner_synthetic_learns(tmp_path):
    from act_amd.datasets.S3DISDataset import SyntheticS3DIS
    cmd = [sys.executable, "-m", "act_amd.tools.runner_semseg", "--synthetic", "--max_steps", "150", "--batch_size", "8",
           "--warmup_epoch", "0", "--learning_rate", "0.0005", "--log_every", "25", "--eval_batches", "12", "--num_workers", "2",
           "--log_dir", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    losses = [float(x) for x in re.findall(r"step \d+: loss ([0-9.]+)", r.stdout)]
    best = float(re.search(r"best mIoU ([0-9.]+)", r.stdout).group(1)) / 100
    # a constant-class predictor's mIoU on the held-out rooms: (share of its class) / 13 at best
    te = SyntheticS3DIS("test", 2048, seed=0)
    share = np.bincount(np.concatenate(te.room_labels).astype(np.int64), minlength=13) / sum(l.size for l in te.room_labels)
    const = share.max() / 13
    assert losses[-1] < losses[0]
    assert best > 4 * const, (best, const)
    assert os.path.exists(tmp_path / "checkpoints" / "best_model.pth")
    ck = torch.load(tmp_path / "checkpoints" / "best_model.pth", map_location="cpu")
    assert set(ck) == {"epoch", "class_avg_iou", "model_state_dict", "optimizer_state_dict"}
