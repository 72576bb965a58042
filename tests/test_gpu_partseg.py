"""GPU: ShapeNetPart part segmentation (act_amd/models/partseg.py, csrc/partseg.hip) -- the category label branch and the category-masked
evaluation kernel against independent transcriptions, the whole model against the reference's own module (g19) and against a float64 CPU
restatement at full geometry, checkpoints across the two segmentation models, and a short synthetic training run."""
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
from tests.test_gpu_semseg import _RefSemSeg, _grad_close
from tests.test_partseg_host import SEG_CLASSES, reference_metrics, counts_from_arrays

pytestmark = pytest.mark.gpu

CATS = sorted(SEG_CLASSES)
FIRST = np.cumsum([0] + [len(SEG_CLASSES[c]) for c in CATS])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- (a) label branch --------------------------------------------------------------------------------------------------------
def _label_modules(seed):
    torch.manual_seed(seed)
    ref = nn.Sequential(nn.Conv1d(16, 64, 1, bias=False), nn.BatchNorm1d(64), nn.LeakyReLU(0.2))
    with torch.no_grad():
        ref[0].weight.normal_(0, 0.5)
        ref[1].weight.uniform_(0.5, 1.5)
        ref[1].bias.normal_(0, 0.3)
        ref[1].running_mean.normal_(0, 0.2)
        ref[1].running_var.uniform_(0.5, 2.0)
    return ref


@pytest.mark.parametrize("onehot", [True, False])
def test_label_branch_vs_float64(dev, onehot):
    from act_amd import kernels as K
    B = 16
    rs = np.random.RandomState(5)
    c = np.eye(16, dtype=np.float32)[rs.randint(0, 16, size=B)] if onehot else rs.standard_normal((B, 16)).astype(np.float32)
    dy = rs.standard_normal((B, 64)).astype(np.float32)
    ref = _label_modules(3)
    ours = _label_modules(3).to(dev)
    r64 = ref.double().train()
    y64 = r64(torch.from_numpy(c).double().unsqueeze(-1)).squeeze(-1)
    y64.backward(torch.from_numpy(dy).double())
    outs = []
    for run in range(2):
        m = _label_modules(3).to(dev).train()
        for p in m.parameters():
            p.grad = None
        y = K.label_branch(torch.from_numpy(c).to(dev), m[0], m[1], m[2], True)
        y.backward(torch.from_numpy(dy).to(dev))
        outs.append((y.detach().clone(), m[0].weight.grad.clone(), m[1].weight.grad.clone(), m[1].bias.grad.clone(),
                     m[1].running_mean.clone(), m[1].running_var.clone()))
    y, dW, dg, db, rm, rv = outs[0]
    assert (y.cpu().double() - y64.detach()).abs().max().item() <= 1e-5
    # dW reaches |dW| = 11 here (fp32 ulp 9.5e-7): the 1e-6 bar needs the kernel's float64 accumulation (one rounding per element)
    rdW = r64[0].weight.grad.view(64, 16)
    print("label branch dW: max |dW|", rdW.abs().max().item(), "max error", (dW.view(64, 16).cpu().double() - rdW).abs().max().item())
    assert (dW.view(64, 16).cpu().double() - rdW).abs().max().item() <= 1e-6
    assert (dg.cpu().double() - r64[1].weight.grad).abs().max().item() <= 1e-5
    assert (db.cpu().double() - r64[1].bias.grad).abs().max().item() <= 1e-5
    assert (rm.cpu().double() - r64[1].running_mean).abs().max().item() <= 1e-5          # momentum update, unbiased variance (count B)
    assert (rv.cpu().double() - r64[1].running_var).abs().max().item() <= 1e-5
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)                                         # fixed-order reductions: bit-identical run to run
    # eval mode: running statistics
    ours.eval()
    r64.eval()
    with torch.no_grad():
        ye = K.label_branch(torch.from_numpy(c).to(dev), ours[0], ours[1], ours[2], False)
        ye64 = _label_modules(3).double().eval()(torch.from_numpy(c).double().unsqueeze(-1)).squeeze(-1)
    assert (ye.cpu().double() - ye64).abs().max().item() <= 1e-5
    # B = 1 in train mode is an error, as in torch
    with pytest.raises(ValueError):
        K.label_branch(torch.from_numpy(c[:1]).to(dev), ours[0], ours[1], ours[2], True)


# ---- (b) category-masked evaluation kernel ---------------------------------------------------------------------------------------
def _masked_argmax(logp, target):
    """main.py:259-263: np.argmax over the category's part range of every shape (ties: first index)"""
    out = np.zeros(target.shape, np.int64)
    for i in range(target.shape[0]):
        c = [k for k in CATS if target[i, 0] in SEG_CLASSES[k]][0]
        out[i] = np.argmax(logp[i][:, SEG_CLASSES[c]], 1) + SEG_CLASSES[c][0]
    return out


def _eval_case(rs, cats, N):
    S = len(cats)
    logp = rs.standard_normal((S, N, 50)).astype(np.float32) - 4
    target = np.zeros((S, N), np.int64)
    for i, c in enumerate(cats):
        lo, hi = FIRST[c], FIRST[c + 1]
        target[i] = rs.randint(lo, hi, size=N)
        out = np.setdiff1d(np.arange(50), np.arange(lo, hi))
        big = rs.rand(N) < 0.3                                           # larger values outside the range: the masked arg-max ignores them
        logp[i][np.ix_(big, out)] = 5.0 + rs.rand(big.sum(), out.size).astype(np.float32)
        tie = rs.rand(N) < 0.2                                           # planted ties inside the range: the first index wins
        if hi - lo >= 2:
            logp[i, tie, lo + 1] = 2.0
            logp[i, tie, hi - 1] = 2.0
            logp[i, tie, lo] = 1.0
        good = rs.rand(N) < 0.5                                          # some right answers
        logp[i, good, target[i, good]] = 3.0
    # one shape with a part absent from both target and prediction (IoU 1.0): the first Motorbike shape uses parts 30, 31 only
    mi = [i for i, c in enumerate(cats) if CATS[c] == "Motorbike"][0]
    target[mi] = rs.randint(30, 32, size=N)
    logp[mi, :, 32:36] = -50.0
    return logp, target


def test_part_eval_kernel_vs_transcription(dev):
    from act_amd import kernels as K
    from act_amd.tools.runner_partseg import part_metrics
    rs = np.random.RandomState(8)
    N = 2048
    cats = list(range(16)) + [10, 3, 0, 15]                              # all 16 categories; batches of 13 and 7 (nothing convenient)
    logp, target = _eval_case(rs, cats, N)
    S = len(cats)
    counts = torch.full((S + 3, K.PART_COUNT_STRIDE), -7, dtype=torch.int32, device=dev)
    seen = torch.zeros(50, dtype=torch.int64, device=dev)
    correct = torch.zeros(50, dtype=torch.int64, device=dev)
    preds = []
    for s0, s1 in ((0, 13), (13, S)):
        pred = torch.empty((s1 - s0) * N, dtype=torch.int32, device=dev)
        K.partseg_eval(torch.from_numpy(logp[s0:s1]).to(dev), torch.from_numpy(target[s0:s1]).to(dev), counts, seen, correct, s0, pred=pred)
        preds.append(pred.cpu().numpy().reshape(s1 - s0, N))
    pred = np.concatenate(preds)
    ref_pred = _masked_argmax(logp, target)
    np.testing.assert_array_equal(pred, ref_pred)
    rc, rseen, rcorr = counts_from_arrays(ref_pred, target)
    c = counts.cpu().numpy()
    np.testing.assert_array_equal(c[:S], rc)
    assert (c[S:] == -7).all()                                           # rows past the written shapes untouched
    np.testing.assert_array_equal(seen.cpu().numpy(), rseen)
    np.testing.assert_array_equal(correct.cpu().numpy(), rcorr)
    m = part_metrics(c[:S], seen.cpu().numpy(), correct.cpu().numpy())
    r = reference_metrics(ref_pred, target)
    for k in ("accuracy", "class_avg_accuracy", "class_avg_iou", "inctance_avg_iou"):
        assert abs(m[k] - r[k]) <= 1e-12, (k, m[k], r[k])
    assert len(m["per_category"]) == 16
    # the scalar-load path (N * 50 not a multiple of 4) and the counts without a prediction buffer
    N2 = 1001
    logp2, target2 = _eval_case(np.random.RandomState(9), [10, 2, 5], N2)
    counts2 = torch.zeros(3, K.PART_COUNT_STRIDE, dtype=torch.int32, device=dev)
    seen2 = torch.zeros(50, dtype=torch.int64, device=dev)
    corr2 = torch.zeros(50, dtype=torch.int64, device=dev)
    K.partseg_eval(torch.from_numpy(logp2).to(dev), torch.from_numpy(target2).to(dev), counts2, seen2, corr2, 0)
    rc2, rs2, rr2 = counts_from_arrays(_masked_argmax(logp2, target2), target2)
    np.testing.assert_array_equal(counts2.cpu().numpy(), rc2)
    np.testing.assert_array_equal(seen2.cpu().numpy(), rs2)
    np.testing.assert_array_equal(corr2.cpu().numpy(), rr2)
    # the widest rows the kernel takes (P = 64: a smaller LDS tile of 200 rows) on a table of 11 categories
    sizes = [6] * 10 + [4]
    first = np.cumsum([0] + sizes)
    table = {f"c{j:02d}": list(range(first[j], first[j + 1])) for j in range(11)}
    rs3 = np.random.RandomState(10)
    S3, N3 = 5, 1000
    cat3 = np.array([0, 10, 4, 7, 10])
    logp3 = rs3.standard_normal((S3, N3, 64)).astype(np.float32)
    logp3[:, :, ::7] = 0.5                                               # ties
    target3 = np.stack([rs3.randint(first[c], first[c + 1], size=N3) for c in cat3])
    pred3 = torch.empty(S3 * N3, dtype=torch.int32, device=dev)
    K.partseg_eval(torch.from_numpy(logp3).to(dev), torch.from_numpy(target3).to(dev), torch.zeros(S3, K.PART_COUNT_STRIDE, dtype=torch.int32,
                   device=dev), torch.zeros(64, dtype=torch.int64, device=dev), torch.zeros(64, dtype=torch.int64, device=dev), 0, pred=pred3,
                   tables=K.part_tables(table, num_part=64, device=dev))
    ref3 = np.stack([np.argmax(logp3[i][:, first[c]:first[c + 1]], 1) + first[c] for i, c in enumerate(cat3)])
    np.testing.assert_array_equal(pred3.cpu().numpy().reshape(S3, N3), ref3)


# ---- (c) whole model against the reference module (g19) -----------------------------------------------------------------------
def _run_g19(dev, pergroup):
    from act_amd.models.partseg import get_model, get_loss, to_categorical
    g = golden("g19_partseg")
    model = fill_module(get_model(50), "g19.").to(dev)
    model.dp1.p = 0.0
    for b in model.blocks.blocks:
        b.drop_prob = 0.0
    pts = torch.from_numpy(g["pts"]).to(dev).transpose(1, 2)
    cls = to_categorical(torch.from_numpy(g["cls"]).to(dev).view(-1, 1), 16)
    target = torch.from_numpy(g["labels"]).to(dev).reshape(-1)
    model.train()
    logp = model(pts, cls, pergroup=pergroup)
    loss = get_loss()(logp, target)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    model.eval()
    with torch.no_grad():
        logp_eval = model(pts, cls, pergroup=pergroup)
    return g, model, logp.detach(), loss.detach(), grads, logp_eval


@pytest.mark.parametrize("pergroup", [True, False])
def test_model_vs_reference_golden(dev, pergroup):
    g, model, logp, loss, grads, logp_eval = _run_g19(dev, pergroup)
    K64 = g["a_logp_train"].shape[1]
    assert list(model.state_dict().keys()) == list(g["sd_keys"])
    # (b): the reference module with the difference-form square_distance (the project's convention): the 1e-4 bars
    assert np.abs(logp.cpu().numpy() - g["b_logp_train"]).max() <= 1e-4
    assert np.abs(logp_eval[:, :K64].cpu().numpy() - g["b_logp_eval"]).max() <= 1e-4
    assert abs(loss.item() - float(g["b_loss"])) <= 1e-4
    ref = dict(zip(g["b_grad_names"], g["b_grad_norms"]))
    assert set(ref) == set(grads)
    names = sorted(grads)
    np.testing.assert_allclose([grads[n].norm().item() for n in names], [ref[n] for n in names], rtol=2e-3, atol=2e-5)
    assert grads["label_conv_cls.0.weight"].norm().item() > 1e-6          # B = 4, three categories: the label branch's gradient is alive
    # (a): the unmodified module (expansion-form distances; see test_gpu_semseg.py): 1e-3
    assert np.abs(logp[:, :K64].cpu().numpy() - g["a_logp_train"]).max() <= 1e-3
    assert np.abs(logp_eval[:, :K64].cpu().numpy() - g["a_logp_eval"]).max() <= 1e-3
    assert abs(loss.item() - float(g["a_loss"])) <= 1e-3


# ---- (d) full geometry against a float64 CPU restatement ------------------------------------------------------------------------
class _RefPartSeg(_RefSemSeg):
    """part_segmentation/models/pt.py on the semantic-segmentation restatement: the label branch in float64 (BatchNorm over the B clouds), its
    64 per-cloud columns appended to the input of convs1_cls (cat(f_level_0, max, mean, label)), 50 parts"""

    def __init__(self):
        super().__init__()
        self.label_conv_cls = nn.Sequential(nn.Conv1d(16, 64, 1, bias=False), nn.BatchNorm1d(64), nn.LeakyReLU(0.2))
        self.convs1_cls = nn.Conv1d(3392, 512, 1)
        self.convs3_cls = nn.Conv1d(256, 50, 1)
        self.convs1_cls.register_forward_pre_hook(
            lambda m, args: (torch.cat((args[0], self._lab.unsqueeze(-1).expand(-1, -1, args[0].shape[-1])), dim=1),))

    def forward(self, xyz32, cls, draws):
        self._lab = self.label_conv_cls(cls.to(self.norm.weight.dtype).unsqueeze(-1)).squeeze(-1)
        return super().forward(xyz32, draws)


def test_full_geometry_vs_cpu_restatement_with_draws(dev):
    """B = 8, N = 2048, G = 128, DropPath 0.1 and Dropout 0.5 with the HIP path's draws replayed; the flip-tolerant gradient rule (max-pool
    arg-maxes may pick another row where two fp32 values are within rounding of each other)"""
    from act_amd.models.partseg import get_model, get_loss, to_categorical
    from act_amd.utils.draws import Draws
    from tests.golden.fill import clouds
    B, N = 8, 2048
    xyz = clouds(191, B, N)
    rs = np.random.RandomState(191)
    cat = np.array([0, 4, 10, 15, 4, 7, 12, 1])
    target = torch.from_numpy(np.concatenate([rs.randint(FIRST[c], FIRST[c + 1], size=N) for c in cat]))
    cls = to_categorical(torch.from_numpy(cat), 16)
    model = fill_module(get_model(50), "g19f.").to(dev).train()
    torch.manual_seed(191)
    draws = Draws(record=True)
    logp = model(torch.from_numpy(xyz).to(dev).transpose(1, 2), cls.to(dev), draws=draws)
    loss = get_loss()(logp, target.to(dev))
    loss.backward()
    ref = _RefPartSeg()
    missing, unexpected = ref.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()}, strict=False)
    assert not [k for k in missing if "num_batches" not in k], missing
    ref = ref.double().train()
    for bn in [m for m in ref.modules() if isinstance(m, nn.BatchNorm1d)]:
        bn.running_mean.zero_(); bn.running_var.fill_(1.0)
    from oracle.layers import Draws as ODraws
    rdraws = ODraws({k: v.cpu().double() for k, v in draws.table.items()})
    rlogp = ref(xyz, cls, rdraws)
    rloss = F.nll_loss(rlogp.reshape(-1, 50), target)
    rloss.backward()
    assert (logp.detach().cpu().double() - rlogp.detach()).abs().max().item() <= 1e-4
    assert abs(loss.item() - rloss.item()) <= 1e-4
    rp = dict(ref.named_parameters())
    for n, p in model.named_parameters():
        _grad_close(p.grad, rp[n].grad, n)


# ---- (e) checkpoints ----------------------------------------------------------------------------------------------------------
def test_checkpoints_round_trip_pretrain_and_cross_task(dev, tmp_path):
    from act_amd.models.partseg import get_model
    from act_amd.models import semseg
    from act_amd.models.act import VisableOnlyMaskTransformer
    from act_amd.utils.config import EasyDict
    m1 = fill_module(get_model(50), "ck1.").to(dev)
    opt = torch.optim.AdamW(m1.parameters(), lr=1e-3)
    path = tmp_path / "best_model.pth"
    torch.save({"epoch": 3, "train_acc": 0.5, "test_acc": 0.6, "class_avg_iou": 0.5, "inctance_avg_iou": 0.55, "model_state_dict": m1.state_dict(),
                "optimizer_state_dict": opt.state_dict()}, path)
    m2 = get_model(50).to(dev)
    inc = m2.load_model_from_ckpt_withrename(str(path))
    assert not inc.missing_keys and not inc.unexpected_keys
    for k, v in m1.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k
    # an ACT pretraining checkpoint loads the encoder; only head keys are missing
    cfg = EasyDict(dict(transformer_config=dict(mask_ratio=0.8, mask_type="rand", embed_dim=384, depth=12, drop_path_rate=0.1, cls_dim=512,
                                                num_heads=6),
                        dvae_config=dict(encoder_dims=384, num_tokens=64)))
    enc = fill_module(VisableOnlyMaskTransformer(cfg), "ck2.")
    sd = {"module.ACT_encoder." + k: v for k, v in enc.state_dict().items()}
    ppath = tmp_path / "ckpt-last.pth"
    torch.save({"base_model": sd}, ppath)
    m3 = get_model(50)
    inc = m3.load_model_from_ckpt(str(ppath))
    esd = enc.state_dict()
    loaded = [k for k in m3.state_dict() if k in esd]
    assert any(k.startswith("blocks.blocks.11.") for k in loaded) and "encoder.second_conv.3.weight" in loaded and "norm.weight" in loaded
    for k in loaded:
        assert torch.equal(m3.state_dict()[k], esd[k]), k
    assert inc.missing_keys and all(k.startswith(("label_conv_cls", "propagation_0_cls", "convs", "bns")) for k in inc.missing_keys)
    # semseg -> partseg and back through _withrename: the shape-mismatched heads are reported and keep their values
    s1 = fill_module(semseg.get_model(13), "ck3.")
    spath = tmp_path / "semseg_best.pth"
    torch.save({"epoch": 1, "class_avg_iou": 0.3, "model_state_dict": s1.state_dict()}, spath)
    p = get_model(50)
    before = {k: v.clone() for k, v in p.state_dict().items()}
    inc = p.load_model_from_ckpt_withrename(str(spath))
    assert set(inc.missing_keys) == {"convs1_cls.weight", "convs3_cls.weight", "convs3_cls.bias"} and not inc.unexpected_keys
    for k, v in p.state_dict().items():
        src = s1.state_dict().get(k)
        if k in inc.missing_keys or k.startswith("label_conv_cls"):
            assert torch.equal(v, before[k]), k
        else:
            assert torch.equal(v, src), k
    s2 = semseg.get_model(13)
    inc = s2.load_model_from_ckpt_withrename(str(path))
    assert set(inc.missing_keys) == {"convs1_cls.weight", "convs3_cls.weight", "convs3_cls.bias"} and not inc.unexpected_keys
    assert torch.equal(s2.state_dict()["blocks.blocks.5.mlp.fc1.weight"], m1.state_dict()["blocks.blocks.5.mlp.fc1.weight"].cpu())


# ---- (f) short synthetic training run -------------------------------------------------------------------------------------------
def test_runner_synthetic_learns(tmp_path):
    from act_amd.datasets.ShapeNetPartDataset import SyntheticShapeNetPart
    from act_amd.tools.runner_partseg import part_metrics
    cmd = [sys.executable, "-m", "act_amd.tools.runner_partseg", "--synthetic", "--max_steps", "150", "--batch_size", "8",
           "--warmup_epoch", "0", "--learning_rate", "0.0005", "--log_every", "25", "--eval_batches", "8", "--num_workers", "2",
           "--log_dir", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    losses = [float(x) for x in re.findall(r"step \d+: loss ([0-9.]+)", r.stdout)]
    best = float(re.search(r"best instance mIoU ([0-9.]+)", r.stdout).group(1)) / 100
    # the best constant-per-category predictor on the held-out shapes: each category's most frequent part
    te = SyntheticShapeNetPart("test", 2048, seed=0)
    tgt = np.stack(te.seg).astype(np.int64)
    pred = np.zeros_like(tgt)
    for c in CATS:
        rows = [i for i in range(len(tgt)) if tgt[i, 0] in SEG_CLASSES[c]]
        vals, cnt = np.unique(tgt[rows], return_counts=True)
        pred[rows] = vals[np.argmax(cnt)]
    const = part_metrics(*counts_from_arrays(pred, tgt))["inctance_avg_iou"]
    print("constant-per-category instance mIoU", const, "trained", best)
    assert losses[-1] < losses[0]
    assert best > 1.5 * const, (best, const)
    ck = torch.load(tmp_path / "checkpoints" / "best_model.pth", map_location="cpu")
    assert set(ck) == {"epoch", "train_acc", "test_acc", "class_avg_iou", "inctance_avg_iou", "model_state_dict", "optimizer_state_dict"}
