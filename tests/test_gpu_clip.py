"""GPU: the CLIP image teacher (csrc/clip.hip, K.ClipBlockFn, ``visual_embed_type: clip:ViT-B/16`` of ACTPromptedDiscreteVAEwithVIT) against float64 numpy,
tests/clip_ref.py and the reference's own arrays in tests/golden/g23_clip.npz.  The GPU machine has neither the reference nor ``clip``."""
import copy
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_module, clouds, TINY_N  # noqa: E402
import clip_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _rel(a, ref):
    a = torch.as_tensor(a).detach().double().cpu(); ref = torch.as_tensor(ref).detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return ((a - ref).abs().max() / max(1.0, ref.abs().max())).item()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def K():
    import act_amd.kernels as K
    return K


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "g23_clip.npz"))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- QuickGELU
PLANTED = np.array([0.0, -0.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4], dtype=np.float32)


def _qg64(x):
    """float64 numpy: (x s, s (1 + a x (1 - s))) with s and 1 - s from exp(-|a x|), exact for every finite x"""
    z = 1.702 * x.astype(np.float64)
    t = np.exp(-np.abs(z))
    big, small = 1.0 / (1.0 + t), t / (1.0 + t)
    s, c = np.where(z >= 0, big, small), np.where(z >= 0, small, big)
    return x * s, s * (1.0 + z * c)


def _inputs(rows, cols):
    """a normal draw scaled by 4 with the planted values at the front AND at the back (the vector body and the scalar tail); shapes too small for that get
    one tensor per chunk of planted values, so every planted value meets every shape"""
    rs = np.random.RandomState(rows * 131 + cols)
    n = rows * cols
    out = []
    if n >= 2 * len(PLANTED):
        x = (4.0 * rs.standard_normal(n)).astype(np.float32)
        x[:len(PLANTED)] = PLANTED
        x[-len(PLANTED):] = PLANTED[::-1]
        out.append(x)
    else:
        out.append((4.0 * rs.standard_normal(n)).astype(np.float32))
        for i in range(0, len(PLANTED), n):
            x = (4.0 * rs.standard_normal(n)).astype(np.float32)
            chunk = PLANTED[i:i + n]
            x[:len(chunk)] = chunk
            out.append(x)
    return [x.reshape(rows, cols) for x in out]


def _err(got, ref):
    """max over elements of |got - ref| / max(1, |ref|): the 1e-4 bar, absolute below 1 and relative above"""
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


@pytest.mark.parametrize("rows,cols", [(1, 4), (3, 260), (65, 1028), (1, 1)])
def test_quickgelu_against_float64(dev, K, rows, cols):
    worst = {"fwd": 0.0, "bwd": 0.0, "bwd_vs_central_differences": 0.0}
    for x in _inputs(rows, cols):
        dy = np.random.RandomState(7).standard_normal(x.shape).astype(np.float32)
        y_ref, g_ref = _qg64(x)
        xd = torch.from_numpy(x).to(dev).requires_grad_(True)
        y = K.quickgelu(xd)
        y.backward(torch.from_numpy(dy).to(dev))
        y, dx = y.detach().cpu().numpy(), xd.grad.cpu().numpy()
        assert np.isfinite(y).all() and np.isfinite(dx).all()
        assert (y[x == 0] == 0).all()
        worst["fwd"] = max(worst["fwd"], _err(y, y_ref))
        worst["bwd"] = max(worst["bwd"], _err(dx, dy * g_ref))
        # the backward is the forward's derivative: central differences of the float64 forward, on the numpy side
        x64 = x.astype(np.float64)
        h = 1e-6 * np.maximum(1.0, np.abs(x64))
        cd = (_qg64(x64 + h)[0] - _qg64(x64 - h)[0]) / (2 * h)
        assert _err(g_ref, cd) <= 1e-6                                     # the float64 formula itself
        worst["bwd_vs_central_differences"] = max(worst["bwd_vs_central_differences"], _err(dx, dy * cd))
    print(f"quickgelu [{rows}, {cols}]: {worst}")
    assert max(worst.values()) <= TOL, worst


def test_quickgelu_on_pointers_off_the_16_byte_grid(dev, K):
    """[3, 260] views that start 4 bytes past a 16-byte boundary: the head lanes + float4 body + tail when all pointers agree modulo 16, the scalar kernel
    when they do not; in place on dy; guard floats around the output stay untouched"""
    rows, cols = 3, 260
    n = rows * cols
    x = _inputs(rows, cols)[0]
    dy = np.random.RandomState(9).standard_normal(x.shape).astype(np.float32)
    y_ref, g_ref = _qg64(x)

    def off(a, k):
        buf = torch.full((n + 8,), 777.0, device=dev)
        buf[k:k + n] = torch.from_numpy(a).to(dev).reshape(-1)
        return buf, buf[k:k + n].view(rows, cols)
    for kx, ko in ((1, 1), (3, 3), (1, 2), (0, 3)):
        _, xv = off(x, kx)
        obuf, ov = off(np.zeros_like(x), ko)
        K.quickgelu_fwd(xv, out=ov)
        assert _err(ov.cpu().numpy(), y_ref) <= TOL, (kx, ko)
        assert (obuf[:ko] == 777.0).all() and (obuf[ko + n:] == 777.0).all(), (kx, ko)
        dbuf, dv = off(dy, ko)
        K.quickgelu_bwd(xv, dv, out=dv)                                   # in place
        assert _err(dv.cpu().numpy(), dy * g_ref) <= TOL, (kx, ko)
        assert (dbuf[:ko] == 777.0).all() and (dbuf[ko + n:] == 777.0).all(), (kx, ko)


# ---------------------------------------------------------------------------------------------- one block
def _block_sd(D, seed):
    g = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=g)        # noqa: E731
    return {"attn.in_proj_weight": r(3 * D, D) / D ** 0.5, "attn.in_proj_bias": 0.05 * r(3 * D), "attn.out_proj.weight": r(D, D) / D ** 0.5,
            "attn.out_proj.bias": 0.05 * r(D), "ln_1.weight": 1 + 0.1 * r(D), "ln_1.bias": 0.05 * r(D), "mlp.c_fc.weight": r(4 * D, D) / D ** 0.5,
            "mlp.c_fc.bias": 0.05 * r(4 * D), "mlp.c_proj.weight": r(D, 4 * D) / (4 * D) ** 0.5, "mlp.c_proj.bias": 0.05 * r(D),
            "ln_2.weight": 1 + 0.1 * r(D), "ln_2.bias": 0.05 * r(D)}


@pytest.mark.parametrize("S", [20, 128])
def test_block_at_head_dim_64_against_clip_ref(dev, K, S):
    B, D, H = 2, 128, 2
    sd = _block_sd(D, S)
    g = _gen(S + 1)
    x, pos, dy = (torch.randn(B, S, D, generator=g) for _ in range(3))
    xr, pr = x.clone().requires_grad_(True), pos.clone().requires_grad_(True)
    want = CR.clip_block(xr + pr, sd, "", H)
    want.backward(dy)
    w = {k: v.to(dev) for k, v in sd.items()}
    xd, pd = x.to(dev).requires_grad_(True), pos.to(dev).requires_grad_(True)
    args = (w["ln_1.weight"], w["ln_1.bias"], w["attn.in_proj_weight"], w["attn.in_proj_bias"], w["attn.out_proj.weight"], w["attn.out_proj.bias"],
            w["ln_2.weight"], w["ln_2.bias"], w["mlp.c_fc.weight"], w["mlp.c_fc.bias"], w["mlp.c_proj.weight"], w["mlp.c_proj.bias"], H)
    y = K.clip_block(xd, pd, *args)
    y.backward(dy.to(dev))
    errs = {"y": _rel(y, want), "dx": _rel(xd.grad, xr.grad), "dpos": _rel(pd.grad, pr.grad)}
    with torch.no_grad():
        assert torch.equal(K.clip_block(xd.detach(), pd.detach(), *args), y)       # the no_grad form (QuickGELU in place) computes the same bits
    print(errs)
    assert max(errs.values()) <= TOL, errs


# ---------------------------------------------------------------------------------------------- model
def _model(dev, cfg, prefix):
    from act_amd.models import build_model_from_cfg
    from act_amd.utils.config import EasyDict
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = build_model_from_cfg(EasyDict(cfg))
    return fill_module(model, prefix).to(dev)


def test_visual_embedding_matches_the_reference_golden(dev, golden):
    from act_amd.utils.draws import Draws
    model = _model(dev, CR.TINY_CLIP, "g23.")
    sampled, center = torch.from_numpy(golden["sampled"]).to(dev), torch.from_numpy(golden["center"]).to(dev)
    model.eval()
    with torch.no_grad():
        errs = {"ve_eval": _rel(model.visual_embedding(sampled, center), golden["ve_eval"])}
    model.train()
    model.zero_grad()
    x = sampled.clone().requires_grad_(True)
    ve = model.visual_embedding(x, center, Draws({"prompt.0": torch.from_numpy(golden["mask.prompt.0"])}, device=dev))
    errs["ve_train"] = _rel(ve, golden["ve_train"])
    (ve ** 2).sum().backward()
    pd = dict(model.named_parameters())
    errs["grad.sampled"] = _rel(x.grad, golden["grad.sampled"])
    for n in CR.GRAD_NAMES:
        assert pd[n].grad.shape == golden["grad." + n].shape
        errs["grad." + n] = float((pd[n].grad.double().cpu() - torch.from_numpy(golden["grad." + n]).double()).abs().max()
                                  / max(1.0, np.abs(golden["grad." + n]).max()))
    assert all(p.grad is None for n, p in pd.items() if n.startswith("visual_embed."))
    print(errs)
    assert max(errs.values()) <= TOL, errs


def test_promptless_variant_matches_the_golden_and_passes_no_gradient_upstream(dev, golden):
    model = _model(dev, dict(CR.TINY_CLIP, num_prompt_token=0), "g23.").train()
    x = torch.from_numpy(golden["sampled"]).to(dev).requires_grad_(True)
    ve = model.visual_embedding(x, torch.from_numpy(golden["center"]).to(dev))
    err = _rel(ve, golden["ve_noprompt"])
    (ve ** 2).sum().backward()
    errs = {"ve_noprompt": err, "grad.proj_post.bias": _rel(model.proj_post.bias.grad, golden["grad_noprompt.proj_post.bias"])}
    print(errs)
    assert bool(golden["noprompt_proj_pre_grad_is_none"]) and model.proj_pre.weight.grad is None and x.grad is None
    assert max(errs.values()) <= TOL, errs


# ---------------------------------------------------------------------------------------------- training steps
def test_stage1_train_step_is_deterministic_under_a_seed(dev):
    """train mode, no injected draws: the prompt keep mask and the gumbel noise come from Philox; the same seed gives the same loss bit for bit, another
    seed another one; the CLIP blocks stay frozen"""
    from act_amd.tools import builder
    from act_amd.tools.runner_pretrain import _Single
    from act_amd.tools import runner_autoencoder as RA
    from act_amd.utils.config import EasyDict
    cfg = EasyDict(dict(optimizer=dict(type="AdamW", kwargs=dict(lr=1e-3, weight_decay=0.05)),
                        scheduler=dict(type="CosLR", kwargs=dict(epochs=300, initial_epochs=10)), step_per_update=1,
                        temp=dict(start=1, target=0.0625, ntime=100000), kldweight=dict(start=0, target=0.1, ntime=100000)))
    pts = torch.from_numpy(clouds(4, 4, TINY_N)).to(dev)
    base = _model(dev, CR.TINY_CLIP, "g23.").train()
    out = []
    for seed in (11, 11, 12):
        model = copy.deepcopy(base)
        vae = _Single(model)
        opt, _ = builder.build_opti_sche(vae, cfg)
        torch.manual_seed(seed)
        l1, l2, _ = RA.train_step(vae, opt, pts, cfg, 20000)
        assert torch.isfinite(l1).all() and torch.isfinite(l2).all()
        out.append((l1.clone(), l2.clone()))
        for n, p in model.named_parameters():
            if n.startswith("visual_embed."):
                assert not p.requires_grad and torch.equal(p, dict(base.named_parameters())[n]), n
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), out
    assert not torch.equal(out[0][0], out[2][0])


def _yaml(path):
    from act_amd.utils.config import cfg_from_yaml_file
    here = os.getcwd()
    os.chdir(os.path.join(os.path.dirname(HERE), "act_amd"))
    try:
        return cfg_from_yaml_file(path)
    finally:
        os.chdir(here)


def test_stage2_step_of_the_synthetic_recipe_prefetched_or_not(dev):
    """cfgs/synthetic/pretrain_act_distill_clip.yaml shrunk to depth 2 (teacher and student) at B = 4: one training step, with the teacher forward of its
    batch prefetched on the second stream and without: finite, and the same loss bit for bit.  A first, uncompared step warms the GEMM configuration
    cache: the first use of an unlisted shape times candidates on operands drawn from the device generator, which would shift every later draw of
    that run alone."""
    from act_amd.models import build_model_from_cfg
    from act_amd.models.dvae import ACTPromptedDiscreteVAEwithVIT, _ClipBlock
    from act_amd.tools import builder
    from act_amd.tools.runner_pretrain import train_step, _Single, freeze_unused_heads
    cfg = _yaml("cfgs/synthetic/pretrain_act_distill_clip.yaml")
    cfg.model.dvae_config.visual_embed_depth = 2
    cfg.model.transformer_config.depth = 2
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = build_model_from_cfg(cfg.model).to(dev).train()
    vae = base.dvae_tokenizer
    assert type(vae) is ACTPromptedDiscreteVAEwithVIT and len(vae.visual_embed) == 3 and isinstance(vae.visual_embed[1][1], _ClipBlock) and vae.training
    pts = torch.from_numpy(clouds(31, 4, 1024)).to(dev)
    losses = []
    for prefetch in (False, False, True):
        model = copy.deepcopy(base)
        freeze_unused_heads(model)
        wrapped = _Single(model)
        opt, _ = builder.build_opti_sche(wrapped, cfg)
        torch.manual_seed(123)
        if prefetch:
            model.prefetch_teacher(pts)
            assert model._prefetched is not None and model._prefetched[0] is pts
        losses.append(train_step(wrapped, opt, pts, cfg, augment=False))
        assert model._prefetched is None
        assert all(p.grad is None for p in model.dvae_tokenizer.parameters())
    torch.cuda.synchronize()
    print(losses)
    losses = losses[1:]                                       # the warm-up step is not compared
    assert torch.isfinite(losses[0]) and torch.equal(losses[0], losses[1]), losses
