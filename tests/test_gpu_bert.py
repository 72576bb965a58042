"""GPU: the language teacher (csrc/bert.hip, K.BertLayerFn, ACTPromptedDiscreteVAEwithBERT) against float64 torch, tests/bert_ref.py and the
reference's own arrays in tests/golden/g21_bert.npz.  The GPU machine has neither the reference nor ``transformers``."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_module, clouds, TINY_STAGE2, TINY_B, TINY_N  # noqa: E402
import bert_ref as BR  # noqa: E402

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
    return np.load(os.path.join(HERE, "golden", "g21_bert.npz"))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- kernel (a)
def _ln_ref(t, res, mask, gamma, beta, p, eps, dy):
    t, res, gamma, beta, dy = (v.double().requires_grad_(True) if i < 2 else v.double() for i, v in enumerate((t, res, gamma, beta, dy)))
    v = (t * mask.double() / (1.0 - p) if p > 0 else t) + res
    y = torch.nn.functional.layer_norm(v, (t.shape[1],), gamma, beta, eps)
    y.backward(dy)
    return y.detach(), t.grad, res.grad


@pytest.mark.parametrize("T,D", [(37, 64), (256, 768)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_dropout_add_layernorm_against_float64(dev, K, T, D, p):
    g = _gen(T + D)
    t, res, dy = (torch.randn(T, D, generator=g) for _ in range(3))
    gamma, beta = 1.0 + 0.1 * torch.randn(D, generator=g), 0.05 * torch.randn(D, generator=g)
    mask = (torch.rand(T, D, generator=g) >= p).float()
    y_ref, dt_ref, dres_ref = _ln_ref(t, res, mask, gamma, beta, p, 1e-12, dy)
    d = lambda v: v.to(dev)        # noqa: E731
    y, rstd = K.dropout_add_layernorm_fwd(d(t), d(res), d(gamma), d(beta), 1e-12, p, 0, d(mask) if p > 0 else None)
    dt, dres = K.dropout_add_layernorm_bwd(d(dy), y, d(gamma), d(beta), rstd, p, 0, d(mask) if p > 0 else None)
    errs = dict(y=_rel(y, y_ref), dt=_rel(dt, dt_ref), dres=_rel(dres, dres_ref))
    print(errs)
    assert max(errs.values()) <= TOL, errs


def test_dropout_add_layernorm_philox(dev, K):
    """the mask the Philox path used is read off a second call (t = 1, res = 0, gamma = 1, beta = 0: a kept entry normalises to a positive value, a
    dropped one to a negative one), then the Philox output / backward must equal the injected-mask ones bit for bit; keep rate, seeds, seed_dev"""
    T, D, p = 64, 256, 0.1
    g = _gen(5)
    t, res, dy = (torch.randn(T, D, generator=g).to(dev) for _ in range(3))
    gamma, beta = (1.0 + 0.1 * torch.randn(D, generator=g)).to(dev), (0.05 * torch.randn(D, generator=g)).to(dev)
    one, zero = torch.ones(D, device=dev), torch.zeros(D, device=dev)

    def mask_of(seed, ctr=None):
        probe, _ = K.dropout_add_layernorm_fwd(torch.ones(T, D, device=dev), torch.zeros(T, D, device=dev), one, zero, 1e-12, p, seed, None, ctr)
        return (probe > 0).float()
    m = mask_of(1234)
    n = T * D
    assert abs(m.mean().item() - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5, m.mean().item()
    y, rstd = K.dropout_add_layernorm_fwd(t, res, gamma, beta, 1e-12, p, 1234)
    y_m, rstd_m = K.dropout_add_layernorm_fwd(t, res, gamma, beta, 1e-12, p, 0, m)
    assert torch.equal(y, y_m) and torch.equal(rstd, rstd_m)
    dt, dres = K.dropout_add_layernorm_bwd(dy, y, gamma, beta, rstd, p, 1234)
    dt_m, dres_m = K.dropout_add_layernorm_bwd(dy, y, gamma, beta, rstd, p, 0, m)
    assert torch.equal(dt, dt_m) and torch.equal(dres, dres_m)
    assert not torch.equal(m, mask_of(1235))
    c0, c1 = torch.zeros(1, dtype=torch.int64, device=dev), torch.ones(1, dtype=torch.int64, device=dev)
    assert torch.equal(m, mask_of(1234, c0)) and not torch.equal(m, mask_of(1234, c1))


# ---------------------------------------------------------------------------------------------- kernel (b)
def _attn_ref(qkv, mask, p, dout):
    """float64: qkv [B,S,3,H,hd], mask [B,H,S,S] -> out [B*S, H*hd], dqkv"""
    qkv = qkv.double().requires_grad_(True)
    B, S, _, H, hd = qkv.shape
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    probs = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1)
    out = ((probs * mask.double() / (1.0 - p)) @ v).transpose(1, 2).reshape(B * S, H * hd)
    out.backward(dout.double())
    return out.detach(), qkv.grad


@pytest.mark.parametrize("S", [5, 20, 128, 200])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_dropout_against_float64(dev, K, S, hd, p):
    B, H = 2, 2
    g = _gen(S * 7 + hd)
    qkv = torch.randn(B, S, 3, H, hd, generator=g)
    dout = torch.randn(B * S, H * hd, generator=g)
    mask = (torch.rand(B, H, S, S, generator=g) >= p).to(torch.uint8)
    mask[0, 1, S // 2] = 0                                        # a query whose every key is dropped: zeros, not NaN
    out_ref, dqkv_ref = _attn_ref(qkv, mask, p, dout)
    qd, md, dd = qkv.to(dev), mask.to(dev), dout.to(dev)
    out, lse = K.attention_dropout_fwd(qd, B, S, H, hd, p, 0, md)
    dqkv = K.attention_dropout_bwd(qd, out, dd, lse, B, S, H, hd, p, 0, md)
    assert torch.isfinite(out).all() and torch.isfinite(dqkv).all()
    assert out.view(B, S, H, hd)[0, S // 2, 1].abs().max().item() == 0.0
    errs = dict(out=_rel(out, out_ref), dq=_rel(dqkv[:, :, 0], dqkv_ref[:, :, 0]), dk=_rel(dqkv[:, :, 1], dqkv_ref[:, :, 1]),
                dv=_rel(dqkv[:, :, 2], dqkv_ref[:, :, 2]))
    print(errs)
    assert max(errs.values()) <= TOL, errs


def test_attention_dropout_philox(dev, K):
    """S = hd = 32 and v = identity: out (1-p) / P is the keep mask the forward used"""
    B, H, S, hd, p = 2, 2, 32, 32, 0.1
    g = _gen(11)
    qkv = 0.5 * torch.randn(B, S, 3, H, hd, generator=g)
    qkv[:, :, 2] = torch.eye(S).view(1, S, 1, hd)
    qkv = qkv.to(dev)
    dout = torch.randn(B * S, H * hd, generator=g).to(dev)
    q, k = qkv[:, :, 0].transpose(1, 2).double(), qkv[:, :, 1].transpose(1, 2).double()
    probs = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1)               # [B,H,S,S], every entry far above fp32 noise

    def run(seed, ctr=None):
        out, lse = K.attention_dropout_fwd(qkv, B, S, H, hd, p, seed, None, ctr)
        ratio = out.view(B, S, H, hd).transpose(1, 2).double() * (1 - p) / probs
        assert ((ratio - ratio.round()).abs() < 1e-3).all() and ratio.round().min() >= 0 and ratio.round().max() <= 1
        return out, lse, ratio.round().to(torch.uint8).contiguous()
    out, lse, m = run(99)
    n = B * H * S * S
    assert abs(m.float().mean().item() - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5, m.float().mean().item()       # +- 0.023
    out_m, lse_m = K.attention_dropout_fwd(qkv, B, S, H, hd, p, 0, m)
    assert torch.equal(out, out_m) and torch.equal(lse, lse_m)
    dqkv = K.attention_dropout_bwd(qkv, out, dout, lse, B, S, H, hd, p, 99)
    dqkv_m = K.attention_dropout_bwd(qkv, out, dout, lse, B, S, H, hd, p, 0, m)
    assert torch.equal(dqkv, dqkv_m)
    assert not torch.equal(m, run(100)[2])
    c0, c1 = torch.zeros(1, dtype=torch.int64, device=dev), torch.ones(1, dtype=torch.int64, device=dev)
    assert torch.equal(m, run(99, c0)[2]) and not torch.equal(m, run(99, c1)[2])


# ---------------------------------------------------------------------------------------------- layer
def _layer_weights(dev, D, inter, seed):
    g = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=g)        # noqa: E731
    w = dict(wqkv=r(3 * D, D) / D ** 0.5, bqkv=0.05 * r(3 * D), wo=r(D, D) / D ** 0.5, bo=0.05 * r(D), g1=1 + 0.1 * r(D), b1=0.05 * r(D),
             wi=r(inter, D) / D ** 0.5, bi=0.05 * r(inter), wo2=r(D, inter) / inter ** 0.5, bo2=0.05 * r(D), g2=1 + 0.1 * r(D), b2=0.05 * r(D))
    return {k: v.to(dev) for k, v in w.items()}


def test_layer_at_p0_is_the_existing_attention_bit_for_bit(dev, K):
    B, S, D, H = 2, 20, 64, 2
    w = _layer_weights(dev, D, 256, 3)
    x = torch.randn(B, S, D, generator=_gen(4)).to(dev).requires_grad_(True)
    seen = {}
    real_f, real_b = K.attention_fwd, K.attention_bwd

    def fwd(qkv, *a, **k):
        seen["qkv"] = qkv
        seen["out"], seen["lse"] = real_f(qkv, *a, **k)
        return seen["out"], seen["lse"]

    def bwd(qkv, out, dout, lse, *a):
        seen["dout"] = dout
        seen["dqkv"] = real_b(qkv, out, dout, lse, *a)
        return seen["dqkv"]
    K.attention_fwd, K.attention_bwd = fwd, bwd
    try:
        y = K.bert_layer(x, *w.values(), H, 1e-12, 0.0, 0.0)
        y.square().sum().backward()
    finally:
        K.attention_fwd, K.attention_bwd = real_f, real_b
    assert set(seen) == {"qkv", "out", "lse", "dout", "dqkv"}              # the p = 0 layer went through the existing kernels ...
    out, lse = K.attention_fwd(seen["qkv"], B, S, H, D // H)
    assert torch.equal(out, seen["out"]) and torch.equal(lse, seen["lse"])   # ... and what it got is what they give on the same qkv
    assert torch.equal(K.attention_bwd(seen["qkv"], out, seen["dout"], lse, B, S, H, D // H), seen["dqkv"])
    with torch.no_grad():
        assert torch.equal(K.bert_layer(x.detach(), *w.values(), H, 1e-12, 0.0, 0.0), y)


# ---------------------------------------------------------------------------------------------- model
def _model(dev, cfg, prefix):
    from act_amd.models import build_model_from_cfg
    from act_amd.utils.config import EasyDict
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = build_model_from_cfg(EasyDict(cfg))
    return fill_module(model, prefix).to(dev)


def _check_visual_embedding(dev, model, sampled, center, masks, want_eval, want_train, want_grads):
    from act_amd.utils.draws import Draws
    model.eval()
    with torch.no_grad():
        e_eval = _rel(model.visual_embedding(sampled.to(dev), center.to(dev)), want_eval)
    model.train()
    model.zero_grad()
    x = sampled.to(dev).requires_grad_(True)
    ve = model.visual_embedding(x, center.to(dev), Draws(masks, device=dev))
    errs = {"ve_eval": e_eval, "ve_train": _rel(ve, want_train)}
    (ve ** 2).sum().backward()
    pd = dict(model.named_parameters())
    errs["grad.sampled"] = _rel(x.grad, want_grads["sampled"])
    for n in BR.GRAD_NAMES:
        errs["grad." + n] = _rel(pd[n].grad, want_grads[n])
    assert all(p.grad is None for n, p in pd.items() if n.startswith("visual_embed."))
    print(errs)
    assert max(errs.values()) <= TOL, errs


def test_visual_embedding_matches_the_reference_golden(dev, golden):
    model = _model(dev, BR.TINY_BERT, "g21.")
    masks = {str(n): torch.from_numpy(golden["mask." + str(n)]) for n in golden["mask_names"]}
    grads = {n: golden["grad." + n] for n in BR.GRAD_NAMES + ("sampled",)}
    _check_visual_embedding(dev, model, torch.from_numpy(golden["sampled"]), torch.from_numpy(golden["center"]), masks, golden["ve_eval"],
                            golden["ve_train"], grads)


def test_visual_embedding_matches_bert_ref_at_head_dim_64(dev):
    B, G, Pn, D, H = 2, 32, 8, 128, 2
    cfg = dict(BR.TINY_BERT, num_group=G, num_prompt_token=Pn, visual_embed_dim=D, visual_embed_heads=H, visual_embed_intermediate=512)
    model = _model(dev, cfg, "g21b.")
    g = _gen(64)
    sampled, center = torch.randn(B, G, 64, generator=g), torch.from_numpy(clouds(22, B, G))
    S = Pn + G
    shapes = {"prompt.0": (B, Pn, D)}
    for i in range(2):
        shapes.update({f"bert.{i}.attn": (B, H, S, S), f"bert.{i}.hidden1": (B, S, D), f"bert.{i}.hidden2": (B, S, D)})
    masks = {k: (torch.rand(s, generator=g) >= 0.1).to(torch.uint8) for k, s in shapes.items()}
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        want_eval = BR.visual_embedding(sampled, center, sd, H, 2, Pn)
    sdg = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    x = sampled.clone().requires_grad_(True)
    want_train = BR.visual_embedding(x, center, sdg, H, 2, Pn, masks)
    (want_train ** 2).sum().backward()
    grads = {n: sdg[n].grad for n in BR.GRAD_NAMES}
    grads["sampled"] = x.grad
    _check_visual_embedding(dev, model, sampled, center, masks, want_eval, want_train.detach(), grads)


def test_full_forward_matches_the_reference_golden(dev, golden):
    from act_amd.utils.draws import Draws
    model = _model(dev, BR.TINY_BERT, "g21.").eval()
    torch.manual_seed(777)
    noise = -torch.empty(2, 16, 64).exponential_().log()
    pts = torch.from_numpy(golden["pts"]).to(dev)
    with torch.no_grad():
        ret = model(pts, temperature=1.0, hard=False, draws=Draws({"gumbel": noise}, device=dev))
        lr, lk = model.get_loss(ret, pts)
    errs = {"coarse": _rel(ret[2], golden["coarse"]), "fine": _rel(ret[3], golden["fine"]), "logits": _rel(ret[5], golden["logits"]),
            "loss": _rel(torch.stack((lr.reshape(()), lk.reshape(()))).double(), golden["loss"])}
    print(errs)
    assert max(errs.values()) <= TOL, errs


def test_promptless_frozen_teacher_passes_no_gradient_upstream(dev):
    """num_prompt_token: 0 runs the frozen language model under no_grad (models/dvae.py:766-768): proj_post learns, proj_pre and the codes do not"""
    model = _model(dev, dict(BR.TINY_BERT, num_prompt_token=0), "g21c.").train()
    x = torch.randn(2, 16, 64, generator=_gen(1)).to(dev).requires_grad_(True)
    model.visual_embedding(x, torch.from_numpy(clouds(21, 2, 16)).to(dev)).square().sum().backward()
    assert x.grad is None and model.proj_pre.weight.grad is None and model.proj_post.weight.grad is not None
    novit = _model(dev, dict(BR.TINY_BERT, visual_embed_dim="none"), "g21d.")
    assert novit.visual_embedding(x, None) is x


def test_train_mode_draws_fresh_masks_and_eval_none(dev):
    model = _model(dev, BR.TINY_BERT, "g21.").train()
    x, c = torch.randn(2, 16, 64, generator=_gen(2)).to(dev), torch.from_numpy(clouds(21, 2, 16)).to(dev)
    with torch.no_grad():
        a, b = model.visual_embedding(x, c), model.visual_embedding(x, c)
        assert not torch.equal(a, b)                                     # both dropouts follow module.training, not requires_grad
        nb = torch.randn(2, 16, 8, 3, generator=_gen(3)).to(dev)
        f0 = model.forward_tokenizer_features(nb, c)                      # this class's default: return_global=False
        assert f0.shape == (2, 16, 64)
        model.eval()
        assert torch.equal(model.visual_embedding(x, c), model.visual_embedding(x, c))


# ---------------------------------------------------------------------------------------------- training steps
def test_stage1_step_trains_prompts_only_and_never_syncs(dev):
    from act_amd.tools import builder
    from act_amd.tools.runner_pretrain import _Single
    from act_amd.tools import runner_autoencoder as RA
    from act_amd.utils.config import EasyDict
    vae = _Single(_model(dev, BR.TINY_BERT, "g21.").train())
    cfg = EasyDict(dict(optimizer=dict(type="AdamW", kwargs=dict(lr=1e-3, weight_decay=0.05)),
                        scheduler=dict(type="CosLR", kwargs=dict(epochs=300, initial_epochs=10)), step_per_update=1,
                        temp=dict(start=1, target=0.0625, ntime=100000), kldweight=dict(start=0, target=0.1, ntime=100000)))
    opt, _ = builder.build_opti_sche(vae, cfg)
    pts = torch.from_numpy(clouds(4, 4, TINY_N)).to(dev)
    before = {n: p.detach().clone() for n, p in vae.named_parameters()}
    losses = [RA.train_step(vae, opt, pts, cfg, 20000 + i) for i in range(2)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses.append(RA.train_step(vae, opt, pts, cfg, 20002))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for out in losses:
        for v in (out if isinstance(out, (tuple, list)) else (out,)):
            if torch.is_tensor(v):
                assert torch.isfinite(v).all()
    for n, p in vae.named_parameters():
        frozen = ".visual_embed." in "." + n
        assert torch.equal(p, before[n]) == frozen, n
        assert p.requires_grad != frozen, n


def _stage2(dev, **dvae):
    return _model(dev, dict(TINY_STAGE2, dvae_config=dict(TINY_STAGE2["dvae_config"], **dvae)), "g4.").train()


def _bert_teacher_cfg():
    return dict(NAME="ACTPromptedDiscreteVAEwithBERT", visual_embed_type="bert-base-uncased", visual_embed_dim=64, use_deep_prompt=False,
                num_prompt_token=4, visual_embed_intermediate=256)


def test_stage2_step_with_the_language_teacher_prefetched_or_not(dev, golden):
    from act_amd.models.dvae import ACTPromptedDiscreteVAEwithBERT
    from act_amd.utils.draws import Draws
    model = _stage2(dev, **_bert_teacher_cfg())
    assert type(model.dvae_tokenizer) is ACTPromptedDiscreteVAEwithBERT and model.dvae_tokenizer.training
    pts = torch.from_numpy(clouds(4, TINY_B, TINY_N)).to(dev)
    g4 = np.load(os.path.join(HERE, "golden", "g4_stage2.npz"))
    torch.manual_seed(777)
    table = {"mask": torch.from_numpy(g4["mask"]), "gumbel": -torch.empty(TINY_B, 16, 64).exponential_().log()}
    table.update({str(n): torch.from_numpy(golden["mask." + str(n)]) for n in golden["mask_names"]})      # S = 4 + 16 here too
    loss0 = model(pts, draws=Draws(table, device=dev))
    model.prefetch_teacher(pts, draws=Draws(table, device=dev))
    assert model._prefetched is not None
    loss1 = model(pts, draws=Draws(table, device=dev))
    assert torch.isfinite(loss0) and torch.equal(loss0, loss1)
    loss1.backward()
    assert all(p.grad is None for p in model.dvae_tokenizer.parameters())
    # without injected draws the teacher draws from its device-resident stream: two forwards differ, and prefetch still feeds the step
    model.prefetch_teacher(pts)
    assert torch.isfinite(model(pts))


def test_stage2_default_teacher_is_unchanged(dev):
    """the existing tiny Stage-II golden through the new build_tokenizer: same class, same loss with and without the explicit default name"""
    from act_amd.models.dvae import ACTPromptedDiscreteVAEwithVIT
    from act_amd.utils.draws import Draws
    g4 = np.load(os.path.join(HERE, "golden", "g4_stage2.npz"))
    pts = torch.from_numpy(clouds(4, TINY_B, TINY_N)).to(dev)
    losses = []
    for extra in ({}, {"NAME": "ACTPromptedDiscreteVAEwithVIT"}):
        model = _stage2(dev, **extra)
        assert type(model.dvae_tokenizer) is ACTPromptedDiscreteVAEwithVIT
        model.dvae_tokenizer.prompt_dropout.p = 0.0
        torch.manual_seed(777)
        draws = Draws({"mask": torch.from_numpy(g4["mask"]), "gumbel": -torch.empty(TINY_B, 16, 64).exponential_().log()}, device=dev)
        losses.append(model(pts, draws=draws))
    assert torch.equal(losses[0], losses[1]) and abs(losses[0].item() - g4["loss"][0]) <= TOL
