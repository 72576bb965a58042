"""CPU: the CLIP image teacher (``visual_embed_type: clip:ViT-B/16`` of ACTPromptedDiscreteVAEwithVIT) builds with the reference's state_dict surface, loads
local CLIP files in every form it promises, refuses what it does not compute, and tests/clip_ref.py (the CPU restatement the GPU tests compare against)
reproduces the reference's own arrays in tests/golden/g23_clip.npz."""
import os
import sys
import warnings
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_module, fill_tensor  # noqa: E402
import clip_ref as CR  # noqa: E402

REL = 1e-5            # both sides fp32 torch on the CPU, differing only in op grouping (nn.MultiheadAttention scales q before the product)


def _rel(a, ref):
    a = torch.as_tensor(a).detach().double(); ref = torch.as_tensor(ref).detach().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return ((a - ref).abs().max() / max(1.0, ref.abs().max())).item()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "g23_clip.npz"))


def _edict(d):
    from act_amd.utils.config import EasyDict
    return EasyDict(d)


def _tiny(quiet=True, **over):
    from act_amd.models import build_model_from_cfg
    with warnings.catch_warnings():
        if quiet:
            warnings.simplefilter("ignore")
        return build_model_from_cfg(_edict(dict(CR.TINY_CLIP, **over)))


@pytest.fixture(scope="module")
def tiny_sd():
    return {k: v.clone() for k, v in fill_module(_tiny(), "g23.").state_dict().items()}


# ---------------------------------------------------------------------------------------------- the state_dict surface
def test_state_dict_keys_equal_the_reference(golden):
    model = _tiny()
    assert len(model.visual_embed) == 3
    assert list(model.state_dict().keys()) == [str(k) for k in golden["keys"]]
    assert list(_tiny(num_prompt_token=0).state_dict().keys()) == [str(k) for k in golden["keys_noprompt"]]
    sd = {str(k): fill_tensor("any." + str(k), model.state_dict()[str(k)].shape) for k in golden["keys"] if "num_batches_tracked" not in str(k)}
    sd.update({k: v for k, v in model.state_dict().items() if "num_batches_tracked" in k})
    model.load_state_dict(sd, strict=True)
    blk = model.visual_embed[1][0]
    assert blk.attn.in_proj_weight.shape == (192, 64) and blk.mlp.c_fc.weight.shape == (256, 64) and blk.ln_1.eps == 1e-5 == model.visual_embed[2].eps
    assert not any(p.requires_grad for p in model.visual_embed.parameters()) and model.visual_prompt_token.requires_grad


@pytest.mark.parametrize("name,width,depth,heads", [("clip:ViT-B/16", 768, 12, 12), ("clip:ViT-B/32", 768, 12, 12), ("clip:ViT-L/14", 1024, 24, 16)])
def test_geometries(name, width, depth, heads):
    from act_amd.models.dvae import _CLIP_GEOMETRY
    assert _CLIP_GEOMETRY[name[5:].lower()] == (depth, heads) and width // heads == 64
    # built small through the overrides (a full ViT-L on the CPU is seconds of initialisation): depth override honoured, heads from the table
    model = _tiny(visual_embed_type=name, visual_embed_dim=width, visual_embed_depth=1, visual_embed_heads=None, tokens_dims=64)
    assert len(model.visual_embed[1]) == 1 and model.visual_embed[1][0].num_heads == heads
    assert model.state_dict()["visual_embed.1.0.attn.in_proj_weight"].shape == (3 * width, width)


def test_a_timm_name_still_builds_the_timm_keys():
    model = _tiny(visual_embed_type="vit_base_patch16_384")
    keys = [k for k in model.state_dict() if k.startswith("visual_embed.")]
    assert len(model.visual_embed) == 2 and "visual_embed.0.0.attn.qkv.weight" in keys and "visual_embed.1.weight" in keys
    assert not any("in_proj" in k or "ln_1" in k for k in keys) and model.visual_embed[1].eps == 1e-6


def test_the_random_teacher_warns_loudly():
    with pytest.warns(UserWarning, match="RANDOMLY INITIALISED"):
        _tiny(quiet=False)


# ---------------------------------------------------------------------------------------------- the refusals
def test_deep_prompts_raise_valueerror_and_say_why():
    with pytest.raises(ValueError, match="attention runs across the clouds of a batch"):
        _tiny(use_deep_prompt=True)


def test_an_unfrozen_teacher_raises_notimplemented():
    with pytest.raises(NotImplementedError, match="freeze_visual_embed"):
        _tiny(freeze_visual_embed=False)


def test_a_tower_without_transformer_blocks_is_refused():
    with pytest.raises(ValueError, match="clip:vit-b/16"):
        _tiny(visual_embed_type="clip:RN50", visual_embed_depth=None, visual_embed_heads=None)
    with pytest.raises(ValueError, match="head dimensions"):
        _tiny(visual_embed_heads=4)                  # head dimension 16


# ---------------------------------------------------------------------------------------------- visual_embed_ckpt
class _Quick(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class _Res(nn.Module):
    def __init__(self, d, h):
        super().__init__()
        self.attn = nn.MultiheadAttention(d, h)
        self.ln_1 = nn.LayerNorm(d)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(d, 4 * d)), ("gelu", _Quick()), ("c_proj", nn.Linear(4 * d, d))]))
        self.ln_2 = nn.LayerNorm(d)

    def forward(self, x):
        y = self.ln_1(x)
        x = x + self.attn(y, y, y, need_weights=False)[0]
        return x + self.mlp(self.ln_2(x))


class _Visual(nn.Module):
    def __init__(self, d=64, layers=2, h=2):
        super().__init__()
        self.ln_pre = nn.LayerNorm(d)
        self.transformer = nn.Module()
        self.transformer.resblocks = nn.Sequential(*[_Res(d, h) for _ in range(layers)])
        self.ln_post = nn.LayerNorm(d)

    def forward(self, x):
        return self.ln_post(self.transformer.resblocks(self.ln_pre(x)))


class _Tower(nn.Module):
    """the tiny visual tower in full-CLIP form: keys ``visual.ln_pre.*``, ``visual.transformer.resblocks.{i}.*``, ``visual.ln_post.*`` plus other keys a
    real CLIP file carries (text tower, logit_scale), which the loader must ignore"""

    def __init__(self):
        super().__init__()
        self.visual = _Visual()
        self.logit_scale = nn.Parameter(torch.ones([]))
        self.token_embedding = nn.Embedding(8, 64)

    def forward(self, x):
        return self.visual(x)


@pytest.fixture(scope="module")
def tower():
    torch.manual_seed(5)
    t = fill_module(_Tower(), "g23t.").eval()
    return t


def _assert_loaded(model, tower, atol):
    want = tower.visual.state_dict()
    got = model.state_dict()
    n = 0
    for k, v in want.items():
        k2 = ("visual_embed.0." + k[7:] if k.startswith("ln_pre.") else "visual_embed.2." + k[8:] if k.startswith("ln_post.")
              else "visual_embed.1." + k[len("transformer.resblocks."):])
        assert got[k2].dtype == torch.float32 and (got[k2] - v).abs().max().item() <= atol, k2
        n += 1
    assert n == len([k for k in got if k.startswith("visual_embed.")]) == 4 + 12 * 2


def test_ckpt_full_clip_form_fp16(tmp_path, tower):
    path = str(tmp_path / "clip_fp16.pt")
    torch.save({k: v.half() if v.is_floating_point() else v for k, v in tower.state_dict().items()}, path)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # a given file: no "RANDOMLY INITIALISED" warning
        model = _tiny(quiet=False, visual_embed_ckpt=path)
    _assert_loaded(model, tower, 2e-3)                       # fp16 rounding of values up to ~1.4: half an ulp is 2^-11 ~ 4.9e-4 (x 2 for the range [2, 4))
    assert not any(p.requires_grad for p in model.visual_embed.parameters())


def test_ckpt_visual_embed_form(tmp_path, tower):
    src = fill_module(_tiny(), "g23.")
    path = str(tmp_path / "visual_embed.pt")
    torch.save({k: v for k, v in src.state_dict().items() if k.startswith("visual_embed.")}, path)
    model = _tiny(visual_embed_ckpt=path)
    for k, v in src.state_dict().items():
        if k.startswith("visual_embed."):
            assert torch.equal(model.state_dict()[k], v), k


def test_ckpt_torchscript_archive(tmp_path, tower):
    path = str(tmp_path / "clip_jit.pt")
    torch.jit.save(torch.jit.trace(tower, torch.zeros(3, 1, 64)), path)
    model = _tiny(visual_embed_ckpt=path)
    _assert_loaded(model, tower, 0.0)


def test_ckpt_missing_or_misshaped_key_is_named(tmp_path, tower):
    sd = dict(tower.state_dict())
    del sd["visual.transformer.resblocks.1.mlp.c_fc.bias"]
    path = str(tmp_path / "missing.pt")
    torch.save(sd, path)
    with pytest.raises(KeyError, match=r"visual_embed\.1\.1\.mlp\.c_fc\.bias"):
        _tiny(visual_embed_ckpt=path)
    sd = dict(tower.state_dict())
    sd["visual.ln_post.weight"] = torch.ones(65)
    path = str(tmp_path / "shape.pt")
    torch.save(sd, path)
    with pytest.raises(ValueError, match=r"visual_embed\.2\.weight"):
        _tiny(visual_embed_ckpt=path)


# ---------------------------------------------------------------------------------------------- recipes
def _yaml(path):
    from act_amd.utils.config import cfg_from_yaml_file
    here = os.getcwd()
    os.chdir(os.path.join(os.path.dirname(HERE), "act_amd"))
    try:
        return cfg_from_yaml_file(path)
    finally:
        os.chdir(here)


@pytest.mark.parametrize("path,teacher", [("cfgs/autoencoder/act_dvae_with_pretrained_clip.yaml", False),
                                          ("cfgs/synthetic/act_dvae_with_pretrained_clip.yaml", False),
                                          ("cfgs/synthetic/pretrain_act_distill_clip.yaml", True)])
def test_model_builds_from_the_yaml(path, teacher):
    from act_amd.models import build_model_from_cfg
    from act_amd.models.dvae import ACTPromptedDiscreteVAEwithVIT
    cfg = _yaml(path)
    with pytest.warns(UserWarning, match="RANDOMLY INITIALISED"):
        model = build_model_from_cfg(cfg.model)
    vae = model.dvae_tokenizer if teacher else model
    assert type(vae) is ACTPromptedDiscreteVAEwithVIT and len(vae.visual_embed) == 3
    sd = vae.state_dict()
    assert len(vae.visual_embed[1]) == 12 and sd["visual_embed.1.11.mlp.c_fc.weight"].shape == (3072, 768) and vae.visual_embed[1][0].num_heads == 12
    assert "deep_prompt_tokens" not in sd and sd["visual_prompt_token"].shape == (1, 64, 768)
    assert not any(p.requires_grad for p in vae.visual_embed.parameters())
    if teacher:
        assert not any(p.requires_grad for p in vae.parameters())
    else:
        assert vae.visual_prompt_token.requires_grad and vae.proj_pre.weight.requires_grad


def test_the_autoencoder_recipe_carries_the_reference_keys():
    ref, new = _yaml("cfgs/autoencoder/act_dvae_with_pretrained_transformer.yaml"), _yaml("cfgs/autoencoder/act_dvae_with_pretrained_clip.yaml")
    assert set(ref.model) == set(new.model) and new.model.visual_embed_type == "clip:ViT-B/16" and new.model.use_deep_prompt is False
    diff = {k for k in ref.model if ref.model[k] != new.model[k]}
    assert diff == {"visual_embed_type", "use_deep_prompt"}
    for k in ("optimizer", "scheduler", "temp", "kldweight", "total_bs", "max_epoch"):
        assert ref[k] == new[k], k


# ---------------------------------------------------------------------------------------------- the restatement against the reference's arrays
def test_clip_ref_reproduces_every_array_of_the_golden(golden, tiny_sd):
    sampled, center = torch.from_numpy(golden["sampled"]), torch.from_numpy(golden["center"])
    with torch.no_grad():
        errs = {"ve_eval": _rel(CR.visual_embedding(sampled, center, tiny_sd, 2, 2, 4), golden["ve_eval"])}
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in tiny_sd.items()}
    x = sampled.clone().requires_grad_(True)
    ve = CR.visual_embedding(x, center, sd, 2, 2, 4, {"prompt.0": torch.from_numpy(golden["mask.prompt.0"])})
    errs["ve_train"] = _rel(ve, golden["ve_train"])
    (ve ** 2).sum().backward()
    errs["grad.sampled"] = _rel(x.grad, golden["grad.sampled"])
    for n in CR.GRAD_NAMES:
        errs["grad." + n] = _rel(sd[n].grad, golden["grad." + n])
    # no prompts: frozen and under no_grad
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in tiny_sd.items() if "prompt" not in k}
    x = sampled.clone().requires_grad_(True)
    ve = CR.visual_embedding(x, center, sd, 2, 2, 0)
    errs["ve_noprompt"] = _rel(ve, golden["ve_noprompt"])
    (ve ** 2).sum().backward()
    errs["grad_noprompt.proj_post.bias"] = _rel(sd["proj_post.bias"].grad, golden["grad_noprompt.proj_post.bias"])
    assert bool(golden["noprompt_proj_pre_grad_is_none"]) and sd["proj_pre.weight"].grad is None and x.grad is None
    print(errs)
    assert max(errs.values()) < REL, errs
