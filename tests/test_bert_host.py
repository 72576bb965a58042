"""CPU: the language teacher ACTPromptedDiscreteVAEwithBERT builds with the reference's state_dict surface, refuses what the reference cannot do,
and tests/bert_ref.py (the CPU restatement the GPU tests compare against) reproduces the reference's own arrays in tests/golden/g21_bert.npz."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_module  # noqa: E402
import bert_ref as BR  # noqa: E402

REL = 1e-5            # both sides fp32 torch on the CPU, differing only in op grouping


def _rel(a, ref):
    a = torch.as_tensor(a).detach().double(); ref = torch.as_tensor(ref).detach().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return ((a - ref).abs().max() / max(1.0, ref.abs().max())).item()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "g21_bert.npz"))


def _edict(d):
    from act_amd.utils.config import EasyDict
    return EasyDict(d)


def _tiny(**over):
    from act_amd.models import build_model_from_cfg
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return build_model_from_cfg(_edict(dict(BR.TINY_BERT, **over)))


@pytest.fixture(scope="module")
def tiny_sd():
    return {k: v.clone() for k, v in fill_module(_tiny(), "g21.").state_dict().items()}


def _masks(golden):
    return {str(n): torch.from_numpy(golden["mask." + str(n)]) for n in golden["mask_names"]}


def test_state_dict_keys_equal_the_reference(golden):
    assert list(_tiny().state_dict().keys()) == [str(k) for k in golden["keys"]]


def test_bert_ref_reproduces_visual_embedding_of_the_golden(golden, tiny_sd):
    """measured: 0.0 for the outputs and all six gradients (the same torch ops in the same order: bit-identical on this torch build)"""
    sampled, center = torch.from_numpy(golden["sampled"]), torch.from_numpy(golden["center"])
    with torch.no_grad():
        ve = BR.visual_embedding(sampled, center, tiny_sd, 2, 2, 4)
    errs = {"ve_eval": _rel(ve, golden["ve_eval"])}
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in tiny_sd.items()}
    x = sampled.clone().requires_grad_(True)
    ve = BR.visual_embedding(x, center, sd, 2, 2, 4, _masks(golden))
    errs["ve_train"] = _rel(ve, golden["ve_train"])
    (ve ** 2).sum().backward()
    errs["grad.sampled"] = _rel(x.grad, golden["grad.sampled"])
    for n in BR.GRAD_NAMES:
        errs["grad." + n] = _rel(sd[n].grad, golden["grad." + n])
    print(errs)
    assert max(errs.values()) < REL, errs


def test_bert_ref_reproduces_the_full_forward_of_the_golden(golden, tiny_sd):
    """the CPU oracle's plain tokenizer with bert_ref as its visual_embedding; measured: 0.0 for coarse, fine, logits and both losses"""
    from oracle import models as OM, layers as OL
    ora = OM.DiscreteVAE(OM.edict(BR.TINY_BERT))
    ora.load_state_dict({k: v for k, v in tiny_sd.items() if k in ora.state_dict()}, strict=True)
    ora.eval()
    ora.visual_embedding = lambda x, center, draws: BR.visual_embedding(x, center, tiny_sd, 2, 2, 4)
    torch.manual_seed(777)
    noise = -torch.empty(2, 16, 64).exponential_().log()
    with torch.no_grad():
        ret = ora(torch.from_numpy(golden["pts"]), OL.Draws({"gumbel": noise}), temperature=1.0, hard=False)
        lr, lk = ora.get_loss(ret)
    errs = {"coarse": _rel(ret[2], golden["coarse"]), "fine": _rel(ret[3], golden["fine"]), "logits": _rel(ret[5], golden["logits"]),
            "loss": _rel(torch.stack((lr, lk)).double(), golden["loss"])}
    print(errs)
    assert max(errs.values()) < REL, errs


def _yaml(path):
    from act_amd.utils.config import cfg_from_yaml_file
    here = os.getcwd()
    os.chdir(os.path.join(os.path.dirname(HERE), "act_amd"))
    try:
        return cfg_from_yaml_file(path)
    finally:
        os.chdir(here)


@pytest.mark.parametrize("path,teacher", [("cfgs/autoencoder/act_dvae_with_pretrained_bert.yaml", False),
                                          ("cfgs/synthetic/act_dvae_with_pretrained_bert.yaml", False),
                                          ("cfgs/synthetic/pretrain_act_distill_bert.yaml", True)])
def test_model_builds_from_the_yaml(path, teacher):
    from act_amd.models import build_model_from_cfg
    from act_amd.models.dvae import ACTPromptedDiscreteVAEwithBERT
    cfg = _yaml(path)
    with pytest.warns(UserWarning, match="RANDOMLY INITIALISED"):
        model = build_model_from_cfg(cfg.model)
    vae = model.dvae_tokenizer if teacher else model
    assert isinstance(vae, ACTPromptedDiscreteVAEwithBERT)
    sd = vae.state_dict()
    assert len(vae.visual_embed[0].layer) == 12 and sd["visual_embed.0.layer.11.intermediate.dense.weight"].shape == (3072, 768)
    assert "deep_prompt_tokens" not in sd and sd["visual_prompt_token"].shape == (1, 64, 768)
    assert not any(p.requires_grad for p in vae.visual_embed.parameters())
    if teacher:
        assert not any(p.requires_grad for p in vae.parameters())
    else:
        assert vae.visual_prompt_token.requires_grad and vae.proj_pre.weight.requires_grad


def test_existing_configs_keep_the_image_teacher():
    from act_amd.models import build_model_from_cfg
    from act_amd.models.dvae import ACTPromptedDiscreteVAEwithVIT
    from fill import TINY_STAGE2
    assert "NAME" not in TINY_STAGE2["dvae_config"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = build_model_from_cfg(_edict(TINY_STAGE2))
    assert type(model.dvae_tokenizer) is ACTPromptedDiscreteVAEwithVIT
    cfg = _yaml("cfgs/synthetic/pretrain_act_distill.yaml")
    assert "NAME" not in cfg.model.dvae_config
    with pytest.raises(KeyError):
        build_model_from_cfg(_edict(dict(TINY_STAGE2, dvae_config=dict(TINY_STAGE2["dvae_config"], NAME="DiscreteVAE"))))


def test_deep_prompt_builds_its_parameters_and_raises_on_forward():
    model = _tiny(use_deep_prompt=True)
    sd = model.state_dict()
    assert sd["deep_prompt_tokens"].shape == (1, 4, 64) and sd["deep_prompt_pos"].shape == (1, 4, 64)
    with pytest.raises(ValueError, match="use_deep_prompt"):
        model.visual_embedding(torch.zeros(2, 16, 64), torch.zeros(2, 16, 3))


def test_unfrozen_language_model_raises():
    with pytest.raises(NotImplementedError, match="freeze_visual_embed"):
        _tiny(freeze_visual_embed=False)


def test_no_language_model_and_no_prompts_build():
    assert _tiny(visual_embed_dim="none").visual_embed is None
    m = _tiny(num_prompt_token=0)
    assert m.visual_prompt_token is None and "visual_prompt_token" not in m.state_dict()


@pytest.mark.parametrize("prefix", ["", "encoder.", "bert.encoder."])
def test_visual_embed_ckpt_loads_a_local_state_dict(tmp_path, prefix, tiny_sd):
    enc = {prefix + k[len("visual_embed.0."):]: v for k, v in tiny_sd.items() if k.startswith("visual_embed.0.")}
    if prefix:
        enc["embeddings.word_embeddings.weight"] = torch.zeros(3, 64)        # a whole BertModel carries more than the encoder
    path = str(tmp_path / "bert.pth")
    torch.save(enc, path)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                        # a given checkpoint: no random-initialisation warning
        from act_amd.models import build_model_from_cfg
        model = build_model_from_cfg(_edict(dict(BR.TINY_BERT, visual_embed_ckpt=path)))
    for k, v in model.state_dict().items():
        if k.startswith("visual_embed.0."):
            assert torch.equal(v, tiny_sd[k]), k
    assert not any(p.requires_grad for p in model.visual_embed.parameters())


def test_qkv_weight_is_built_once_and_follows_the_weights():
    lyr = _tiny().visual_embed[0].layer[0]
    w, b = lyr.qkv()
    assert lyr.qkv()[0] is w and w.shape == (192, 64) and b.shape == (192,)
    att = getattr(lyr.attention, "self")
    assert torch.equal(w[64:128], att.key.weight) and torch.equal(b[128:], att.value.bias)
    with torch.no_grad():
        att.key.weight.add_(1.0)
    assert lyr.qkv()[0] is not w and torch.equal(lyr.qkv()[0][64:128], att.key.weight)
