#!/usr/bin/env python3
"""Generate tests/golden/g23_clip.npz from the REFERENCE'S OWN ACTPromptedDiscreteVAEwithVIT (models/dvae.py:360-615) with a CLIP teacher
(``visual_embed_type: clip:ViT-B/16``, :394-403, :500-511), on the CPU, with the import shims of make_golden.py.

The ``clip`` package is not installed and nothing is downloaded: a stub module named ``clip`` is put into ``sys.modules`` BEFORE the reference is imported.
Its ``load()`` returns a tiny visual tower written here from CLIP's public model definition -- ``ln_pre``, ``transformer.resblocks`` (each
``nn.MultiheadAttention`` + ``nn.LayerNorm`` (eps 1e-5) + ``c_fc`` / QuickGELU / ``c_proj``), ``ln_post`` -- and records that it was called; the script asserts
that it was the one called.  Parameters are then filled by name (fill.py): no weights are stored.

Geometry as g21_bert.npz: B = 2, G = 16, Pn = 4 -> S = 20 tokens (no multiple of 16), D = 64, 2 heads (head dimension 32), depth 2.

Run:  python tests/golden/make_golden_clip.py      (build container only: the reference never travels)
"""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
from fill import fill_module, fill_tensor, clouds  # noqa: E402

B, G, PN, D, HEADS, DEPTH = 2, 16, 4, 64, 2, 2
CFG = dict(NAME="ACTPromptedDiscreteVAEwithVIT", group_size=8, num_group=G, num_tokens=64, encoder_dims=64, tokens_dims=64, decoder_dims=64,
           visual_embed_type="clip:ViT-B/16", visual_embed_dim=D, freeze_visual_embed=True, num_prompt_token=PN, use_deep_prompt=False)
GRAD_NAMES = ["visual_prompt_token", "visual_prompt_pos", "proj_pre.weight", "visual_pos_embed.0.weight", "proj_post.bias"]
CALLS = []


class QuickGELU(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class ResidualAttentionBlock(nn.Module):
    """CLIP's residual block: sequence-first input [L, N, D]"""

    def __init__(self, d_model, n_head):
        super().__init__()
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ln_1 = nn.LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(d_model, d_model * 4)), ("gelu", QuickGELU()),
                                              ("c_proj", nn.Linear(d_model * 4, d_model))]))
        self.ln_2 = nn.LayerNorm(d_model)

    def forward(self, x):
        y = self.ln_1(x)
        x = x + self.attn(y, y, y, need_weights=False)[0]
        return x + self.mlp(self.ln_2(x))


class TinyClip(nn.Module):
    """what the reference reads of ``clip.load(...)[0]``: visual.ln_pre, visual.transformer.{resblocks, layers}, visual.ln_post"""

    def __init__(self, width=D, layers=DEPTH, heads=HEADS):
        super().__init__()
        self.visual = nn.Module()
        self.visual.ln_pre = nn.LayerNorm(width)
        self.visual.transformer = nn.Module()
        self.visual.transformer.width, self.visual.transformer.layers = width, layers
        self.visual.transformer.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads) for _ in range(layers)])
        self.visual.ln_post = nn.LayerNorm(width)


def stub_load(name, *args, **kwargs):
    CALLS.append(name)
    return TinyClip(), None


def build(dvae, cfg):
    from easydict import EasyDict
    n = len(CALLS)
    model = dvae.ACTPromptedDiscreteVAEwithVIT(EasyDict(cfg))
    assert CALLS[n:] == ["ViT-B/16"], f"the stub clip.load must be the one called, exactly once: {CALLS[n:]}"
    assert len(model.visual_embed) == 3
    return fill_module(model, "g23.")


def main():
    os.chdir(MG.REF)
    MG.install_shims()
    MG._mod("clip", load=stub_load)
    import models.dvae as dvae
    import clip
    assert clip.load is stub_load
    torch.set_num_threads(8)
    torch.manual_seed(0)
    model = build(dvae, CFG)
    keys = list(model.state_dict().keys())

    sampled = fill_tensor("g23.in.sampled", (B, G, 64), "code")
    center = torch.from_numpy(clouds(23, B, G))

    model.eval()
    with torch.no_grad():
        ve_eval = model.visual_embedding(sampled, center)

    # train mode: record the prompt dropout's draw (the only dropout of the graph: nn.MultiheadAttention is built with dropout 0)
    recorded = []
    real_dropout = F.dropout

    def recording_dropout(input, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return input
        keep = torch.rand_like(input) >= p
        recorded.append(keep.to(torch.uint8))
        return input * keep.to(input.dtype) / (1.0 - p)
    model.train()
    x = sampled.clone().requires_grad_(True)
    F.dropout = recording_dropout
    try:
        torch.manual_seed(23)
        ve_train = model.visual_embedding(x, center)
    finally:
        F.dropout = real_dropout
    (ve_train ** 2).sum().backward()
    assert [tuple(m.shape) for m in recorded] == [(B, PN, D)], [tuple(m.shape) for m in recorded]
    pd = dict(model.named_parameters())
    assert all(p.grad is None for n, p in pd.items() if n.startswith("visual_embed."))
    grads = {"grad." + n: pd[n].grad for n in GRAD_NAMES}
    grads["grad.sampled"] = x.grad

    # no prompts: frozen and under no_grad (:523-525) -- nothing in front of the Transformer receives a gradient
    bare = build(dvae, dict(CFG, num_prompt_token=0))
    bare.train()
    x0 = sampled.clone().requires_grad_(True)
    ve_bare = bare.visual_embedding(x0, center)
    (ve_bare ** 2).sum().backward()
    bare_pre_grad_is_none = bare.proj_pre.weight.grad is None and x0.grad is None
    assert bare_pre_grad_is_none and bare.proj_post.bias.grad is not None

    MG.save("g23_clip", keys=np.array(keys), keys_noprompt=np.array(list(bare.state_dict().keys())), sampled=sampled, center=center,
            ve_eval=ve_eval, ve_train=ve_train, **{"mask.prompt.0": recorded[0]}, **grads, ve_noprompt=ve_bare,
            noprompt_proj_pre_grad_is_none=np.array(bare_pre_grad_is_none), **{"grad_noprompt.proj_post.bias": bare.proj_post.bias.grad})


if __name__ == "__main__":
    main()
