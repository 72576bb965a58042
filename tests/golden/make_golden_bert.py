#!/usr/bin/env python3
"""Generate tests/golden/g21_bert.npz from the REFERENCE'S OWN ACTPromptedDiscreteVAEwithBERT (models/dvae.py:617-857), on the CPU, with the import
shims of make_golden.py (timm, pointnet2_ops, knn_cuda, Chamfer, .cuda()) and ``transformers`` as installed.

Nothing is downloaded: ``transformers.BertModel.from_pretrained`` is REPLACED, before the class is built, by a function that returns a randomly
initialised 2-layer BertModel (hidden 64, 2 heads, intermediate 256, eager attention so that its probability dropout goes through
``torch.nn.functional.dropout``); the patch is asserted to be in place.  Parameters are then filled by name (fill.py): no weights are stored.
During the train-mode pass ``torch.nn.functional.dropout`` is a recording version, so the stored uint8 masks are the reference's own draws in call order
(prompt dropout, then attention / hidden / hidden per layer).

Geometry: B = 2, G = 16, Pn = 4 -> S = 20 tokens (no multiple of 16), head dimension 32.

Run:  python tests/golden/make_golden_bert.py      (build container only: the reference never travels)
"""
import os
import sys
import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
from fill import fill_module, fill_tensor, clouds  # noqa: E402

B, G, PN, D, HEADS, DEPTH, INTER, N = 2, 16, 4, 64, 2, 2, 256, 128
CFG = dict(NAME="ACTPromptedDiscreteVAEwithBERT", group_size=8, num_group=G, num_tokens=64, encoder_dims=64, tokens_dims=64, decoder_dims=64,
           visual_embed_type="bert-base-uncased", visual_embed_dim=D, freeze_visual_embed=True, num_prompt_token=PN, use_deep_prompt=False)
GRAD_NAMES = ["visual_prompt_token", "visual_prompt_pos", "proj_pre.weight", "visual_pos_embed.0.weight", "proj_post.bias"]


def main():
    import transformers                                   # before the shims: its import probes the real packages (a stub timm has no __spec__)
    from transformers import BertConfig, BertModel
    os.chdir(MG.REF)
    MG.install_shims()
    MG.STUB_VIT.update(dim=768)

    def tiny_bert(*args, **kwargs):
        return BertModel(BertConfig(hidden_size=D, num_hidden_layers=DEPTH, num_attention_heads=HEADS, intermediate_size=INTER,
                                    attn_implementation="eager"))
    BertModel.from_pretrained = tiny_bert
    assert transformers.BertModel.from_pretrained is tiny_bert, "from_pretrained must never run unpatched (it would reach for the network)"
    import models.dvae as dvae
    from easydict import EasyDict
    torch.set_num_threads(8)
    torch.manual_seed(0)
    model = dvae.ACTPromptedDiscreteVAEwithBERT(EasyDict(CFG))
    fill_module(model, "g21.")
    keys = list(model.state_dict().keys())

    sampled = fill_tensor("g21.in.sampled", (B, G, 64), "code")
    center = torch.from_numpy(clouds(21, B, G))

    model.eval()
    with torch.no_grad():
        ve_eval = model.visual_embedding(sampled, center)

    # train mode: record every dropout draw
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
        torch.manual_seed(21)
        ve_train = model.visual_embedding(x, center)
    finally:
        F.dropout = real_dropout
    (ve_train ** 2).sum().backward()
    S = PN + G
    want = [(B, PN, D)] + [(B, HEADS, S, S), (B, S, D), (B, S, D)] * DEPTH
    assert [tuple(m.shape) for m in recorded] == want, [tuple(m.shape) for m in recorded]
    names = ["prompt.0"] + [f"bert.{i}.{k}" for i in range(DEPTH) for k in ("attn", "hidden1", "hidden2")]
    pd = dict(model.named_parameters())
    assert all(p.grad is None for n, p in pd.items() if n.startswith("visual_embed."))
    grads = {"grad." + n: pd[n].grad for n in GRAD_NAMES}
    grads["grad.sampled"] = x.grad

    # full forward + get_loss, eval mode, seeded gumbel noise (torch.manual_seed(777), as the other goldens)
    model.eval()
    model.zero_grad()
    pts = torch.from_numpy(clouds(21, B, N))
    real_gs = F.gumbel_softmax

    def seeded_gumbel(logits, tau=1.0, hard=False, eps=1e-10, dim=-1):
        torch.manual_seed(777)
        return real_gs(logits, tau=tau, hard=hard, dim=dim)
    F.gumbel_softmax = seeded_gumbel
    try:
        with torch.no_grad():
            ret = model(pts, temperature=1.0, hard=False)
            lr, lk = model.get_loss(ret, pts)
    finally:
        F.gumbel_softmax = real_gs
    MG.save("g21_bert", keys=np.array(keys), sampled=sampled, center=center, ve_eval=ve_eval, ve_train=ve_train,
            mask_names=np.array(names), **{"mask." + n: m for n, m in zip(names, recorded)}, **grads,
            pts=pts, coarse=ret[2], fine=ret[3], logits=ret[5], loss=np.array([lr.item(), lk.item()], dtype=np.float64))


if __name__ == "__main__":
    main()
