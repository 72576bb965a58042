"""Plain-torch CPU restatement of the CLIP image teacher's shallow path: one residual block of CLIP's visual Transformer and ``visual_embedding`` of
ACTPromptedDiscreteVAEwithVIT with ``visual_embed_type: clip:...`` (reference models/dvae.py:500-534 over CLIP's ResidualAttentionBlock), with the prompt
dropout's keep mask injectable.  It imports neither ``clip`` nor the reference.

Test infrastructure (the role of tests/bert_ref.py): the GPU machine has no reference, so the GPU tests compare against this file and
tests/golden/g23_clip.npz; tests/test_clip_host.py pins this file to the golden.

Parameters are read from a ``state_dict``-like mapping by the reference's key names.  Masks: a dict with the ``Draws`` key ``prompt.0`` [B,Pn,D] (0/1, any
dtype); a missing key means "no dropout"."""
import torch
import torch.nn.functional as F

# the golden geometry (tests/golden/make_golden_clip.py): B = 2, G = 16, Pn = 4 -> S = 20, two blocks, head dimension 32
TINY_CLIP = dict(NAME="ACTPromptedDiscreteVAEwithVIT", group_size=8, num_group=16, num_tokens=64, encoder_dims=64, tokens_dims=64, decoder_dims=64,
                 visual_embed_type="clip:ViT-B/16", visual_embed_dim=64, freeze_visual_embed=True, num_prompt_token=4, use_deep_prompt=False,
                 visual_embed_depth=2, visual_embed_heads=2)
GRAD_NAMES = ("visual_prompt_token", "visual_prompt_pos", "proj_pre.weight", "visual_pos_embed.0.weight", "proj_post.bias")
BLOCK_KEYS = ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "ln_1.weight", "ln_1.bias",
              "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias", "ln_2.weight", "ln_2.bias")

P_DROP = 0.1          # prompt_dropout
EPS = 1e-5            # CLIP's LayerNorm
ALPHA = 1.702         # QuickGELU


def quickgelu(x):
    return x * torch.sigmoid(ALPHA * x)


def clip_block(x, sd, prefix, heads, eps=EPS):
    """x [B,S,D] (batch first; the reference's permutes to sequence first are layout only) -> [B,S,D]; sd[prefix + 'attn.in_proj_weight'] etc."""
    B, S, D = x.shape
    hd = D // heads
    w = lambda n: sd[prefix + n].to(x.dtype)        # noqa: E731
    y = F.layer_norm(x, (D,), w("ln_1.weight"), w("ln_1.bias"), eps)
    qkv = (y @ w("attn.in_proj_weight").t() + w("attn.in_proj_bias")).view(B, S, 3, heads, hd)
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    probs = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1)
    ctx = (probs @ v).transpose(1, 2).reshape(B, S, D)
    x = x + ctx @ w("attn.out_proj.weight").t() + w("attn.out_proj.bias")
    y = F.layer_norm(x, (D,), w("ln_2.weight"), w("ln_2.bias"), eps)
    h = quickgelu(y @ w("mlp.c_fc.weight").t() + w("mlp.c_fc.bias"))
    return x + h @ w("mlp.c_proj.weight").t() + w("mlp.c_proj.bias")


def visual_embedding(sampled, center, sd, heads, depth, num_prompt, masks=None):
    """sampled [B,G,tokens_dims], center [B,G,3] -> [B,G,tokens_dims]: proj_pre, prompts prepended once, ln_pre (pos is not normalised),
    x = blk(x + pos) per block, ln_post, prompts cut, proj_post.  num_prompt == 0: the Transformer runs under no_grad (frozen teacher, :523-525)."""
    masks = masks or {}
    w = lambda n: sd[n].to(sampled.dtype)           # noqa: E731
    D = w("proj_pre.weight").shape[0]
    pos = F.gelu(center @ w("visual_pos_embed.0.weight").t() + w("visual_pos_embed.0.bias")) @ w("visual_pos_embed.2.weight").t() + w("visual_pos_embed.2.bias")
    x = sampled @ w("proj_pre.weight").t() + w("proj_pre.bias")
    B = x.shape[0]

    def tower(x, pos):
        x = F.layer_norm(x, (D,), w("visual_embed.0.weight"), w("visual_embed.0.bias"), EPS)
        for i in range(depth):
            x = clip_block(x + pos, sd, f"visual_embed.1.{i}.", heads)
        return F.layer_norm(x, (D,), w("visual_embed.2.weight"), w("visual_embed.2.bias"), EPS)
    if num_prompt > 0:
        m = masks.get("prompt.0")
        tok = w("visual_prompt_token").expand(B, -1, -1)
        tok = tok if m is None else tok * m.to(tok.dtype) / (1.0 - P_DROP)
        x = torch.cat((tok, x), dim=1)
        pos = torch.cat((w("visual_prompt_pos").expand(B, -1, -1), pos), dim=1)
        x = tower(x, pos)[:, num_prompt:]
    else:
        with torch.no_grad():
            x = tower(x, pos)
    return x @ w("proj_post.weight").t() + w("proj_post.bias")
