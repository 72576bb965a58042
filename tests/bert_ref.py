"""Plain-torch CPU restatement of the language teacher's Transformer: one post-LayerNorm BERT layer and ``visual_embedding`` of
ACTPromptedDiscreteVAEwithBERT (reference models/dvae.py:738-777 over transformers' BertLayer), with every dropout keep mask injectable.

Test infrastructure (the role of tests/svm_ref.py and tests/tsne_ref.py): the GPU machine has neither the reference nor necessarily
``transformers``, so the GPU tests compare against this file and tests/golden/g21_bert.npz; tests/test_bert_host.py pins this file to the golden.

Parameters are read from a ``state_dict``-like mapping by the reference's key names.  Masks: a dict with the ``Draws`` keys ``prompt.0`` [B,Pn,D],
``bert.{i}.attn`` [B,H,S,S], ``bert.{i}.hidden1`` / ``bert.{i}.hidden2`` [B,S,D] (0/1, any dtype); a missing key means "no dropout there"."""
import torch
import torch.nn.functional as F

# the golden geometry (tests/golden/make_golden_bert.py): B = 2, G = 16, Pn = 4 -> S = 20, two layers, head dimension 32
TINY_BERT = dict(NAME="ACTPromptedDiscreteVAEwithBERT", group_size=8, num_group=16, num_tokens=64, encoder_dims=64, tokens_dims=64, decoder_dims=64,
                 visual_embed_type="bert-base-uncased", visual_embed_dim=64, freeze_visual_embed=True, num_prompt_token=4, use_deep_prompt=False,
                 visual_embed_depth=2, visual_embed_heads=2, visual_embed_intermediate=256)
GRAD_NAMES = ("visual_prompt_token", "visual_prompt_pos", "proj_pre.weight", "visual_pos_embed.0.weight", "proj_post.bias")

P_DROP = 0.1          # prompt_dropout, attention_probs_dropout_prob and hidden_dropout_prob of bert-base
EPS = 1e-12


def _drop(t, mask, p=P_DROP):
    return t if mask is None else t * mask.to(t.dtype) / (1.0 - p)


def bert_layer(x, sd, prefix, heads, m_attn=None, m_h1=None, m_h2=None, p=P_DROP, eps=EPS):
    """x [B,S,D] -> y [B,S,D]; sd[prefix + 'attention.self.query.weight'] etc."""
    B, S, D = x.shape
    hd = D // heads
    w = lambda n: sd[prefix + n].to(x.dtype)        # noqa: E731

    def lin(t, n):
        return t @ w(n + ".weight").t() + w(n + ".bias")
    q, k, v = (lin(x, "attention.self." + n).view(B, S, heads, hd).transpose(1, 2) for n in ("query", "key", "value"))
    probs = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1)
    ctx = (_drop(probs, m_attn, p) @ v).transpose(1, 2).reshape(B, S, D)
    a = F.layer_norm(_drop(lin(ctx, "attention.output.dense"), m_h1, p) + x, (D,), w("attention.output.LayerNorm.weight"),
                     w("attention.output.LayerNorm.bias"), eps)
    h = F.gelu(lin(a, "intermediate.dense"))
    return F.layer_norm(_drop(lin(h, "output.dense"), m_h2, p) + a, (D,), w("output.LayerNorm.weight"), w("output.LayerNorm.bias"), eps)


def visual_embedding(sampled, center, sd, heads, depth, num_prompt, masks=None):
    """sampled [B,G,tokens_dims], center [B,G,3] -> [B,G,tokens_dims]: proj_pre, + pos ONCE, prompts prepended once, the layers, prompts cut, proj_post"""
    masks = masks or {}
    w = lambda n: sd[n].to(sampled.dtype)           # noqa: E731
    pos = F.gelu(center @ w("visual_pos_embed.0.weight").t() + w("visual_pos_embed.0.bias")) @ w("visual_pos_embed.2.weight").t() + w("visual_pos_embed.2.bias")
    x = sampled @ w("proj_pre.weight").t() + w("proj_pre.bias") + pos
    B = x.shape[0]
    if num_prompt > 0:
        tok = _drop(w("visual_prompt_token").expand(B, -1, -1), masks.get("prompt.0"))
        x = torch.cat((tok + w("visual_prompt_pos").expand(B, -1, -1), x), dim=1)
    for i in range(depth):
        x = bert_layer(x, sd, f"visual_embed.0.layer.{i}.", heads, masks.get(f"bert.{i}.attn"), masks.get(f"bert.{i}.hidden1"),
                       masks.get(f"bert.{i}.hidden2"))
    x = x[:, num_prompt:]
    return x @ w("proj_post.weight").t() + w("proj_post.bias")
