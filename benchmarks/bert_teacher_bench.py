#!/usr/bin/env python3
"""The language teacher (csrc/bert.hip, ACTPromptedDiscreteVAEwithBERT): one JSON line.

    python benchmarks/bert_teacher_bench.py [--reps 5] [--inner 10] [--commit ID] [--out profiles/bert_teacher_bench.json]

Geometry B = 128, G = 64, Pn = 64 (S = 128 tokens), D = 768, 12 heads.  Reported, as medians of ``--reps`` with min and max (no time is a bar):
  * dropout + residual + LayerNorm forward / backward per launch at 16,384 x 768, and its fraction of the HBM peak ``bench.py --full`` uses
    (12 bytes per element forward, 16 backward);
  * the dropout attention (p = 0.1, Philox) forward / backward at S = 128, H = 12, hd = 64 next to act_attention_fwd_f32 / _bwd_f32 on the same
    tensors, and the ratios;
  * one 12-layer teacher forward (visual_embedding under no_grad) in train mode and in eval mode;
  * a Stage-I step of the synthetic BERT recipe next to the ViT recipe.
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_HBM_GBS = 8000.0               # the figure of bench.py --full


def spread(vals, digits=4):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def event_ms(fn, reps, inner):
    """per-call milliseconds of ``inner`` back-to-back calls between two events, ``reps`` times after a warm-up"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bert_teacher_bench.json"))
    args = ap.parse_args()
    import act_amd.kernels as K
    from act_amd.models import build_model_from_cfg
    from act_amd.utils.config import cfg_from_yaml_file, EasyDict
    from act_amd.tools import builder, runner_autoencoder as RA
    from act_amd.tools.runner_pretrain import _Single
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, G, Pn, D, H = 128, 64, 64, 768, 12
    S, hd = G + Pn, D // H
    T = B * S
    res = {"bench": "bert_teacher", "commit": args.commit, "device": torch.cuda.get_device_name(0), "geometry": dict(B=B, G=G, Pn=Pn, D=D, H=H, S=S)}

    # (a) dropout + residual + LayerNorm
    t, r, dy = (torch.randn(T, D, device=dev) for _ in range(3))
    gamma, beta = 1 + 0.1 * torch.randn(D, device=dev), 0.05 * torch.randn(D, device=dev)
    y, rstd = K.dropout_add_layernorm_fwd(t, r, gamma, beta, 1e-12, 0.1, 7)
    f = event_ms(lambda: K.dropout_add_layernorm_fwd(t, r, gamma, beta, 1e-12, 0.1, 7), args.reps, args.inner)
    b = event_ms(lambda: K.dropout_add_layernorm_bwd(dy, y, gamma, beta, rstd, 0.1, 7), args.reps, args.inner)
    res["dropout_ln"] = {"rows": T, "D": D, "fwd_ms": spread(f), "bwd_ms": spread(b),
                         "fwd_hbm_frac": round(12.0 * T * D / (statistics.median(f) * 1e-3) / (PEAK_HBM_GBS * 1e9), 3),
                         "bwd_hbm_frac": round(16.0 * T * D / (statistics.median(b) * 1e-3) / (PEAK_HBM_GBS * 1e9), 3)}
    del t, r, dy, y

    # (b) attention with and without dropout on the same tensors
    qkv, dout = torch.randn(B, S, 3, H, hd, device=dev), torch.randn(T, D, device=dev)
    out, lse = K.attention_dropout_fwd(qkv, B, S, H, hd, 0.1, 7)
    out0, lse0 = K.attention_fwd(qkv, B, S, H, hd)
    af = event_ms(lambda: K.attention_dropout_fwd(qkv, B, S, H, hd, 0.1, 7), args.reps, args.inner)
    ab = event_ms(lambda: K.attention_dropout_bwd(qkv, out, dout, lse, B, S, H, hd, 0.1, 7), args.reps, args.inner)
    f0 = event_ms(lambda: K.attention_fwd(qkv, B, S, H, hd), args.reps, args.inner)
    b0 = event_ms(lambda: K.attention_bwd(qkv, out0, dout, lse0, B, S, H, hd), args.reps, args.inner)
    res["attention"] = {"S": S, "H": H, "hd": hd, "p": 0.1, "dropout_fwd_ms": spread(af), "dropout_bwd_ms": spread(ab), "p0_fwd_ms": spread(f0),
                        "p0_bwd_ms": spread(b0), "fwd_ratio": round(statistics.median(af) / statistics.median(f0), 2),
                        "bwd_ratio": round(statistics.median(ab) / statistics.median(b0), 2)}
    del qkv, dout, out, out0

    # 12-layer teacher forward under no_grad, and the Stage-I step of both recipes
    os.chdir(os.path.join(ROOT, "act_amd"))
    opt_cfg = dict(optimizer=dict(type="AdamW", kwargs=dict(lr=5e-4, weight_decay=5e-4)),
                   scheduler=dict(type="CosLR", kwargs=dict(epochs=300, initial_epochs=10)), step_per_update=1,
                   temp=dict(start=1, target=0.0625, ntime=100000), kldweight=dict(start=0, target=0.1, ntime=100000))
    pts = torch.randn(B, 1024, 3, device=dev)
    for name, path in (("bert", "cfgs/synthetic/act_dvae_with_pretrained_bert.yaml"), ("vit", "cfgs/synthetic/act_dvae_with_pretrained_transformer.yaml")):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = build_model_from_cfg(cfg_from_yaml_file(path).model).to(dev).train()
        if name == "bert":
            sampled, center = torch.randn(B, G, model.tokens_dims, device=dev), torch.rand(B, G, 3, device=dev)

            def teacher():
                with torch.no_grad():
                    rng = model._rng(dev)
                    model.visual_embedding(sampled, center, None, rng)
                    rng[1].add_(1)
            res["teacher_forward_train_ms"] = spread(event_ms(teacher, args.reps, 2))
            model.eval()
            res["teacher_forward_eval_ms"] = spread(event_ms(teacher, args.reps, 2))
            model.train()
        wrapped = _Single(model)
        cfg = EasyDict(opt_cfg)
        opt, _ = builder.build_opti_sche(wrapped, cfg)
        step = [20000]

        def train():
            RA.train_step(wrapped, opt, pts, cfg, step[0])
            step[0] += 1
        res["stage1_step_ms_" + name] = spread(event_ms(train, args.reps, 2))
        del model, wrapped, opt
        torch.cuda.empty_cache()
    res["stage1_step_ratio"] = round(res["stage1_step_ms_bert"]["median"] / res["stage1_step_ms_vit"]["median"], 2)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
