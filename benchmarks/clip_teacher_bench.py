#!/usr/bin/env python3
"""The CLIP image teacher (csrc/clip.hip, K.ClipBlockFn, visual_embed_type: clip:ViT-B/16): one JSON line.

    python benchmarks/clip_teacher_bench.py [--reps 5] [--inner 10] [--commit ID] [--out profiles/clip_teacher_bench.json]

Geometry B = 128, G = 64, Pn = 64 (S = 128 tokens), D = 768, 12 heads.  Reported, as medians of ``--reps`` with min and max (no time is a bar):
  * QuickGELU forward / backward per launch at 16,384 x 3,072 and its fraction of the HBM peak ``bench.py --full`` uses, against the compulsory bytes
    (8 per element forward: read pre, write out; 12 backward: read pre and dy, write dx);
  * the price of QuickGELU as its own pass: c_fc GEMM (EPI_NONE) + the pass, next to the fc1 GEMM with the GELU epilogue (which also writes the
    pre-activation) at the same 16,384 x 3,072 x 768 shape; and the two LayerNorm forwards of a block (with and without pos) for scale;
  * one 12-layer teacher forward (visual_embedding under no_grad, train mode) of the CLIP recipe next to the SHALLOW ViT recipe
    (cfgs/synthetic/act_dvae_with_pretrained_transformer.yaml with use_deep_prompt: False) at the same geometry;
  * a Stage-I step of the synthetic CLIP recipe next to that shallow ViT recipe.
The shallow ViT side runs on the parent commit as well (nothing of it is changed here): ``--only vit`` measures it alone there.
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
    ap.add_argument("--only", choices=("all", "vit"), default="all", help="vit: the shallow ViT yardstick alone (runs on a commit without the CLIP teacher)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_teacher_bench.json"))
    args = ap.parse_args()
    args.out = os.path.abspath(args.out)                 # the recipes are read relative to act_amd/, below
    import act_amd.kernels as K
    from act_amd.models import build_model_from_cfg
    from act_amd.utils.config import cfg_from_yaml_file, EasyDict
    from act_amd.tools import builder, runner_autoencoder as RA
    from act_amd.tools.runner_pretrain import _Single
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, G, Pn, D, H = 128, 64, 64, 768, 12
    S = G + Pn
    T, N = B * S, 4 * D
    med = statistics.median
    res = {"bench": "clip_teacher", "commit": args.commit, "device": torch.cuda.get_device_name(0), "geometry": dict(B=B, G=G, Pn=Pn, D=D, H=H, S=S)}

    if args.only == "all":
        # (a) QuickGELU as a streaming pass
        pre, dy = torch.randn(T, N, device=dev), torch.randn(T, N, device=dev)
        out = torch.empty_like(pre)
        f = event_ms(lambda: K.quickgelu_fwd(pre, out=out), args.reps, args.inner)
        b = event_ms(lambda: K.quickgelu_bwd(pre, dy, out=out), args.reps, args.inner)
        res["quickgelu"] = {"rows": T, "cols": N, "fwd_ms": spread(f), "bwd_ms": spread(b), "fwd_bytes": 8 * T * N, "bwd_bytes": 12 * T * N,
                            "fwd_hbm_frac": round(8.0 * T * N / (med(f) * 1e-3) / (PEAK_HBM_GBS * 1e9), 3),
                            "bwd_hbm_frac": round(12.0 * T * N / (med(b) * 1e-3) / (PEAK_HBM_GBS * 1e9), 3)}
        # (b) what the separate pass costs next to the fused GELU epilogue, and the two LayerNorms of a block for scale
        x, w, bias = torch.randn(T, D, device=dev), torch.randn(N, D, device=dev) / D ** 0.5, 0.05 * torch.randn(N, device=dev)
        pos, gamma, beta = torch.randn(T, D, device=dev), 1 + 0.1 * torch.randn(D, device=dev), 0.05 * torch.randn(D, device=dev)
        hpre = torch.empty(T, N, device=dev)

        def clip_fc():
            K.quickgelu_fwd(K.gemm(x, w, True, True, bias=bias, act=K.EPI_NONE, out=hpre), out=out)
        plain = event_ms(lambda: K.gemm(x, w, True, True, bias=bias, act=K.EPI_NONE, out=hpre), args.reps, args.inner)
        split = event_ms(clip_fc, args.reps, args.inner)
        fused = event_ms(lambda: K.gemm(x, w, True, True, bias=bias, act=K.EPI_GELU, aux=hpre, out=out), args.reps, args.inner)
        ln1 = event_ms(lambda: K.layernorm_fwd(x, pos, gamma, beta, 1e-5), args.reps, args.inner)
        ln2 = event_ms(lambda: K.layernorm_fwd(x, None, gamma, beta, 1e-5), args.reps, args.inner)
        extra = med(split) - med(fused)
        res["c_fc"] = {"M": T, "N": N, "K": D, "gemm_epi_none_ms": spread(plain), "gemm_plus_quickgelu_ms": spread(split),
                       "gemm_gelu_epilogue_with_aux_ms": spread(fused), "extra_pass_ms": round(extra, 4),
                       "layernorm_fwd_with_pos_ms": spread(ln1), "layernorm_fwd_ms": spread(ln2),
                       "extra_pass_over_two_layernorms": round(extra / (med(ln1) + med(ln2)), 2)}
        del pre, dy, out, x, w, hpre, pos
        torch.cuda.empty_cache()

    # 12-layer teacher forward under no_grad, and the Stage-I step: CLIP recipe against the shallow ViT recipe
    os.chdir(os.path.join(ROOT, "act_amd"))
    opt_cfg = dict(optimizer=dict(type="AdamW", kwargs=dict(lr=5e-4, weight_decay=5e-4)),
                   scheduler=dict(type="CosLR", kwargs=dict(epochs=300, initial_epochs=10)), step_per_update=1,
                   temp=dict(start=1, target=0.0625, ntime=100000), kldweight=dict(start=0, target=0.1, ntime=100000))
    pts = torch.randn(B, 1024, 3, device=dev)
    recipes = [("vit_shallow", "cfgs/synthetic/act_dvae_with_pretrained_transformer.yaml")]
    if args.only == "all":
        recipes.insert(0, ("clip", "cfgs/synthetic/act_dvae_with_pretrained_clip.yaml"))
    for name, path in recipes:
        mcfg = cfg_from_yaml_file(path).model
        mcfg.use_deep_prompt = False
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = build_model_from_cfg(mcfg).to(dev).train()
        sampled, center = torch.randn(B, G, model.tokens_dims, device=dev), torch.rand(B, G, 3, device=dev)

        def teacher():
            with torch.no_grad():
                model.visual_embedding(sampled, center, None, None)
        res["teacher_forward_ms_" + name] = spread(event_ms(teacher, args.reps, 2))
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
    if args.only == "all":
        res["teacher_forward_ratio"] = round(res["teacher_forward_ms_clip"]["median"] / res["teacher_forward_ms_vit_shallow"]["median"], 3)
        res["stage1_step_ratio"] = round(res["stage1_step_ms_clip"]["median"] / res["stage1_step_ms_vit_shallow"]["median"], 3)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
