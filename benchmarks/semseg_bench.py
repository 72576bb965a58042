#!/usr/bin/env python3
"""S3DIS semantic-segmentation training step at B = 32, N = 2048 (act_amd/models/semseg.py): one JSON line.

    python benchmarks/semseg_bench.py [--batch 32] [--npoint 2048] [--steps 20] [--warmup 5]

Reports ms per training step and clouds/s for the per-group first propagation conv (default) and the plain form (ACT_SEG_FP_PERGROUP=0),
per-phase event times of the default form (group+tokenise, encoder, propagation, head, loss, backward, optimizer), the FLOP per step of both
formulations with TFLOP/s against the 157.3 TFLOP/s f32 MFMA peak, and the three_nn / interp_rows kernel times against their byte models.
A training step is what runner_semseg does: device augmentation, forward, weighted NLL, backward, AdamW step, clipping, AdamW step.
FLOP counts are computed from the shapes (training = 3 x forward, an estimate); times are device events.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TFLOPS = 157.3           # f32 MFMA, MI355X
PEAK_TBS = 8.0                # HBM


def flops_forward(B, N, G=128, M=32, D=384, depth=12, ncls=13):
    """multiply-adds x 2 of the forward, per step: (mini-PointNet + blocks, head reference form, head per-group form)"""
    r = G * M
    pointnet = 2 * r * (3 * 128 + 128 * 256 + 512 * 512 + 512 * D)
    blocks = depth * (2 * G * D * 3 * D + 4 * G * G * D + 2 * G * D * D + 4 * G * D * 4 * D) + 2 * G * (3 * 128 + 128 * D)
    conv2 = 2 * N * 1536 * 1024
    tail = 2 * N * (512 * 256 + 256 * ncls)
    head_ref = 2 * N * 1155 * 1536 + 2 * N * 3 * 1152 + conv2 + 2 * N * 3328 * 512 + tail
    head_pg = 2 * G * 1152 * 1536 + 2 * N * 6 * 1536 + conv2 + 2 * N * 1024 * 512 + 2 * 2304 * 512 + tail
    return B * (pointnet + blocks), B * head_ref, B * head_pg


def ev():
    return torch.cuda.Event(enable_timing=True)


def build(B, N, dev):
    from act_amd.models.semseg import get_model, get_loss
    from act_amd.tools.builder import FusedAdamW
    from act_amd.tools.runner_semseg import add_weight_decay
    torch.manual_seed(0)
    model = get_model(13).to(dev).train()
    opt = FusedAdamW(add_weight_decay(model, 0.05), lr=2e-4, weight_decay=0.05, fused=True)
    g = torch.Generator(device="cpu").manual_seed(0)
    pts = (torch.rand(B, N, 3, generator=g) * torch.tensor([1.0, 1.0, 3.0]) - torch.tensor([0.5, 0.5, 0.0])).to(dev)
    tgt = torch.randint(0, 13, (B * N,), generator=g).to(dev)
    w = (1 + torch.rand(13, generator=g)).to(dev)
    return model, get_loss(), opt, pts, tgt, w


def step(model, crit, opt, pts, tgt, w, pergroup, marks=None):
    from act_amd import kernels as K
    from act_amd.datasets.data_transforms import PointcloudScaleAndTranslate
    B, N, _ = pts.shape
    mark = (lambda i: marks[i].record()) if marks is not None else (lambda i: None)
    mark(0)
    x = pts.clone()
    scale = torch.empty(B, 1, device=x.device).uniform_(0.8, 1.25).expand(B, 3)
    PointcloudScaleAndTranslate(0.8, 1.25, 0.1)(x, scale=scale)
    # model.forward, split at the phase boundaries
    nb, center = model.group_divider(x)
    tokens = model.encoder(nb)
    pe = model.pos_embed
    pos = K.mlp(center, pe[0].weight, pe[0].bias, pe[2].weight, pe[2].bias)
    mark(1)
    from act_amd.models.act import stack_gates
    blocks = model.blocks.blocks
    gates = stack_gates(blocks, B, x.device, None, model.blocks.__dict__.setdefault("_keep_cache", {}))
    taps = K.block_stack(blocks, tokens, pos, gates, None, "enc", chunk=4, taps=True)
    f = torch.cat([K.layer_norm(t, model.norm.weight, model.norm.bias, model.norm.eps) for t in taps], dim=-1).reshape(B * 128, -1)
    mark(2)
    f0 = model.propagation_0_cls(x, center, f, pergroup=pergroup)
    mark(3)
    G = 128
    glob = torch.cat((K.group_max(f, G), K.group_mean(f, G)), dim=1)
    w1 = model.convs1_cls.weight.view(512, -1)
    gg = K.linear(glob, w1[:, 1024:], model.convs1_cls.bias)
    h = K.batch_norm_act(K.linear_group_add(f0, w1[:, :1024], gg, N), model.bns1_cls, True, relu=True)
    h = model._dropout(h, None)
    h = K.batch_norm_act(K.linear(h, model.convs2_cls.weight.view(256, 512), model.convs2_cls.bias), model.bns2_cls, True, relu=True)
    logp = K.log_softmax(K.linear(h, model.convs3_cls.weight.view(13, 256), model.convs3_cls.bias)).view(B, N, 13)
    mark(4)
    loss = crit(logp, tgt, w)
    mark(5)
    loss.backward()
    mark(6)
    opt.step()
    torch.nn.utils.clip_grad_norm_(model.parameters(), 10, norm_type=2)
    opt.step()
    model.zero_grad(set_to_none=True)
    mark(7)
    return loss


def time_steps(args, dev, pergroup):
    model, crit, opt, pts, tgt, w = build(args.batch, args.npoint, dev)
    for _ in range(args.warmup):
        step(model, crit, opt, pts, tgt, w, pergroup)
    torch.cuda.synchronize()
    a, b = ev(), ev()
    a.record()
    for _ in range(args.steps):
        step(model, crit, opt, pts, tgt, w, pergroup)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / args.steps
    phases = None
    if pergroup:
        names = ["group_tokenise", "encoder", "propagation", "head", "loss", "backward", "optimizer"]
        acc = [0.0] * len(names)
        for _ in range(args.steps):
            marks = [ev() for _ in range(8)]
            step(model, crit, opt, pts, tgt, w, pergroup, marks)
            torch.cuda.synchronize()
            for i in range(len(names)):
                acc[i] += marks[i].elapsed_time(marks[i + 1])
        phases = {n: round(v / args.steps, 3) for n, v in zip(names, acc)}
    del model, opt
    torch.cuda.empty_cache()
    return ms, phases


def kernel_times(args, dev, reps=50):
    from act_amd import kernels as K
    B, N, G, C = args.batch, args.npoint, 128, 1536
    g = torch.Generator(device="cpu").manual_seed(1)
    xyz = torch.rand(B, N, 3, generator=g).to(dev)
    ctr = xyz[:, torch.randperm(N, generator=g)[:G]].contiguous()
    P = torch.randn(B * G, C, generator=g).to(dev)
    dY = torch.randn(B * N, C, generator=g).to(dev)

    def timed(fn):
        for _ in range(5):
            fn()
        a, b = ev(), ev()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3                            # us
    nn3 = K.three_nn(xyz, ctr)
    t_nn = timed(lambda: K.three_nn(xyz, ctr, want_adj=False))
    t_nn_adj = timed(lambda: K.three_nn(xyz, ctr)) - t_nn
    t_fwd = timed(lambda: K.interp_rows_fwd(P, nn3[0], nn3[1], B, N, G))
    t_bwd = timed(lambda: K.interp_rows_bwd(dY, nn3[2], nn3[3], nn3[1], B, N, G))
    by_nn = 4.0 * (B * N * 3 + B * G * 3 + B * N * 6)
    by_adj = 4.0 * (B * N * 3 + B * (G + 1) + B * N * 3)
    by_fwd = 4.0 * (B * G * C + B * N * 6 + B * N * C)                 # unique bytes: P once (re-reads hit the caches), idx / w, Y
    by_bwd = 4.0 * (B * N * C + B * N * 6 + B * G * C)

    def row(us, by):
        return {"us": round(us, 2), "model_bytes": int(by), "GBps": round(by / us * 1e-3, 1), "frac_of_hbm_peak": round(by / us * 1e-6 / PEAK_TBS, 3)}
    return {"three_nn": row(t_nn, by_nn), "three_nn_adjacency": row(t_nn_adj, by_adj), "interp_rows_fwd_C1536": row(t_fwd, by_fwd),
            "interp_rows_bwd_C1536": row(t_bwd, by_bwd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--npoint", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    import __graft_entry__
    __graft_entry__.build()
    ms_pg, phases = time_steps(args, dev, True)
    ms_plain, _ = time_steps(args, dev, False)
    base, head_ref, head_pg = flops_forward(args.batch, args.npoint)
    f_ref, f_pg = 3 * (base + head_ref), 3 * (base + head_pg)
    out = {
        "workload": "semseg_train_step", "batch": args.batch, "npoint": args.npoint, "steps": args.steps,
        "ms_per_step": round(ms_pg, 3), "clouds_per_s": round(args.batch / ms_pg * 1e3, 1),
        "ms_per_step_plain_fp": round(ms_plain, 3), "clouds_per_s_plain_fp": round(args.batch / ms_plain * 1e3, 1),
        "phases_ms": phases,
        "gflop_fwd_per_cloud": {"pointnet_and_blocks": round(base / args.batch / 1e9, 2), "head_plain": round(head_ref / args.batch / 1e9, 2),
                                "head_pergroup": round(head_pg / args.batch / 1e9, 2)},
        "gflop_step_estimate_3x_fwd": {"plain": round(f_ref / 1e9, 1), "pergroup": round(f_pg / 1e9, 1)},
        "tflops": {"pergroup": round(f_pg / ms_pg * 1e-9, 2), "plain": round(f_ref / ms_plain * 1e-9, 2)},
        "frac_of_f32_mfma_peak": {"pergroup": round(f_pg / ms_pg * 1e-9 / PEAK_TFLOPS, 3), "plain": round(f_ref / ms_plain * 1e-9 / PEAK_TFLOPS, 3)},
        "kernels": kernel_times(args, dev),
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
