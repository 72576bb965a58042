#!/usr/bin/env python3
"""ShapeNetPart part-segmentation training step and evaluation (act_amd/models/partseg.py): one JSON line.

    python benchmarks/partseg_bench.py [--batches 16,32] [--npoint 2048] [--steps 20] [--warmup 5]

Reports, per batch size (16 is the reference's default), ms per training step and clouds/s, with per-phase event times (group+tokenise, encoder,
label branch, propagation, head, loss, backward, optimizer); the label-branch and part-evaluation kernel times against their byte models; and the
evaluation time per test batch at B = 16: the device path (kernels.partseg_eval into the evaluation's buffers) against the reference's host form
(copy the [B, N, 50] log-probs to the host, masked arg-max and per-shape IoU loop in numpy, main.py:253-283) on the same log-probs.
A training step is what runner_partseg does: device augmentation, forward, NLL, backward, AdamW step, clipping, AdamW step.  Times are device
events (the host form: wall clock around a synchronised copy and the numpy loop).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TBS = 8.0                # HBM


def ev():
    return torch.cuda.Event(enable_timing=True)


def build(B, N, dev):
    from act_amd.models.partseg import get_model, get_loss, to_categorical
    from act_amd.tools.builder import FusedAdamW
    from act_amd.tools.runner_semseg import add_weight_decay
    torch.manual_seed(0)
    model = get_model(50).to(dev).train()
    opt = FusedAdamW(add_weight_decay(model, 0.05), lr=2e-4, weight_decay=0.05, fused=True)
    g = torch.Generator(device="cpu").manual_seed(0)
    pts = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(dev)
    cat = torch.randint(0, 16, (B,), generator=g)
    cls = to_categorical(cat, 16).to(dev)
    tgt = torch.randint(0, 50, (B * N,), generator=g).to(dev)
    return model, get_loss(), opt, pts, cls, tgt


def step(model, crit, opt, pts, cls, tgt, marks=None):
    from act_amd import kernels as K
    from act_amd.datasets.data_transforms import PointcloudScaleAndTranslate
    from act_amd.models.act import stack_gates
    B, N, _ = pts.shape
    mark = (lambda i: marks[i].record()) if marks is not None else (lambda i: None)
    mark(0)
    x = pts.clone()
    scale = torch.empty(B, 1, device=x.device).uniform_(0.8, 1.25).expand(B, 3)
    PointcloudScaleAndTranslate(0.8, 1.25, 0.1)(x, scale=scale)
    nb, center = model.group_divider(x)
    tokens = model.encoder(nb)
    pe = model.pos_embed
    pos = K.mlp(center, pe[0].weight, pe[0].bias, pe[2].weight, pe[2].bias)
    mark(1)
    blocks = model.blocks.blocks
    gates = stack_gates(blocks, B, x.device, None, model.blocks.__dict__.setdefault("_keep_cache", {}))
    taps = K.block_stack(blocks, tokens, pos, gates, None, "enc", chunk=4, taps=True)
    f = torch.cat([K.layer_norm(t, model.norm.weight, model.norm.bias, model.norm.eps) for t in taps], dim=-1).reshape(B * 128, -1)
    mark(2)
    lc = model.label_conv_cls
    lab = K.label_branch(cls, lc[0], lc[1], lc[2], True)
    mark(3)
    f0 = model.propagation_0_cls(x, center, f)
    mark(4)
    G = 128
    glob = torch.cat((K.group_max(f, G), K.group_mean(f, G), lab), dim=1)
    w1 = model.convs1_cls.weight.view(512, -1)
    gg = K.linear(glob, w1[:, 1024:], model.convs1_cls.bias)
    h = K.batch_norm_act(K.linear_group_add(f0, w1[:, :1024], gg, N), model.bns1_cls, True, relu=True)
    h = model._dropout(h, None)
    h = K.batch_norm_act(K.linear(h, model.convs2_cls.weight.view(256, 512), model.convs2_cls.bias), model.bns2_cls, True, relu=True)
    logp = K.log_softmax(K.linear(h, model.convs3_cls.weight.view(50, 256), model.convs3_cls.bias)).view(B, N, 50)
    mark(5)
    loss = crit(logp, tgt)
    mark(6)
    loss.backward()
    mark(7)
    opt.step()
    torch.nn.utils.clip_grad_norm_(model.parameters(), 10, norm_type=2)
    opt.step()
    model.zero_grad(set_to_none=True)
    mark(8)
    return loss


def time_steps(B, args, dev):
    model, crit, opt, pts, cls, tgt = build(B, args.npoint, dev)
    for _ in range(args.warmup):
        step(model, crit, opt, pts, cls, tgt)
    torch.cuda.synchronize()
    a, b = ev(), ev()
    a.record()
    for _ in range(args.steps):
        step(model, crit, opt, pts, cls, tgt)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / args.steps
    names = ["group_tokenise", "encoder", "label_branch", "propagation", "head", "loss", "backward", "optimizer"]
    acc = [0.0] * len(names)
    for _ in range(args.steps):
        marks = [ev() for _ in range(len(names) + 1)]
        step(model, crit, opt, pts, cls, tgt, marks)
        torch.cuda.synchronize()
        for i in range(len(names)):
            acc[i] += marks[i].elapsed_time(marks[i + 1])
    del model, opt
    torch.cuda.empty_cache()
    return {"ms_per_step": round(ms, 3), "clouds_per_s": round(B / ms * 1e3, 1), "phases_ms": {n: round(v / args.steps, 3) for n, v in zip(names, acc)}}


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    a, b = ev(), ev()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3                                # us


def row(us, by):
    return {"us": round(us, 2), "model_bytes": int(by), "GBps": round(by / us * 1e-3, 1), "frac_of_hbm_peak": round(by / us * 1e-6 / PEAK_TBS, 4)}


def host_eval(logp_dev, target_np, seg_classes, seg_label_to_cat):
    """main.py:253-283 on one batch: copy the log-probs to the host, masked arg-max per shape, per-shape part IoUs in Python"""
    cur = logp_dev.cpu().numpy()
    B, N, _ = cur.shape
    pred = np.zeros((B, N), np.int32)
    for i in range(B):
        cat = seg_label_to_cat[target_np[i, 0]]
        pred[i] = np.argmax(cur[i][:, seg_classes[cat]], 1) + seg_classes[cat][0]
    seen = [np.sum(target_np == l) for l in range(50)]
    corr = [np.sum((pred == l) & (target_np == l)) for l in range(50)]
    ious = []
    for i in range(B):
        segp, segl = pred[i], target_np[i]
        cat = seg_label_to_cat[segl[0]]
        part = []
        for l in seg_classes[cat]:
            if np.sum(segl == l) == 0 and np.sum(segp == l) == 0:
                part.append(1.0)
            else:
                part.append(np.sum((segl == l) & (segp == l)) / float(np.sum((segl == l) | (segp == l))))
        ious.append(np.mean(part))
    return pred, seen, corr, ious


def kernel_times(dev, N):
    from act_amd import kernels as K
    from act_amd.datasets.ShapeNetPartDataset import seg_classes, seg_label_to_cat, CATEGORIES
    out = {}
    g = torch.Generator(device="cpu").manual_seed(1)
    for B in (16, 32):
        lc = torch.nn.Sequential(torch.nn.Conv1d(16, 64, 1, bias=False), torch.nn.BatchNorm1d(64), torch.nn.LeakyReLU(0.2)).to(dev)
        cls = torch.eye(16)[torch.randint(0, 16, (B,), generator=g)].to(dev)
        dy = torch.randn(B, 64, generator=g).to(dev)
        W = lc[0].weight.view(64, 16)
        outs = [torch.empty(64, 16, device=dev), torch.empty(64, device=dev), torch.empty(64, device=dev)]
        by_lb = 4.0 * (B * 16 + 64 * 16 + B * 64 + 6 * 64)
        t_f = timed(lambda: K.LabelBranchFn.apply(cls, W, lc[1].weight, lc[1].bias, lc[1].running_mean, lc[1].running_var, True, 0.1, 1e-5, 0.2))
        t_b = timed(lambda: K.lib.act_label_branch_bwd_f32(K.ptr(cls), K.ptr(W), K.ptr(lc[1].weight), K.ptr(lc[1].bias), K.ptr(dy), B, 1e-5, 0.2,
                                                           K.ptr(outs[0]), K.ptr(outs[1]), K.ptr(outs[2]), K.stream()))
        out[f"label_branch_fwd_B{B}"] = row(t_f, by_lb)
        out[f"label_branch_bwd_B{B}"] = row(t_b, by_lb + 4.0 * 64 * 16 - 4.0 * 2 * 64)
        cat = torch.randint(0, 16, (B,), generator=g)
        tgt = torch.stack([torch.randint(int(seg_classes[CATEGORIES[c]][0]), int(seg_classes[CATEGORIES[c]][-1]) + 1, (N,), generator=g) for c in cat])
        logp = torch.log_softmax(torch.randn(B, N, 50, generator=g), -1).to(dev)
        tgt_d = tgt.to(dev)
        counts = torch.zeros(B, K.PART_COUNT_STRIDE, dtype=torch.int32, device=dev)
        seen = torch.zeros(50, dtype=torch.int64, device=dev)
        corr = torch.zeros(50, dtype=torch.int64, device=dev)
        t_e = timed(lambda: K.partseg_eval(logp, tgt_d, counts, seen, corr, 0))
        out[f"part_eval_B{B}"] = row(t_e, 4.0 * B * N * 50 + 8.0 * B * N)
        if B == 16:
            tn = tgt.numpy()
            host_eval(logp, tn, seg_classes, seg_label_to_cat)
            reps = 5
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                host_eval(logp, tn, seg_classes, seg_label_to_cat)
            t_host = (time.perf_counter() - t0) / reps * 1e3
            out["eval_per_test_batch_B16"] = {"device_ms": round(t_e * 1e-3, 4), "reference_host_form_ms": round(t_host, 3),
                                              "speedup": round(t_host / (t_e * 1e-3), 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=str, default="16,32")
    ap.add_argument("--npoint", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    import __graft_entry__
    __graft_entry__.build()
    out = {"workload": "partseg_train_step", "npoint": args.npoint, "steps": args.steps}
    for B in [int(b) for b in args.batches.split(",")]:
        out[f"B{B}"] = time_steps(B, args, dev)
    out["kernels"] = kernel_times(dev, args.npoint)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
