#!/usr/bin/env python3
"""The DGCNN segmentation networks' two-layer EdgeConv (csrc/edge_mlp2.hip, models/dgcnn_nets.py): one JSON line.

    python benchmarks/dgcnn_seg_bench.py [--reps 10] [--commit ID] [--out FILE]        # FILE defaults to profiles/dgcnn_seg_bench.json

Device-event medians (with min / max) of ``--reps`` repetitions after a warm-up:
  * K.edge_mlp2_bn forward and forward + backward in train mode at (B x N, k, C1 -> C2) = (16 x 2,048, 40, 64 -> 64), (16 x 2,048, 40, 64 -> 128)
    and (16 x 4,096, 20, 64 -> 64), the per-point product pq = [P | Q] and the search excluded;
  * the same shapes through the composition of the ops the parent commit has -- the rows v = P[idx] + Q materialised (K.group_rows), then
    K.batch_norm_act(slope=0.2), K.linear, K.batch_norm_act(slope=0.2), K.group_max -- which writes and re-reads the [B*N*k, C] edge tensors.  The
    two are timed in the same process, ALTERNATING repetition by repetition, on the same inputs; their outputs are compared (the worst difference
    is reported, not asserted);
  * one training step (forward, loss, backward) of dgcnn_partseg(50) at 16 x 2,048, k = 40 and of dgcnn_semseg(13, in_channel=3) at 16 x 4,096,
    k = 20, the searches included.
The capability is new, so there is no earlier time of this project to compare with: ``--commit`` names the parent whose ops the composition uses.

Rate.  ``edge_product_flops_per_s`` is 2 * B*N*k * C1 * C2 over the fused FORWARD time: the per-edge product alone, the one thing the matrix
cores do in that time; notebook/dgcnn_seg.md sets it against the issue model of the tile loop.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from benchmarks.sa_bench import spread                           # noqa: E402

SHAPES = [(16, 2048, 40, 64, 64), (16, 2048, 40, 64, 128), (16, 4096, 20, 64, 64)]
SLOPE = 0.2


def timed_pair(f, g, reps):
    """f and g alternating, one device-event interval each per repetition, after one warm-up of both"""
    f(); g()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(reps):
        for fn, acc in ((f, out[0]), (g, out[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b))
    return out


def tail(B, N, k, C1, C2, reps, K, dev):
    g = torch.Generator(device="cpu").manual_seed(C1 + C2 + k)
    x = torch.randn(B, N, C1, generator=g).to(dev)
    idx = K.knn_features(x, k)
    pq = torch.randn(B * N, 2 * C1, generator=g).to(dev).requires_grad_(True)
    w2 = (torch.randn(C2, C1, generator=g) / C1 ** 0.5).to(dev).requires_grad_(True)
    bns = [torch.nn.BatchNorm2d(C1).to(dev).train(), torch.nn.BatchNorm2d(C2).to(dev).train(), torch.nn.BatchNorm1d(C1).to(dev).train(),
           torch.nn.BatchNorm1d(C2).to(dev).train()]

    def fused():
        return K.edge_mlp2_bn(pq, C1, idx, B, N, k, C1, bns[0], w2, bns[1], True, slope=SLOPE, validate=False)

    def composed():
        P, Q = pq[:, :C1], pq[:, C1:]
        v = K.group_rows(None, None, P.reshape(B, N, C1), idx, use_xyz=False).view(B * N, k, C1) + Q.reshape(B * N, 1, C1)
        h = K.batch_norm_act(v.reshape(B * N * k, C1), bns[2], True, slope=SLOPE)
        return K.group_max(K.batch_norm_act(K.linear(h, w2), bns[3], True, slope=SLOPE), k)

    def step(fn):
        def run():
            pq.grad = w2.grad = None
            for bn in bns:
                bn.zero_grad(set_to_none=True)
            fn().square().mean().backward()
        return run

    def fwd(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    with torch.no_grad():
        diff = float((fused() - composed()).abs().max())
    tf, tc = timed_pair(fwd(fused), fwd(composed), reps)
    sf, sc = timed_pair(step(fused), step(composed), reps)
    med = statistics.median
    return {"B": B, "N": N, "k": k, "C1": C1, "C2": C2, "fused_fwd_ms": spread(tf), "composed_fwd_ms": spread(tc), "fused_fwd_bwd_ms": spread(sf),
            "composed_fwd_bwd_ms": spread(sc), "composed_over_fused_fwd": round(med(tc) / med(tf), 2),
            "composed_over_fused_fwd_bwd": round(med(sc) / med(sf), 2), "max_abs_difference_of_the_outputs": float("%.3g" % diff),
            "edge_product_flops_per_s": float("%.4g" % (2.0 * B * N * k * C1 * C2 / (med(tf) * 1e-3)))}


def network(name, reps, K, M, dev):
    from benchmarks.sa_bench import timed
    g = torch.Generator(device="cpu").manual_seed(0)
    if name == "dgcnn_partseg":
        B, N, classes = 16, 2048, 50
        net = M.dgcnn_partseg(classes).to(dev).train()
        onehot = torch.zeros(B, 16)
        onehot[torch.arange(B), torch.randint(0, 16, (B,), generator=g)] = 1.0
        args = (torch.randn(B, 3, N, generator=g).to(dev), onehot.to(dev))
    else:
        B, N, classes = 16, 4096, 13
        net = M.dgcnn_semseg(classes, in_channel=3).to(dev).train()
        args = (torch.randn(B, 3, N, generator=g).to(dev),)
    lab = torch.randint(0, classes, (B * N,), generator=g).to(dev)

    def step():
        net.zero_grad(set_to_none=True)
        K.nll_weighted(net(*args).view(B * N, classes), lab)[0].backward()
    return {"B": B, "N": N, "k": net.k, "step_ms": spread(timed(step, reps), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "dgcnn_seg_bench.json"))
    ap.add_argument("--commit", type=str, default=os.environ.get("ACT_BENCH_COMMIT"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dgcnn_seg_bench needs a GPU: there is nothing to time without one")
    from act_amd import kernels as K
    from act_amd.models import dgcnn_nets as M
    dev = torch.device("cuda:0")
    res = {"workload": "dgcnn_segmentation", "parent_commit": args.commit, "reps": args.reps,
           "edge_mlp2": [tail(*s, args.reps, K, dev) for s in SHAPES],
           "dgcnn_partseg_step": network("dgcnn_partseg", args.reps, K, M, dev),
           "dgcnn_semseg_step": network("dgcnn_semseg", args.reps, K, M, dev)}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
