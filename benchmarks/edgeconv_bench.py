#!/usr/bin/env python3
"""The DGCNN classifier's kernels (csrc/edgeconv.hip, models/dgcnn_nets.py): one JSON line.

    python benchmarks/edgeconv_bench.py [--reps 10] [--commit ID] [--out FILE]        # FILE defaults to profiles/edgeconv_bench.json

Device-event medians (with min / max) of ``--reps`` repetitions after a warm-up, at the classifier's published sizes B = 32, N = 1,024, k = 20:
  * the feature-space search (K.knn_features) for the four layers' inputs, C = 3, 64, 64, 128, against torch.cdist + topk on the same device (the
    index sets are compared where cdist's expansion form leaves them comparable: the agreeing fraction is reported, not asserted);
  * one EdgeConv layer forward + backward (search excluded) for the four layer shapes (C -> out = 3 -> 64, 64 -> 64, 64 -> 128, 128 -> 256), against
    the composition of the ops that existed before: K.group_rows(use_xyz=False) + K.linear + K.batch_norm_act(relu=True) + K.group_max, which
    materialises the [B*N*k, 2C] and [B*N*k, out] edge tensors.  The composition is a TIMING stand-in (ReLU in place of LeakyReLU), not a parity
    target;
  * one training step (forward, loss, backward) of dgcnn_cls(40).
The capability is new, so there is no earlier time of this project to compare with.

Rate.  A distance term is one (query, candidate, channel) subtract-multiply-add.  ``terms_per_s`` is B * N * N * C over the search time;
notebook/edgeconv.md sets it against the vector-issue model of the kernel.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from benchmarks.sa_bench import spread, timed                    # noqa: E402

B, N, KNN = 32, 1024, 20
LAYERS = [(3, 64), (64, 64), (64, 128), (128, 256)]


def search(C, reps, K, dev):
    g = torch.Generator(device="cpu").manual_seed(C)
    x = torch.randn(B, N, C, generator=g).to(dev)
    idx = K.knn_features(x, KNN)
    ref = torch.cdist(x, x).topk(KNN, dim=-1, largest=False).indices
    same = float((idx.long().sort(-1).values == ref.sort(-1).values).all(-1).float().mean())
    t = timed(lambda: K.knn_features(x, KNN), reps)
    t_ref = timed(lambda: torch.cdist(x, x).topk(KNN, dim=-1, largest=False), reps)
    return {"B": B, "N": N, "C": C, "k": KNN, "knn_features_ms": spread(t), "cdist_topk_ms": spread(t_ref),
            "queries_with_the_same_index_set": round(same, 5), "speedup_over_cdist_topk": round(statistics.median(t_ref) / statistics.median(t), 2),
            "terms_per_s": float("%.4g" % (B * N * N * C / (statistics.median(t) * 1e-3)))}


def layer(C, out, reps, K, M, dev):
    g = torch.Generator(device="cpu").manual_seed(C + out)
    x = torch.randn(B, N, C, generator=g).to(dev).requires_grad_(C != 3)
    idx = K.knn_features(x, KNN)
    fused = M.EdgeConv(C, out, KNN).to(dev).train()
    conv = torch.nn.Conv2d(2 * C, out, 1, bias=False).to(dev)
    bn = torch.nn.BatchNorm1d(out).to(dev).train()
    centre = x.detach().reshape(B * N, 1, C)

    def fused_step():
        fused.zero_grad(set_to_none=True)
        x.grad = None
        fused(x, idx).square().mean().backward()

    def composed_step():
        conv.zero_grad(set_to_none=True); bn.zero_grad(set_to_none=True)
        x.grad = None
        nbr = K.group_rows(None, None, x, idx, use_xyz=False).view(B * N, KNN, C)
        rows = torch.cat((nbr - centre, centre.expand(B * N, KNN, C)), dim=2).reshape(B * N * KNN, 2 * C)
        h = K.batch_norm_act(K.linear(rows, conv.weight.view(out, 2 * C)), bn, True, relu=True)
        K.group_max(h, KNN).square().mean().backward()

    t, t_ref = timed(fused_step, reps), timed(composed_step, reps)
    return {"B": B, "N": N, "k": KNN, "C": C, "out": out, "fused_fwd_bwd_ms": spread(t), "composed_relu_stand_in_fwd_bwd_ms": spread(t_ref),
            "composed_over_fused": round(statistics.median(t_ref) / statistics.median(t), 2)}


def network(reps, K, M, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    net = M.dgcnn_cls(40).to(dev).train()
    pts = torch.randn(B, N, 3, generator=g).to(dev)
    lab = torch.randint(0, 40, (B,), generator=g).to(dev)

    def step():
        net.zero_grad(set_to_none=True)
        K.softmax_xent(net(pts), lab)[0].backward()
    return {"B": B, "N": N, "k": KNN, "step_ms": spread(timed(step, reps), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "edgeconv_bench.json"))
    ap.add_argument("--commit", type=str, default=os.environ.get("ACT_BENCH_COMMIT"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edgeconv_bench needs a GPU: there is nothing to time without one")
    from act_amd import kernels as K
    from act_amd.models import dgcnn_nets as M
    dev = torch.device("cuda:0")
    res = {"workload": "dgcnn_classifier", "commit": args.commit, "reps": args.reps,
           "search": [search(C, args.reps, K, dev) for C, _ in LAYERS],
           "edgeconv_layer": [layer(C, out, args.reps, K, M, dev) for C, out in LAYERS],
           "dgcnn_cls_step": network(args.reps, K, M, dev)}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
