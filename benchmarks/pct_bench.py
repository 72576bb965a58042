#!/usr/bin/env python3
"""PCT's offset attention (csrc/offset_attn.hip) and network (models/pct.py): one JSON line.

    python benchmarks/pct_bench.py [--reps 10] [--commit ID] [--out FILE]        # FILE defaults to profiles/pct_bench.json

Device-event medians (with min / max) of ``--reps`` repetitions after a warm-up:
  * K.offset_attention (x fused, the form the network uses) forward and forward + backward at (B, N, Dq, C) = (32, 256, 64, 256), the shipped
    shape, and (32, 1024, 64, 256), against the torch composition on the same device: bmm, softmax, sum, divide, bmm, which materialises four
    [B,N,N] tensors per direction;
  * one training step (forward, cross-entropy, backward) of pct(40) at 32 x 1,024, FPS and kNN included.
Fused and composed forms are timed in one process, ALTERNATING repetition by repetition, on the same inputs; the worst difference of their outputs
is reported, not asserted.  The capability is new, so there is no earlier time of this project to compare with: ``--commit`` names the parent.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from benchmarks.dgcnn_seg_bench import timed_pair                # noqa: E402
from benchmarks.sa_bench import spread, timed                    # noqa: E402

SHAPES = [(32, 256, 64, 256), (32, 1024, 64, 256)]


def _fwd(fn):
    def run():
        with torch.no_grad():
            fn()
    return run


def attention(B, N, Dq, C, reps, K, dev):
    g = torch.Generator(device="cpu").manual_seed(N + C)
    q = (torch.randn(B * N, Dq, generator=g) * Dq ** -0.25).to(dev).requires_grad_(True)
    v = torch.randn(B * N, C, generator=g).to(dev).requires_grad_(True)
    x = torch.randn(B * N, C, generator=g).to(dev).requires_grad_(True)
    cot = torch.randn(B * N, C, generator=g).to(dev)

    def fused():
        return K.offset_attention(q, q, v, B, N, x=x)

    def composed():
        qb, vb = q.view(B, N, Dq), v.view(B, N, C)
        attention = torch.softmax(torch.bmm(qb, qb.transpose(1, 2)), dim=-1)
        attention = attention / (1e-9 + attention.sum(dim=1, keepdim=True))
        return x - torch.bmm(attention.transpose(1, 2), vb).reshape(B * N, C)

    def step(fn):
        def run():
            q.grad = v.grad = x.grad = None
            fn().backward(cot)
        return run

    with torch.no_grad():
        diff = float((fused() - composed()).abs().max())
    tf, tc = timed_pair(_fwd(fused), _fwd(composed), reps)
    sf, sc = timed_pair(step(fused), step(composed), reps)
    med = statistics.median
    return {"B": B, "N": N, "Dq": Dq, "C": C, "fused_fwd_ms": spread(tf), "composed_fwd_ms": spread(tc), "fused_fwd_bwd_ms": spread(sf),
            "composed_fwd_bwd_ms": spread(sc), "composed_over_fused_fwd": round(med(tc) / med(tf), 2),
            "composed_over_fused_fwd_bwd": round(med(sc) / med(sf), 2), "max_abs_difference_of_the_outputs": float("%.3g" % diff),
            "composed_nn_bytes_per_direction": 4 * 4 * B * N * N}


def network(reps, K, dev):
    from act_amd.models.pct import pct
    B, N, classes = 32, 1024, 40
    g = torch.Generator(device="cpu").manual_seed(0)
    net = pct(classes).to(dev).train()
    pts = torch.rand(B, N, 3, generator=g).to(dev)
    lab = torch.randint(0, classes, (B,), generator=g).to(dev)

    def step():
        net.zero_grad(set_to_none=True)
        K.softmax_xent(net(pts), lab)[0].backward()
    return {"B": B, "N": N, "parameters": sum(p.numel() for p in net.parameters()), "step_ms": spread(timed(step, reps), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "pct_bench.json"))
    ap.add_argument("--commit", type=str, default=os.environ.get("ACT_BENCH_COMMIT"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pct_bench needs a GPU: there is nothing to time without one")
    from act_amd import kernels as K
    dev = torch.device("cuda:0")
    res = {"workload": "pct", "parent_commit": args.commit, "reps": args.reps,
           "offset_attention": [attention(*s, args.reps, K, dev) for s in SHAPES],
           "pct_step": network(args.reps, K, dev)}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
