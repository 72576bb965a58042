#!/usr/bin/env python3
"""Isolated per-launch time of the split-f16 GEMM (csrc/gemm_bf16x3.hip) on each of its tiles, alternating, with device events, and torch.equal of the two
results at every shape; the column `rule` is what act_sgemm_nt_f16x3_pick_tile answers for the device's CU count.  usage: python benchmarks/x3_tiles_bench.py
-> profiles/x3_tiles_micro.txt"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import act_amd.kernels as K                      # noqa: E402
from act_amd.composite import f16x3_act_scale    # noqa: E402

ROUNDS, LAUNCHES = 5, 40
SHAPES = [(8192, 768, 768), (8192, 768, 3072), (8192, 2304, 768), (8192, 3072, 768),                       # the teacher's proj, fc2, qkv, fc1 at B = 128
          (16384, 768, 768), (16384, 768, 3072), (16384, 2304, 768), (16384, 3072, 768),                   # ... and at the stress geometry
          (128, 384, 64), (128, 384, 3072), (256, 384, 192), (1024, 768, 768), (2048, 768, 768), (4096, 768, 768), (4096, 768, 3072),
          (2048, 2304, 768), (4096, 2304, 768), (4096, 3072, 768), (8192, 384, 768), (8192, 1152, 768), (8192, 1536, 768), (12288, 768, 768), (6144, 768, 3072)]


def main():
    if not torch.cuda.is_available():
        raise SystemExit("x3_tiles_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    print(f"device CUs: {cus}")
    print(f"{'M':>6s} {'N':>5s} {'K':>5s}  {'us 128x128':>10s} {'us 128x192':>10s}  {'ratio':>6s}  rule  wg128 wg192  equal   "
          f"(median of {ROUNDS} rounds x {LAUNCHES} launches, min..max per round)")
    for M, N, Kd in SHAPES:
        g = torch.Generator().manual_seed(M + N + Kd)
        a = torch.randn(M, Kd, generator=g).to(dev)
        w = (0.05 * torch.randn(N, Kd, generator=g)).to(dev)
        s_a = f16x3_act_scale(a.abs().max().item())
        sb, inv = K.f16x3_row_scales(w)
        ap, bp = K.split_f16x2(a, s_a), K.split_f16x2(w, 1.0, sb)
        bias, res = torch.randn(N, generator=g).to(dev), torch.randn(M, N, generator=g).to(dev)
        outs = {t: torch.empty(M, N, device=dev) for t in (128, 192)}

        def launch(t):
            K.gemm_nt_f16x3(ap, s_a, bp, inv, bias=bias, res=res, out=outs[t], tile=t)
        for t in (128, 192):
            for _ in range(10):
                launch(t)
        torch.cuda.synchronize()
        eq = torch.equal(outs[128], outs[192])
        times = {128: [], 192: []}
        for _ in range(ROUNDS):
            for t in (128, 192):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(LAUNCHES):
                    launch(t)
                e1.record()
                torch.cuda.synchronize()
                times[t].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
        m = {t: statistics.median(v) for t, v in times.items()}
        rule = K.lib.act_sgemm_nt_f16x3_pick_tile(M, N, Kd, cus)
        print(f"{M:6d} {N:5d} {Kd:5d}  {m[128]:10.1f} {m[192]:10.1f}  {m[192] / m[128]:6.3f}  {rule:4d}  {M // 128 * (N // 128):5d} {M // 128 * (N // 192):5d}  {eq}   "
              f"128: {min(times[128]):.1f}..{max(times[128]):.1f}  192: {min(times[192]):.1f}..{max(times[192]):.1f}", flush=True)
        if not eq:
            raise SystemExit("the two tiles gave different results")


if __name__ == "__main__":
    main()
