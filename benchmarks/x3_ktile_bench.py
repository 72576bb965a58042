#!/usr/bin/env python3
"""The split-f16 product alone, B row-major against B K-tile-major (and A as well where the step hands it on that way), at the shapes of the Stage-II step:
alternating, device events, three rounds of 20 launches each (notebook/x3_ktile.md).  One JSON line per shape."""
import json
import statistics
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import act_amd.kernels as K   # noqa: E402

SHAPES = [("teacher fc1", 8192, 3072, 768), ("teacher fc2", 8192, 768, 3072), ("teacher qkv", 8192, 2304, 768), ("teacher proj", 8192, 768, 768),
          ("prompt keys / values", 8192, 1536, 768), ("tokenizer head", 8192, 8192, 2304)]
ROUNDS, REPS = 3, 20


def timed(fn):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for name, M, N, Kd in SHAPES:
        a = torch.randn(M, Kd, generator=g).to(dev)
        w = (0.05 * torch.randn(N, Kd, generator=g)).to(dev)
        sb, sb_inv = K.f16x3_row_scales(w)
        ap, bp = K.split_f16x2(a, 64.0), K.split_f16x2(w, 1.0, sb)
        akt, bkt = K.repack_ktile(ap), K.repack_ktile(bp)
        out = torch.empty(M, N, dtype=torch.float32, device=dev)
        flat = lambda p: (p[0].reshape(-1), p[1].reshape(-1))
        forms = {
            "row": lambda: K.gemm_nt_f16x3_layout(M, N, Kd, flat(ap), 64.0, flat(bp), sb_inv, out=out),
            "b_kt": lambda: K.gemm_nt_f16x3_layout(M, N, Kd, flat(ap), 64.0, flat(bkt), sb_inv, b_layout=K.X3_KTILE, b_rows_total=N, out=out),
            "ab_kt": lambda: K.gemm_nt_f16x3_layout(M, N, Kd, flat(akt), 64.0, flat(bkt), sb_inv, a_layout=K.X3_KTILE, a_rows_total=M, b_layout=K.X3_KTILE,
                                                    b_rows_total=N, out=out),
        }
        ref = forms["row"]().clone()
        for f in forms.values():
            assert torch.equal(f(), ref)
            for _ in range(5):
                f()
        res = {k: [] for k in forms}
        for _ in range(ROUNDS):
            for k, f in forms.items():
                res[k].append(round(timed(f), 1))
        print(json.dumps({"product": name, "M": M, "N": N, "K": Kd, "median_us_per_round": res,
                          "tflops_equiv": {k: round(2.0 * M * N * Kd / (statistics.median(v) * 1e-6) / 1e12, 1) for k, v in res.items()}}), flush=True)


if __name__ == "__main__":
    main()
