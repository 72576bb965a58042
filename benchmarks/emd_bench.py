#!/usr/bin/env python3
"""Earth Mover's Distance (extensions/emd, csrc/emd.hip): one JSON line.

    python benchmarks/emd_bench.py [--n 1024 2048] [--b 1 32 128] [--eps 1e-5] [--reps 5] [--commit ID] [--out profiles/emd_bench.json]

Cloud pairs uniform on the unit sphere, the second scaled by 0.9 (the inputs of tests/golden/g24_emd.npz, other seeds).  Per (N, B): the device
time of the forward solve and of the backward (device-event medians of ``--reps`` repetitions after a warm-up, with min / max), the rounds used
(median and max over the batch) and the bids made.  The capability is new, so there is no earlier time of this project to compare with; the time
of scipy.optimize.linear_sum_assignment on the first pair, on the host, is recorded next to it when scipy imports.

Rates.  A bid is one scan of the N objects, so distance evaluations = bids x N (the sum over rounds of unassigned bidders x N).  The
vector-issue model (notebook/emd.md): the scan loop issues 20 vector instructions per 64 evaluations, a wave64 instruction occupies its SIMD
for 2 cycles, and a pair has the 4 SIMDs of ONE compute unit, so a pair can do at most 4 * 64 / (20 * 2) = 6.4 evaluations per cycle, 1.54e10
per second at 2.4 GHz; ``share_of_issue_model`` is evaluations per second over that, times the pairs in flight (min(B, 256 compute units)).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLOCK_HZ, CUS, SCAN_VALU_PER_64, CYCLES_PER_WAVE_OP, SIMDS = 2.4e9, 256, 20, 2, 4
MODEL_EVALS_PER_S_PER_PAIR = SIMDS * 64 / (SCAN_VALU_PER_64 * CYCLES_PER_WAVE_OP) * CLOCK_HZ


def spread(vals, digits=3):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def sphere(rs, B, N, scale=1.0):
    x = rs.standard_normal((B, N, 3))
    return (scale * x / np.linalg.norm(x, axis=2, keepdims=True)).astype(np.float32)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def host_lsa(x1, x2):
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        return None
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from emd_ref import sqdist
    c = sqdist(x1, x2).astype(np.float64)
    t = time.perf_counter()
    rows, cols = linear_sum_assignment(c)
    return {"ms": round((time.perf_counter() - t) * 1e3, 2), "optimum": float(c[rows, cols].sum())}


def one(N, B, args, E):
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(100 + N)
    h1, h2 = sphere(rs, B, N), sphere(rs, B, N, 0.9)
    x1, x2 = torch.from_numpy(h1).to(dev), torch.from_numpy(h2).to(dev)
    dist, assignment, info, bids = E.emd_cuda.forward(x1, x2, args.eps, want_evals=True)
    g = torch.ones_like(dist)
    fwd = timed(lambda: E.emd_cuda.forward(x1, x2, args.eps), args.reps)
    bwd = timed(lambda: E.emd_cuda.backward(x1, x2, assignment, g), args.reps)
    info, bids = info.cpu().numpy(), bids.cpu().numpy()
    evals = float(bids.sum()) * N
    per_s = evals / (statistics.median(fwd) * 1e-3)
    res = {"N": N, "B": B, "forward_ms": spread(fwd), "backward_ms": spread(bwd, 4),
           "rounds": {"median": float(np.median(np.abs(info))), "max": int(np.abs(info).max())}, "capped": int((info < 0).sum()),
           "bids": int(bids.sum()), "distance_evaluations": evals, "evaluations_per_s": float("%.4g" % per_s),
           "share_of_issue_model": round(per_s / (MODEL_EVALS_PER_S_PER_PAIR * min(B, CUS)), 4),
           "us_per_round": round(statistics.median(fwd) * 1e3 / float(np.abs(info).max()), 3),
           "sum_dist_pair0": float(dist[0].double().sum())}
    if B == 1:
        res["scipy_linear_sum_assignment_host"] = host_lsa(h1[0], h2[0])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--b", type=int, nargs="+", default=[1, 32, 128])
    ap.add_argument("--eps", type=float, default=1e-5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--commit", type=str, default=os.environ.get("ACT_BENCH_COMMIT"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("emd_bench needs a GPU: there is nothing to time without one")
    from act_amd.extensions import emd as E
    res = {"workload": "emd", "commit": args.commit, "reps": args.reps, "eps_final": args.eps,
           "issue_model_evaluations_per_s_per_pair": float("%.4g" % MODEL_EVALS_PER_S_PER_PAIR),
           "runs": [one(N, B, args, E) for N in args.n for B in args.b]}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
