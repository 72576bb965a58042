#!/usr/bin/env python3
"""Linear-SVM validation of pretrained features (utils/svm.py, csrc/svm.hip): one JSON line.

    python benchmarks/svm_bench.py [--n 9843] [--d 384] [--k 40] [--reps 5] [--no-sklearn] [--commit ID] [--out profiles/svm_bench.json]

Synthetic cluster features of the ModelNet40 validation's size (9,843 train rows, 384 features, 40 classes; 2,468 test rows).  Reports the wall
time of ``LinearSVC().fit`` (ending in a synchronise), its Newton / CG iteration counts and exit flags, the device time per launch of the two
products (scores X W^T + b and the transposed product P^T X) against their compulsory bytes, and ``sklearn.svm.LinearSVC()`` on the same arrays on
the host (as many threads as the process is given; liblinear itself is single-threaded) with the ratio of the two times.  No bar is set on
the ratio.  Times are medians of ``--reps`` repetitions after a warm-up, with min / max; kernel times are device events around ``inner``
back-to-back launches.
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


def spread(vals, digits=3):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def make(N, D, K, seed, sep, rows_test):
    r = np.random.default_rng(seed)
    mu = r.normal(size=(K, D)) * sep
    y, yt = r.integers(0, K, N), r.integers(0, K, rows_test)
    X = (mu[y] + r.normal(size=(N, D))).astype(np.float32)
    Xt = (mu[yt] + r.normal(size=(rows_test, D))).astype(np.float32)
    return X, y.astype(np.int64), Xt, yt.astype(np.int64)


def device_us(fn, reps, inner=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) / inner * 1e3)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=9843)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--rows-test", type=int, default=2468)
    ap.add_argument("--sep", type=float, default=0.12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--commit", type=str, default=os.environ.get("ACT_BENCH_COMMIT"))
    args = ap.parse_args()
    from act_amd import kernels as K
    from act_amd.utils.svm import LinearSVC
    dev = torch.device("cuda:0")
    N, D, Kc = args.n, args.d, args.k
    X, y, Xt, yt = make(N, D, Kc, 0, args.sep, args.rows_test)
    Xd, yd, Xtd, ytd = (torch.from_numpy(a).to(dev) for a in (X, y, Xt, yt))

    clf = LinearSVC().fit(Xd, yd)                                   # warm-up
    torch.cuda.synchronize()
    fit_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        clf = LinearSVC().fit(Xd, yd)
        torch.cuda.synchronize()
        fit_ms.append((time.perf_counter() - t0) * 1e3)
    acc = float((clf.predict(Xtd) == ytd).float().mean()) * 100
    st = clf.status_.tolist()

    W = torch.randn(Kc, D, device=dev)
    b = torch.randn(Kc, device=dev)
    P = torch.randn(N, Kc, device=dev)
    out = torch.empty(N, Kc, device=dev)
    us_scores = device_us(lambda: K.svm_scores(Xd, W, b, out=out), args.reps)
    us_masked = device_us(lambda: K.svm_scores(Xd, W, b, mask=P, out=out), args.reps)
    us_tprod = device_us(lambda: K.svm_tprod(P, Xd), args.reps)
    us_hinge = device_us(lambda: K.svm_hinge(out, yd, clf.classes_), args.reps)
    xb, nk, kd = 4.0 * N * D, 4.0 * N * Kc, 4.0 * Kc * D

    def prod(us, nbytes):
        med = statistics.median(us)
        return {"us": spread(us, 2), "compulsory_bytes": int(nbytes), "GB_per_s": round(nbytes / med * 1e-3, 1),
                "GFLOP_per_s": round(2.0 * N * D * Kc / med * 1e-3, 1)}
    res = {"workload": "svm_val", "sizes": {"N": N, "D": D, "K": Kc, "rows_test": args.rows_test, "sep": args.sep}, "commit": args.commit,
           "reps": args.reps, "fit_ms": spread(fit_ms), "newton_iterations": clf.n_iter_, "cg_iterations_max_class": clf.n_cg_,
           "exit_flags": {"tol": st.count(1), "no_progress": st.count(2), "cap": st.count(0)},
           "grad_norm_max_at_last_iteration": float(clf.grad_norm_.max()), "test_accuracy": round(acc, 3),
           "scores": prod(us_scores, xb + kd + nk), "scores_masked": prod(us_masked, xb + kd + 2 * nk),
           "tprod_with_reduction": prod(us_tprod, xb + nk + kd), "hinge_two_launches_us": spread(us_hinge, 2)}
    if not args.no_sklearn:
        from sklearn.svm import LinearSVC as SkSVC
        X64 = X.astype(np.float64)
        sk_ms = []
        for _ in range(max(1, min(args.reps, 3))):
            t0 = time.perf_counter()
            sk = SkSVC().fit(X64, y)
            sk_ms.append((time.perf_counter() - t0) * 1e3)
        sk_acc = float((sk.predict(Xt.astype(np.float64)) == yt).mean()) * 100
        agree = float((sk.predict(Xt.astype(np.float64)) == clf.predict(Xtd).cpu().numpy()).mean()) * 100
        res["sklearn"] = {"fit_ms": spread(sk_ms), "test_accuracy": round(sk_acc, 3), "predictions_equal_percent": round(agree, 3),
                          "cpus": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count(),
                          "ratio_sklearn_over_device": round(statistics.median(sk_ms) / statistics.median(fit_ms), 2)}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
