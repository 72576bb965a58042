#!/usr/bin/env python3
"""Exact t-SNE of classifier features (utils/tsne.py, csrc/tsne.hip): one JSON line.

    python benchmarks/tsne_bench.py [--n 2468 9843] [--d 768] [--perplexity 25] [--reps 5] [--no-sklearn] [--commit ID] [--out profiles/tsne_bench.json]

Synthetic cluster features of ModelNet40's two split sizes (2,468 test and 9,843 train clouds, 768 = 2 x 384 concat_f features, 40 classes).  Per
size: the time of the kNN graph, the perplexity search, the symmetrisation, one optimisation step and a whole 250 + 500 iteration fit (PCA
initialisation included, ending in a synchronise), and the pair evaluations per second of the all-pairs sweep against a vector-issue model of
its inner loop: 8 full-rate and 1 quarter-rate vector instruction per pair, 256 CUs x 4 SIMDs x 32 lanes at 2.4 GHz (the fraction reached is
reported, no target is set).  When sklearn imports, the wall time of ``sklearn.manifold.TSNE(method="exact", metric="cosine")`` on the same
array on the host.  Times are medians of ``--reps`` repetitions after a warm-up, with min / max.
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

SWEEP_SLOTS_PER_PAIR = 8 + 4            # sub, sub, 2 fma, add, mul, 2 fma at full rate; one reciprocal at a quarter of it
PEAK_LANE_OPS = 256 * 4 * 32 * 2.4e9    # vector lanes x clock


def spread(vals, digits=3):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def make(N, D, K, seed, sep):
    r = np.random.default_rng(seed)
    mu = r.normal(size=(K, D)) * sep
    y = r.integers(0, K, N)
    return (mu[y] + r.normal(size=(N, D))).astype(np.float32), y.astype(np.int64)


def wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def one_size(N, D, args, K, TSNE):
    dev = torch.device("cuda:0")
    X, _ = make(N, D, 40, 0, args.sep)
    Xd = torch.from_numpy(X).to(dev)
    k = min(N - 1, int(3 * args.perplexity))
    lr = max(200.0, N / 12.0)
    idx, dist = K.tsne_knn_cosine(Xd, k)
    p = K.tsne_conditional_p(dist, args.perplexity)
    csr = K.tsne_symmetrize(idx, p)
    Y = K.tsne_pca_init(Xd)
    U, G = torch.zeros_like(Y), torch.ones_like(Y)
    inner = 50
    res = {"N": N, "k": k, "nnz": int(csr[1].numel()),
           "knn_ms": spread(wall_ms(lambda: K.tsne_knn_cosine(Xd, k), args.reps)),
           "perplexity_search_ms": spread(wall_ms(lambda: K.tsne_conditional_p(dist, args.perplexity), args.reps)),
           "symmetrize_ms": spread(wall_ms(lambda: K.tsne_symmetrize(idx, p), args.reps)),
           "pca_init_ms": spread(wall_ms(lambda: K.tsne_pca_init(Xd), args.reps))}
    step_ms = [t / inner for t in wall_ms(lambda: K.tsne_steps(csr, Y, U, G, inner, 12.0, 0.5, lr), args.reps)]
    res["step_ms"] = spread(step_ms, 4)
    pairs = float(N) * N / (statistics.median(step_ms) * 1e-3)
    res["step_pairs_per_s"] = float("%.4g" % pairs)
    res["step_fraction_of_vector_issue_model"] = round(pairs * SWEEP_SLOTS_PER_PAIR / PEAK_LANE_OPS, 3)
    tsne = TSNE(perplexity=args.perplexity)
    fit = wall_ms(lambda: tsne.fit(Xd), args.reps)
    res["fit_750_iterations_ms"] = spread(fit, 1)
    res["kl_divergence"] = round(tsne.kl_divergence_, 4)
    if not args.no_sklearn and N <= args.sklearn_max_n:
        try:
            from sklearn.manifold import TSNE as SkTSNE
            t0 = time.perf_counter()
            sk = SkTSNE(method="exact", metric="cosine", perplexity=args.perplexity, init="pca").fit(X)
            res["sklearn_exact"] = {"fit_s": round(time.perf_counter() - t0, 1), "kl_divergence": round(float(sk.kl_divergence_), 4),
                                    "cpus": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()}
        except Exception as e:                                    # the line is printed without it
            res["sklearn_exact"] = {"error": "%s: %s" % (type(e).__name__, e)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2468, 9843])
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--perplexity", type=float, default=25)
    ap.add_argument("--sep", type=float, default=0.12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--sklearn-max-n", type=int, default=2468, help="largest N the host's exact t-SNE is run at (it is O(N^2) per iteration on the CPU)")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--commit", type=str, default=os.environ.get("ACT_BENCH_COMMIT"))
    args = ap.parse_args()
    from act_amd import kernels as K
    from act_amd.utils.tsne import TSNE
    res = {"workload": "tsne", "sizes": {"D": args.d, "perplexity": args.perplexity, "sep": args.sep}, "commit": args.commit, "reps": args.reps,
           "runs": [one_size(N, args.d, args, K, TSNE) for N in args.n]}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
