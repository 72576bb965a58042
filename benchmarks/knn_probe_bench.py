#!/usr/bin/env python3
"""Weighted k-NN probe of frozen features (utils/knn_probe.py, csrc/knn_probe.hip): one JSON line.

    python benchmarks/knn_probe_bench.py [--nq 2468] [--nb 9843 52470] [--d 768] [--k 20 200] [--reps 7] [--commit ID] [--out profiles/knn_probe_bench.json]

Synthetic cluster features at ModelNet40's split sizes (2,468 test clouds against 9,843 train clouds) and against a ShapeNet-55-sized bank
(52,470 rows), 768 = 2 x 384 concat_f features, 40 classes.  Per shape and k: the time of the fused search (both normalisations, similarity +
streaming top-k, merge), of the vote, and of the torch composition of the same probe on the same device (normalize, mm, topk, exp, scatter_add,
argmax), which writes the Nq x Nb similarity matrix.  Times are device-event medians of ``--reps`` repetitions after a warm-up, with min / max; the
two versions alternate inside one repetition.  The capability is new, so there is no earlier time of this project to compare with.

Model numbers, from the shapes: 2 Nq Nb Dp FLOP over the search time against the 157.3 TFLOP/s f32 MFMA peak (Dp: D padded to 16), and the bytes the
search moves through the memory system as launched: every query tile reads its bank range once and every bank tile re-reads its query tile
(both mostly from L2), plus the padded copies and the partial lists.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.3e12


def spread(vals, digits=3):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def make(N, D, K, seed, sep):
    r = np.random.default_rng(seed)
    mu = r.normal(size=(K, D)) * sep
    y = r.integers(0, K, N)
    return (mu[y] + r.normal(size=(N, D))).astype(np.float32), y.astype(np.int64)


def timed(fns, reps):
    """device-event milliseconds of every function of ``fns``, alternating them inside a repetition"""
    for f in fns:
        f()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            out[i].append(a.elapsed_time(b))
    return out


def torch_probe(q, bank, cls, C, k, T):
    qn, bn = torch.nn.functional.normalize(q, dim=1, eps=1e-12), torch.nn.functional.normalize(bank, dim=1, eps=1e-12)
    sim, idx = torch.mm(qn, bn.t()).topk(k, dim=1)
    scores = torch.zeros(q.shape[0], C, dtype=torch.float32, device=q.device).scatter_add_(1, cls[idx], torch.exp(sim / T))
    return scores.argmax(dim=1)


def one(Nq, Nb, D, k, args, K):
    dev = torch.device("cuda:0")
    xb, yb = make(Nb, D, 40, 0, args.sep)
    xq, _ = make(Nq, D, 40, 1, args.sep)
    bank, q = torch.from_numpy(xb).to(dev), torch.from_numpy(xq).to(dev)
    cls32, cls64 = torch.from_numpy(yb).to(dev).int(), torch.from_numpy(yb).to(dev)
    sim, idx = K.knn_probe_search(q, bank, k)
    search, vote, ref = timed([lambda: K.knn_probe_search(q, bank, k),
                               lambda: K.knn_probe_vote(sim, idx, cls32, 40, [k], args.T, want_scores=False),
                               lambda: torch_probe(q, bank, cls64, 40, k, args.T)], args.reps)
    _, pred, _ = K.knn_probe_vote(sim, idx, cls32, 40, [k], args.T, want_scores=False)
    agree = float((pred[:, 0] == torch_probe(q, bank, cls64, 40, k, args.T)).float().mean())
    dp = (D + 15) // 16 * 16
    qt = 64 if k <= 128 else 32
    splits = K.lib.act_knn_probe_splits(Nq, Nb, k, 0)
    tiles_q, tiles_b = (Nq + qt - 1) // qt, (Nb + 127) // 128
    flop = 2.0 * Nq * Nb * dp
    moved = 4.0 * dp * (tiles_q * Nb + tiles_b * Nq * 1.0) + 8.0 * dp * (Nq + Nb) + 16.0 * splits * Nq * k
    s_med = statistics.median(search) * 1e-3
    return {"Nq": Nq, "Nb": Nb, "D": D, "k": k, "splits": splits, "query_tile": qt,
            "search_ms": spread(search), "vote_ms": spread(vote, 4), "torch_mm_topk_scatter_ms": spread(ref),
            "fused_over_torch": round((statistics.median(search) + statistics.median(vote)) / statistics.median(ref), 3),
            "search_tflops": round(flop / s_med / 1e12, 2), "fraction_of_f32_mfma_peak": round(flop / s_med / PEAK_F32_MFMA, 3),
            "bytes_moved_model": int(moved), "bytes_per_s_model": float("%.4g" % (moved / s_med)),
            "similarity_matrix_bytes_not_written": 4 * Nq * Nb, "prediction_agreement_with_torch": round(agree, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=2468)
    ap.add_argument("--nb", type=int, nargs="+", default=[9843, 52470])
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, nargs="+", default=[20, 200])
    ap.add_argument("--T", type=float, default=0.07)
    ap.add_argument("--sep", type=float, default=0.12)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--commit", type=str, default=os.environ.get("ACT_BENCH_COMMIT"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_probe_bench needs a GPU: there is nothing to time without one")
    from act_amd import kernels as K
    res = {"workload": "knn_probe", "commit": args.commit, "reps": args.reps, "T": args.T,
           "runs": [one(args.nq, nb, args.d, k, args, K) for nb in args.nb for k in args.k]}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
