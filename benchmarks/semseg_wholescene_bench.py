#!/usr/bin/env python3
"""S3DIS whole-room sliding-window testing (act_amd/tools/runner_semseg_test.py, csrc/wholescene.hip) on one synthetic room: one JSON line.

    python benchmarks/semseg_wholescene_bench.py [--points 1000000] [--batch 32] [--npoint 2048] [--votes 2]

Reports blocks and rows per vote; device times (events) of membership (once per room), and per vote of the keyed row build, gather + centre,
the summed vote launches, the finish and the inference; the non-inference fraction of a vote; each kernel's HBM fraction against a byte model of
compulsory bytes (8 TB/s peak); the reference's host path on the same room (the restated dataset.py __getitem__ on the CPU, and main_test.py's
add_vote timed on a subset of rows and scaled: an estimate); and the eval forward per batch with and without the inverse adjacency.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TBS = 8.0                # HBM


def ev():
    return torch.cuda.Event(enable_timing=True)


def timed(fn):
    a, b = ev(), ev()
    a.record()
    out = fn()
    b.record()
    return out, (a, b)


def ms(pair):
    return pair[0].elapsed_time(pair[1])


def hbm(us, nbytes):
    return {"us": round(us, 1), "model_bytes": int(nbytes), "frac_of_hbm_peak": round(nbytes / (us * 1e-6) / (PEAK_TBS * 1e12), 4)}


def add_vote(pool, point_idx, pred_label, weight):
    """main_test.py add_vote, as written"""
    B, N = pred_label.shape
    for b in range(B):
        for n in range(N):
            if weight[b, n] != 0 and not np.isinf(weight[b, n]):
                pool[int(point_idx[b, n]), int(pred_label[b, n])] += 1
    return pool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--npoint", type=int, default=2048)
    ap.add_argument("--votes", type=int, default=2)
    ap.add_argument("--skip_host", action="store_true", help="skip the reference host path")
    args = ap.parse_args()
    from act_amd import kernels as K
    from act_amd.datasets.S3DISDataset import S3DISWholeScene, synthetic_room
    from act_amd.models.semseg import get_model
    from act_amd.tools.runner_semseg_test import Room
    dev = torch.device("cuda", 0)
    tmp = tempfile.mkdtemp()
    np.save(os.path.join(tmp, "Area_5_bench.npy"), synthetic_room(np.random.default_rng(0), args.points))
    ds = S3DISWholeScene(tmp, block_points=args.npoint)
    P = ds.scene_points_num[0]
    torch.manual_seed(0)
    model = get_model(13).to(dev).eval()
    lw = torch.from_numpy(ds.labelweights.astype(np.float32)).to(dev)

    # membership, once per room (warm-up room first: first-use GEMM tuning, allocations)
    room = Room(ds, 0, dev)
    torch.cuda.synchronize()
    (counts, off, ws), t_count = timed(lambda: K.scene_member_count(room.xyz, room.table, room.gx, room.gy))
    total = int(counts.sum().item())
    members, t_fill = timed(lambda: K.scene_member_fill(room.xyz, room.table, room.gx, room.gy, off, total, ws))
    torch.cuda.synchronize()
    bp, B, nblk = args.npoint, args.batch, room.num_blocks
    votes = torch.zeros(P, 13, dtype=torch.int32, device=dev)
    res = {k: [] for k in ("rows", "gather", "vote", "finish", "inference")}
    with torch.no_grad():
        for v in range(args.votes + 1):                                  # vote 0 is the warm-up
            rows, t_rows = timed(lambda: room.rows(0, 0, v))
            data, t_gather = timed(lambda: K.scene_gather(room.xyz, room.table, rows, room.block_ids, room.row_off).view(nblk, bp, 3))
            t_inf, t_vote = [], []
            for s in range(0, nblk, B):
                e = min(s + B, nblk)
                logp, ti = timed(lambda: model(data[s:e].transpose(2, 1)))
                _, tv = timed(lambda: K.scene_vote(logp, rows[s * bp:e * bp], room.label, lw, votes))
                t_inf.append(ti)
                t_vote.append(tv)
            (pred, cm), t_fin = timed(lambda: K.scene_finish(votes, room.label))
            torch.cuda.synchronize()
            if v:
                res["rows"].append(ms(t_rows)); res["gather"].append(ms(t_gather)); res["finish"].append(ms(t_fin))
                res["vote"].append(sum(ms(t) for t in t_vote)); res["inference"].append(sum(ms(t) for t in t_inf))
    m = {k: float(np.mean(x)) for k, x in res.items()}
    R, M = room.R, total
    non_inf = m["rows"] + m["gather"] + m["vote"] + m["finish"]
    out = {"bench": "semseg_wholescene", "points": P, "grid": [room.gx, room.gy], "blocks_per_vote": nblk, "rows_per_vote": R,
           "members": M, "batch": B, "npoint": bp,
           "membership_ms": round(ms(t_count) + ms(t_fill), 3),
           "per_vote_ms": {k: round(x, 3) for k, x in m.items()},
           "non_inference_ms": round(non_inf, 3), "non_inference_frac_of_vote": round(non_inf / (non_inf + m["inference"]), 5),
           "non_inference_over_inference": round(non_inf / m["inference"], 5),
           "kernels_hbm": {"member_count": hbm(ms(t_count) * 1e3, 16 * P + 8 * room.gx * room.gy),
                           "member_fill": hbm(ms(t_fill) * 1e3, 16 * P + 4 * M),
                           "rows": hbm(m["rows"] * 1e3, 8 * R),
                           "gather": hbm(m["gather"] * 1e3, 16 * R + 24 * P),
                           "vote_sum": hbm(m["vote"] * 1e3, 56 * R + 4 * P + 104 * P),
                           "finish": hbm(m["finish"] * 1e3, 60 * P)}}

    # eval forward per batch: with and without the inverse adjacency (semseg asks for it only when grad is enabled)
    x = data[:B].transpose(2, 1)
    orig = K.three_nn
    fw = {}
    with torch.no_grad():
        for tag, fn in (("without_adj", orig), ("with_adj", lambda a, c, want_adj=True: orig(a, c, True))):
            K.three_nn = fn
            try:
                for _ in range(3):
                    model(x)
                ts = [timed(lambda: model(x))[1] for _ in range(10)]
                torch.cuda.synchronize()
                fw[tag] = float(np.median([ms(t) for t in ts]))
            finally:
                K.three_nn = orig
    out["eval_forward_ms_per_batch"] = {k: round(v, 3) for k, v in fw.items()}
    out["eval_forward_adj_saving_ms"] = round(fw["with_adj"] - fw["without_adj"], 3)

    if not args.skip_host:
        t0 = time.perf_counter()
        data_room, label_room, smpw, index_room = ds.__getitem__(0, np.random.RandomState(0))
        t_get = time.perf_counter() - t0
        sub = min(16, index_room.shape[0])
        pred_sub = np.random.RandomState(1).randint(0, 13, size=(sub, bp))
        t0 = time.perf_counter()
        add_vote(np.zeros((P, 13)), index_room[:sub], pred_sub, smpw[:sub])
        t_vote_sub = time.perf_counter() - t0
        est_vote = t_vote_sub * index_room.shape[0] / sub
        host_ms = (t_get + est_vote) * 1e3
        out["reference_host"] = {"getitem_restated_ms": round(t_get * 1e3, 1), "add_vote_ms_estimate_scaled": round(est_vote * 1e3, 1),
                                 "add_vote_rows_timed": sub * bp, "per_vote_ms_estimate": round(host_ms, 1)}
        out["speedup_non_inference_vs_reference_host_estimate"] = round(host_ms / non_inf, 1)
        out["speedup_vote_end_to_end_estimate"] = round((host_ms + m["inference"]) / (non_inf + m["inference"]), 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
