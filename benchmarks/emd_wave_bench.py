#!/usr/bin/env python3
"""The one-wave-per-pair Earth Mover's Distance (extensions/emd ``solver="wave"``, csrc/emd.hip) and the Stage-I loss built on it: one JSON line.

    python benchmarks/emd_wave_bench.py [--pairs 8192] [--windows 5] [--calls 200] [--no-step] [--train-steps 150] [--commit ID]
                                        [--out profiles/emd_wave_bench.json]

Every time is the median over ``--windows`` windows of back-to-back calls between two device events (window time / calls), kept with the
windows' min and max.
  * solver: 8,192 pairs of 32 points, centred gaussian patches of scale 0.1, eps = 1e-12, eps_rel = 2^-18: the wave solver and the workgroup
    solver through the same Python entry (``emd_cuda.forward``) on the same inputs (the workgroup solver takes an absolute eps: it gets the
    median of the wave solver's ``eps_used``), and the wave solver at 8,192 x 64;
  * bids per pair (``info`` of the wave solver): median and maximum;
  * the Stage-I training step of the synthetic ViT recipe (cfgs/synthetic/act_dvae_with_pretrained_transformer.yaml, and act_dvae_emd_loss.yaml
    for the key) at B = 128: ``runner_autoencoder.train_step`` with and without ``emd_loss``, same seed, same clouds;
  * with ``--train-steps K``: K training steps of both recipes at B = 8 from the same seed, then the evaluation table of each (F-Score, CDL1,
    CDL2 and the EMD column).
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

EPS, EPS_REL = 1e-12, 2.0 ** -18


def spread(vals, digits=4):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def windows(fn, n_windows, calls, warm=2):
    """ms per call: ``n_windows`` windows of ``calls`` back-to-back calls between device events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return out


def patches(rs, B, N, scale=0.1):
    return (scale * rs.standard_normal((B, N, 3))).astype(np.float32), (scale * rs.standard_normal((B, N, 3))).astype(np.float32)


def solver(args, E, N, with_workgroup):
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(100 + N)
    x1, x2 = (torch.from_numpy(t).to(dev) for t in patches(rs, args.pairs, N))
    dist, _, info, eps_used = E.emd_cuda.forward(x1, x2, EPS, solver="wave", eps_rel=EPS_REL, want_eps=True)
    info = info.cpu().numpy()
    wave = windows(lambda: E.emd_cuda.forward(x1, x2, EPS, solver="wave", eps_rel=EPS_REL), args.windows, args.calls)
    res = {"pairs": args.pairs, "N": N, "wave_ms": spread(wave), "bids": {"median": float(np.median(np.abs(info))), "max": int(np.abs(info).max())},
           "capped": int((info < 0).sum()), "ns_per_bid_per_pair": round(statistics.median(wave) * 1e6 / float(np.abs(info).sum()), 4),
           "mean_sqrt_dist": float(dist.double().sqrt().mean())}
    if with_workgroup:
        eps_abs = float(eps_used.median())
        d2, _, info2 = E.emd_cuda.forward(x1, x2, eps_abs)
        wg = windows(lambda: E.emd_cuda.forward(x1, x2, eps_abs), args.windows, max(1, args.calls // 4))
        res.update(workgroup_ms=spread(wg), workgroup_eps=eps_abs, workgroup_capped=int((info2 < 0).sum()),
                   workgroup_over_wave=round(statistics.median(wg) / statistics.median(wave), 3),
                   workgroup_mean_sqrt_dist=float(d2.double().sqrt().mean()))
    return res


def stage1_step(args, recipe):
    import logging
    from act_amd.models import build_model_from_cfg
    from act_amd.tools import builder
    from act_amd.tools.runner_autoencoder import train_step
    from act_amd.tools.runner_pretrain import _Single
    from act_amd.utils.config import cfg_from_yaml_file
    from act_amd.utils.logger import get_logger
    for n in ("ACT", "Transformer"):
        get_logger(n).setLevel(logging.ERROR)
    dev = torch.device("cuda:0")
    config = cfg_from_yaml_file(recipe)
    torch.manual_seed(0)
    model = build_model_from_cfg(config.model).to(dev).train()
    wrapped = _Single(model)
    optimizer, _ = builder.build_opti_sche(wrapped, config)
    torch.manual_seed(1234)
    rs = np.random.RandomState(1234)
    pool = []
    for _ in range(4):
        x = rs.standard_normal((args.batch, 1024, 3)).astype(np.float32)
        x -= x.mean(axis=1, keepdims=True)
        x /= np.sqrt((x ** 2).sum(axis=2)).max(axis=1)[:, None, None]
        pool.append(torch.from_numpy(x).to(dev))
    it = [0]

    def step():
        train_step(wrapped, optimizer, pool[it[0] % 4], config, 20000 + it[0])
        it[0] += 1
    ms = windows(step, args.windows, args.step_calls, warm=4)
    res = {"recipe": recipe, "batch": args.batch, "step_ms": spread(ms, 3)}
    if getattr(model, "emd_loss", None):
        info = model.emd_last_info.cpu().numpy()
        res.update(bids={"median": float(np.median(np.abs(info))), "max": int(np.abs(info).max())}, capped_total=int(model.emd_capped))
    return res


def train_run(args, recipe, tmp):
    """``--train-steps`` steps of the recipe at ``--train-batch`` from seed 0, then the evaluation table (with the EMD column) of the last checkpoint
    on 256 synthetic test clouds: an observation of what the loss does to the two distances, not a pass criterion"""
    import logging
    from act_amd.tools import runner_autoencoder as RA
    from act_amd.utils.config import cfg_from_yaml_file
    from act_amd.utils.logger import get_logger
    cfg = cfg_from_yaml_file(recipe)
    cfg.emd_val = True
    bs = args.train_batch
    for name, split in cfg.dataset.items():
        split._base_.update(NUM_SAMPLES=bs * args.train_steps if name == "train" else 256)
        split.others.update(bs=bs if name == "train" else 32)
    cfg.total_bs, cfg.max_epoch = bs, 0
    ns = argparse.Namespace(log_name="emd_wave_bench", use_gpu=True, local_rank=0, distributed=False, sync_bn=False, resume=False, start_ckpts=None,
                            experiment_path=tmp, num_workers=0, world_size=1, val_freq=1, ckpts=os.path.join(tmp, "ckpt-last.pth"))
    get_logger(ns.log_name).setLevel(logging.ERROR)
    torch.manual_seed(0)
    np.random.seed(0)
    log = RA.run_net(ns, cfg, max_steps=args.train_steps, log_every=50)
    m = RA.validate_net(ns, cfg)
    return {"recipe": recipe, "steps": len(log), "batch": bs, "last_recon_loss_x1000": round(float(np.mean([l1 for l1, _ in log[-10:]])), 3),
            "F-Score": round(m.state_dict()["F-Score"], 4), "CDL1": round(m.state_dict()["CDL1"], 3), "CDL2": round(m.state_dict()["CDL2"], 3),
            "EMD": round(m.emd["overall"], 3), "emd_val_capped": m.emd["capped"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8192)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--step-calls", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--train-steps", type=int, default=0, help="also train the two recipes for this many steps and evaluate them (0: skip)")
    ap.add_argument("--train-batch", type=int, default=8)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--commit", type=str, default=os.environ.get("ACT_BENCH_COMMIT"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("emd_wave_bench needs a GPU: there is nothing to time without one")
    from act_amd.extensions import emd as E
    res = {"workload": "emd_wave", "commit": args.commit, "windows": args.windows, "calls_per_window": args.calls, "eps": EPS, "eps_rel": EPS_REL,
           "solver": [solver(args, E, 32, True), solver(args, E, 64, False)]}
    if not args.no_step:
        off = stage1_step(args, "cfgs/synthetic/act_dvae_with_pretrained_transformer.yaml")
        on = stage1_step(args, "cfgs/synthetic/act_dvae_emd_loss.yaml")
        extra = on["step_ms"]["median"] - off["step_ms"]["median"]
        res["stage1_step"] = {"without_emd_loss": off, "with_emd_loss": on, "extra_ms": round(extra, 3),
                              "share_of_step": round(extra / on["step_ms"]["median"], 4)}
    if args.train_steps > 0:
        import tempfile
        runs = []
        for recipe in ("cfgs/synthetic/act_dvae_with_pretrained_transformer.yaml", "cfgs/synthetic/act_dvae_emd_loss.yaml"):
            with tempfile.TemporaryDirectory() as tmp:
                runs.append(train_run(args, recipe, tmp))
        res["train_runs"] = runs
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
