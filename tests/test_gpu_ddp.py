"""The PRODUCT model under DistributedDataParallel with world_size 2 on one GPU (gloo transporting CUDA tensors, both ranks on
cuda:0): runner_pretrain.wrap_ddp + train_step(next_points=...) with the cross-step teacher prefetch on auxiliary stream 0, the
weight-gradient GEMMs on auxiliary stream 1 and gradient_as_bucket_view buckets, i.e. DDP's bucket hooks racing against both
side streams (reference: tools/runner_pretrain.py:84-93,145-167).

  * trajectory: 4 pipelined AdamW steps with identical shards / seeds on both ranks are bit-identical to the single-process run
    (the all-reduce mean of two equal fp32 values is exact);
  * averaging: with different shards and seeds per rank, the gradients DDP leaves in .grad equal the mean of the single-rank
    gradients (same seeds, no DDP), and are identical on both ranks.
"""
import argparse
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 4


def _cfg(step_per_update=1):
    from act_amd.utils.config import EasyDict
    return EasyDict(optimizer=dict(type="AdamW", kwargs=dict(lr=1e-3, weight_decay=0.05)),
                    scheduler=dict(type="CosLR", kwargs=dict(epochs=300, initial_epochs=10)), step_per_update=step_per_update)


def _model(dev):
    import copy
    from act_amd.models import build_model_from_cfg
    from act_amd.tools.runner_pretrain import freeze_unused_heads
    from act_amd.utils.config import EasyDict
    from tests.golden.fill import fill_module, TINY_STAGE2
    cfg = copy.deepcopy(TINY_STAGE2)
    cfg["transformer_config"]["drop_path_rate"] = 0.2            # DropPath draws active
    torch.manual_seed(0)
    model = fill_module(build_model_from_cfg(EasyDict(cfg)), "ddp.").to(dev).train()
    freeze_unused_heads(model)
    return model


def _batches(seed0, dev):
    from tests.golden.fill import clouds
    return [torch.from_numpy(clouds(seed0 + i, 4, 128)).to(dev) for i in range(STEPS)]


def _trajectory(wrapped, model, seed, data_seed, dev):
    """STEPS pipelined steps -> (losses, parameters)"""
    from act_amd.tools import builder
    from act_amd.tools.runner_pretrain import train_step
    cfg = _cfg()
    opt, _ = builder.build_opti_sche(wrapped, cfg)
    torch.manual_seed(seed)
    pts = _batches(data_seed, dev)
    losses = []
    for i in range(STEPS):
        nxt = pts[i + 1] if i + 1 < STEPS else None
        losses.append(train_step(wrapped, opt, pts[i], cfg, next_points=nxt))
        if nxt is not None:
            assert model._prefetched is not None and model._prefetched[0] is nxt      # the pipelined path really ran
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), {n: p.detach().clone().cpu() for n, p in model.named_parameters()}


def _one_step_grads(wrapped, model, seed, data_seed, dev):
    """forward + backward of one pipelined step without the optimizer step -> gradients left in .grad"""
    from act_amd.tools import builder
    from act_amd.tools.runner_pretrain import train_step
    cfg = _cfg(step_per_update=2)                                   # num_iter=1 != 2: train_step does not step / zero the grads
    opt, _ = builder.build_opti_sche(wrapped, cfg)
    torch.manual_seed(seed)
    pts = _batches(data_seed, dev)
    loss = train_step(wrapped, opt, pts[0], cfg, num_iter=1, next_points=pts[1])
    torch.cuda.synchronize()
    return loss.item(), {n: p.grad.detach().clone().cpu() for n, p in model.named_parameters() if p.grad is not None}


class _fixed_gemm_configs:
    """Bitwise comparisons ACROSS processes need the same GEMM launch configuration (tile / split-K = fp32 summation order) in each
    of them: switch the timing-based first-use autotuner off (built-in cost model + shipped table only) and drop cached winners."""

    def __enter__(self):
        import act_amd.kernels as K
        import act_amd.composite as CP
        self.K, self.CP, self.saved = K, CP, (K.AUTOTUNE, dict(K._GEMM_CACHE))
        K.AUTOTUNE = False
        K._GEMM_CACHE.clear()
        CP.reset_tuning()                      # C-side table back to the shipped entries only

    def __exit__(self, *exc):
        self.K.AUTOTUNE = self.saved[0]
        self.K._GEMM_CACHE.clear()
        self.K._GEMM_CACHE.update(self.saved[1])
        self.CP.reset_tuning()                 # composites re-collect (and re-register the cached winners) on next use


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["ACT_GEMM_AUTOTUNE"] = "0"
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from act_amd.tools.runner_pretrain import wrap_ddp
    ns = argparse.Namespace(local_rank=rank, use_gpu=True)
    # (1) same data and seeds on both ranks: trajectory must equal the single-process one bit for bit
    model = _model(dev)
    ddp = wrap_ddp(model, ns)
    assert isinstance(ddp, torch.nn.parallel.DistributedDataParallel) and ddp.gradient_as_bucket_view
    losses, params = _trajectory(ddp, model, seed=123, data_seed=20, dev=dev)
    # (2) different shards and seeds: gradients are the mean over ranks
    model2 = _model(dev)
    ddp2 = wrap_ddp(model2, ns)
    loss2, grads2 = _one_step_grads(ddp2, model2, seed=500 + rank, data_seed=40 + 10 * rank, dev=dev)
    torch.save({"losses": losses, "params": params, "loss2": loss2, "grads2": grads2}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_product_model_under_ddp_two_ranks_one_gpu(tmp_path):
    assert torch.cuda.is_available()
    from act_amd.tools.runner_pretrain import _Single
    dev = torch.device("cuda:0")
    port = 29500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r = [torch.load(tmp_path / f"r{i}.pt") for i in range(2)]

    # ---- (1) 4-step pipelined trajectory: DDP(2 ranks, equal shards) == single process, bitwise -----------------------
    with _fixed_gemm_configs():
        model = _model(dev)
        losses, params = _trajectory(_Single(model), model, seed=123, data_seed=20, dev=dev)
        single = []
        for rank in range(2):
            m = _model(dev)
            single.append(_one_step_grads(_Single(m), m, seed=500 + rank, data_seed=40 + 10 * rank, dev=dev))
    for rank in range(2):
        assert torch.equal(r[rank]["losses"], losses), (rank, r[rank]["losses"], losses)
        for n, p in params.items():
            assert torch.equal(r[rank]["params"][n], p), (rank, n)
    assert len(set(losses.tolist())) == STEPS                       # the model actually moved

    # ---- (2) gradient averaging across different shards ---------------------------------------------------------------
    assert set(r[0]["grads2"]) == set(single[0][1])
    assert not any("lm_head" in n or "cls_head" in n for n in r[0]["grads2"])
    for rank in range(2):
        assert abs(r[rank]["loss2"] - single[rank][0]) <= 1e-6      # the local loss is not averaged
    assert abs(single[0][0] - single[1][0]) > 1e-4                   # the shards really differ
    for n, g0 in single[0][1].items():
        want = 0.5 * (g0.double() + single[1][1][n].double())
        scale = max(1e-6, want.abs().max().item())
        for rank in range(2):
            err = (r[rank]["grads2"][n].double() - want).abs().max().item()
            assert err <= 2e-6 * scale + 1e-9, (n, rank, err, scale)
        assert torch.equal(r[0]["grads2"][n], r[1]["grads2"][n]), n  # identical on both ranks after the all-reduce


# ---- --sync_bn: SyncBatchNorm statistics across ranks (tools/runner_pretrain.py:86-88) -----------------------------------------
def _sync_bn_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from act_amd.models.dvae import Encoder
    from tests.golden.fill import fill_module
    enc = torch.nn.SyncBatchNorm.convert_sync_batchnorm(fill_module(Encoder(64), "sbn.")).to(dev).train()
    assert isinstance(enc.first_conv[1], torch.nn.SyncBatchNorm)
    g = torch.Generator().manual_seed(5)
    nb_all = 0.3 * torch.randn(8, 16, 8, 3, generator=g); dout_all = torch.randn(8, 16, 64, generator=g)
    sl = slice(4 * rank, 4 * rank + 4)
    y = enc(nb_all[sl].to(dev))
    y.backward(dout_all[sl].to(dev))
    torch.cuda.synchronize()
    torch.save({"y": y.detach().cpu(), "grads": {n: p.grad.cpu() for n, p in enc.named_parameters()},
                "rm": enc.second_conv[1].running_mean.cpu(), "rv": enc.first_conv[1].running_var.cpu()}, os.path.join(out_dir, f"s{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_sync_batchnorm_two_ranks_equals_full_batch(tmp_path):
    """2 ranks x 4 clouds under SyncBatchNorm == 1 process x 8 clouds under BatchNorm: outputs, running statistics, and the
    rank-summed parameter gradients (train-mode statistics over the rows of all ranks, forward and backward)."""
    from act_amd.models.dvae import Encoder
    from tests.golden.fill import fill_module
    dev = torch.device("cuda:0")
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_sync_bn_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r = [torch.load(tmp_path / f"s{i}.pt") for i in range(2)]
    enc = fill_module(Encoder(64), "sbn.").to(dev).train()
    g = torch.Generator().manual_seed(5)
    nb_all = 0.3 * torch.randn(8, 16, 8, 3, generator=g); dout_all = torch.randn(8, 16, 64, generator=g)
    y = enc(nb_all.to(dev)); y.backward(dout_all.to(dev))
    rel = lambda a, b: ((a.double() - b.double()).abs().max() / max(1.0, b.double().abs().max().item())).item()
    assert rel(torch.cat([r[0]["y"], r[1]["y"]]), y.detach().cpu()) <= 1e-5
    for n, p in enc.named_parameters():
        # relative to the per-rank summands: a conv bias in front of BatchNorm has an exactly-zero total gradient, +x on one rank, -x on the other
        scale = max(1.0, r[0]["grads"][n].abs().max().item(), r[1]["grads"][n].abs().max().item())
        err = (r[0]["grads"][n].double() + r[1]["grads"][n].double() - p.grad.cpu().double()).abs().max().item()
        assert err <= 2e-5 * scale, (n, err, scale)
    for rank in range(2):
        assert rel(r[rank]["rm"], enc.second_conv[1].running_mean.cpu()) <= 1e-5
        assert rel(r[rank]["rv"], enc.first_conv[1].running_var.cpu()) <= 1e-5
    # without synchronisation the two halves would normalise with their own statistics
    assert rel(r[0]["y"], enc(nb_all[:4].to(dev)).detach().cpu()) > 1e-3


@pytest.mark.parametrize("launcher", ["torchrun", "self"])
def test_bench_two_ranks_on_one_gpu_prints_one_line(tmp_path, launcher):
    """bench.py at world size 2 (both ranks on cuda:0, gloo instead of RCCL: the only multi-rank form a one-GPU box allows), launched (i) the
    driver's way under torch.distributed.run and (ii) as plain ``python bench.py --gpus 2`` with NO launcher environment -- bench.py then spawns
    its own ranks (reference main.py:21-28,44-58 takes the ranks from the launcher env; utils/dist_utils.py:9-24).  Warm-up, timed steps, the
    idle-GPU host-cost steps, the all-reduce probe and the instrumented pass all run on EVERY rank (each step contains the gradient all-reduce, so a
    rank-0-only pass would wait in a collective for ever); rank 0 prints exactly one JSON line with the whole-job value."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ACT_BENCH_SHARE_GPU="1", ACT_BENCH_BACKEND="gloo", ACT_GEMM_AUTOTUNE="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    tail = [os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "8", "--full", "--no-cpu-baseline"]
    if launcher == "torchrun":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29547"] + tail
    else:
        cmd = [sys.executable] + tail
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["config"]["parallelism"] == "dp2" and d["scaling"] == "weak"
    assert d["value"] > 0 and abs(d["value"] - 2 * 8 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]      # whole-job clouds/s = B * world / step time
    assert "roofline" in d and "cpu_baseline" not in d and d["config"]["final_loss"] == d["config"]["final_loss"]
    assert d["roofline"]["step"]["executed_tflop"] > 0 and "parity_bar" in d["config"]
    assert len(d["ms_per_step_by_rank"]) == 2 and max(d["ms_per_step_by_rank"]) == pytest.approx(d["ms_per_step"], rel=1e-3)
    c = d["comm"]
    assert c["backend"] == "gloo" and c["world_size_seen_by_rccl"] == 2 and c["allreduce_ms"] > 0 and c["allreduce_bus_GBps"] > 0
    assert ("bench.py itself" in c["launched_by"]) == (launcher == "self")


@pytest.mark.parametrize("gpus", [2, 1])
def test_bench_preflight_self_launched(tmp_path, gpus):
    """``python bench.py --gpus N --preflight`` (reference main.py:21-28,44-67, utils/dist_utils.py:9-24): the <= 30 s readiness check a
    SCALE run can be preceded by -- process-group init on every rank, the all-reduce probe of the gradient payload, 1 + 2 DDP steps, per-rank core
    pinning -- self-launched at 2 ranks (both on cuda:0 over gloo: what a one-GPU box allows) and at 1 rank (a world-1 RCCL group: the nccl code path)."""
    import json
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ACT_GEMM_AUTOTUNE="0")
    if gpus == 2:
        env.update(ACT_BENCH_SHARE_GPU="1", ACT_BENCH_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "ACT_PIN_CORES", "ACT_BLOCK_STACK_CHUNK"):
        env.pop(k, None)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(gpus), "--preflight", "--batch", "8"], cwd=root, env=env,
                       capture_output=True, text=True, timeout=600)
    wall = time.time() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    pf = d["preflight"]
    assert pf["ok"] and pf["world_size_seen_by_rccl"] == gpus and pf["backend"] == ("gloo" if gpus == 2 else "nccl")
    assert d["n_gpus"] == gpus and d["steps"] == 2 and pf["allreduce_ms"] > 0 and pf["final_loss"] == pf["final_loss"]
    aff = d["config"]["host_affinity_by_rank"]
    assert len(aff) == gpus
    if gpus == 2:
        assert pf["stack_chunk"] == 4                                   # multi-rank DDP: block stacks in chunks of 4 (wrap_ddp)
        if all(a["pinned"] for a in aff):                              # (a one-core cpuset cannot be split)
            assert pf["ranks_pinned"] == 2 and aff[0]["cores"] != aff[1]["cores"]
    else:
        assert pf["stack_chunk"] == 0 and not aff[0]["pinned"]
        # the one-JSON-line contract on stdout also holds with RCCL initialised (its warnings go to stderr: NCCL_DEBUG_FILE)
        assert [l for l in r.stdout.splitlines() if l.strip()] == lines, r.stdout[-1500:]
    assert "roofline" not in d and "cpu_baseline" not in d and "other_workloads" not in d
    print(f"[preflight] gpus={gpus}: wall {wall:.1f} s (in-process {pf['wall_s']} s), process group init {pf['process_group_init_s']} s, "
          f"all-reduce {pf['allreduce_ms']:.2f} ms, affinity {aff}")


def test_bench_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """a plain ``python bench.py --steps K --warmup W --dump-outputs DIR``: exactly K timed steps, the headline fields only (the instrumented
    pass, CPU baseline and other workloads are --full), and the last timed step's outputs as DIR/<name>.npy -- the same bits in two processes."""
    import json
    import subprocess
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["ACT_GEMM_AUTOTUNE"] = "0"
    dumps = []
    for run in range(2):
        out = os.path.join(tmp_path, "run%d" % run)
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8",
                            "--dump-outputs", out], cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "clouds/s" and d["higher_is_better"] and d["dtype"] == "f32"
        assert d["metric"] == "stage2_pretrain_point_clouds_per_sec" and abs(d["value"] - 8 * 3 / (d["ms_per_step"] * 3e-3)) < 1e-6 * d["value"]
        assert not {"roofline", "kernels", "group_fps_knn", "other_workloads", "cpu_baseline", "comm"} & set(d)
        files = sorted(os.listdir(out))
        assert files == ["loss.npy", "params_sample.npy"], files
        arrays = {f: np.load(os.path.join(out, f)) for f in files}
        assert all(a.dtype == np.float32 for a in arrays.values()) and sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert float(arrays["loss.npy"]) == d["config"]["final_loss"] and arrays["params_sample.npy"].shape == (1 << 20,)
        assert np.isfinite(arrays["params_sample.npy"]).all()
        dumps.append(arrays)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f


def test_bench_tolerates_a_gpus_flag_that_disagrees_with_the_launcher(tmp_path):
    """the launcher's WORLD_SIZE is the truth: ``--gpus 8`` under a one-rank launcher environment reports n_gpus = 1 instead of dying on an assert
    (round-4 verdict: the one 8-GPU slot must not be lost to a flag)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", ACT_GEMM_AUTOTUNE="0")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1", "--batch", "8", "--no-cpu-baseline",
           "--no-instrument", "--no-other-workloads"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 1 and d["config"]["parallelism"] == "dp1" and "reporting n_gpus=1" in r.stderr


# ---- the RCCL backend itself (backend "nccl" == RCCL on ROCm), world size 1 on the one GPU of the box --------------------------------
def _rccl_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["ACT_GEMM_AUTOTUNE"] = "0"
    os.environ["ACT_OVERLAP_TEACHER"] = "1"
    os.environ["ACT_OVERLAP_DW"] = "1"
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    assert dist.get_backend() == "nccl"
    import act_amd.kernels as K
    import act_amd.models.act as AM
    assert K.OVERLAP_DW and AM._OVERLAP_TEACHER              # the three-stream schedule is what is under test
    from act_amd.tools.runner_pretrain import wrap_ddp
    ns = argparse.Namespace(local_rank=rank, use_gpu=True)
    model = _model(dev)
    ddp = wrap_ddp(model, ns)
    assert isinstance(ddp, torch.nn.parallel.DistributedDataParallel) and ddp.gradient_as_bucket_view
    losses, params = _trajectory(ddp, model, seed=123, data_seed=20, dev=dev)
    # a small bucket cap: many buckets -> many stream-ordered all-reduces interleaved with the auxiliary-stream weight gradients
    model3 = _model(dev)
    ddp3 = torch.nn.parallel.DistributedDataParallel(model3, device_ids=[0], broadcast_buffers=False, gradient_as_bucket_view=True,
                                                     bucket_cap_mb=0.05)
    losses3, params3 = _trajectory(ddp3, model3, seed=123, data_seed=20, dev=dev)
    # the logged-loss reduction of the runner (utils/dist_utils.py:41-48) through RCCL
    from act_amd.utils import dist_utils
    red = dist_utils.reduce_tensor(losses.to(dev), argparse.Namespace(world_size=world))
    torch.cuda.synchronize()
    torch.save({"losses": losses, "params": params, "losses3": losses3, "params3": params3, "reduced": red.cpu()},
               os.path.join(out_dir, f"n{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_product_model_under_rccl_ddp_world1_is_bit_identical(tmp_path):
    """backend='nccl' (RCCL) at world size 1: process-group initialisation over RCCL, the bucket views, the hook plumbing of wrap_ddp and the
    runner's loss reduction.  It does NOT exercise stream ordering: RCCL launches no kernel for a one-rank in-place all-reduce (profiles/README.md),
    so nothing reads a bucket here -- the test that does is test_ddp_buckets_are_final_when_a_stream_ordered_reader_takes_them below.
    4 pipelined AdamW steps through wrap_ddp must equal the _Single run bit for bit, with the default 25 MB buckets and with 50 KB buckets
    (reference: tools/runner_pretrain.py:84-93,159-167)."""
    assert torch.cuda.is_available()
    from act_amd.tools.runner_pretrain import _Single
    dev = torch.device("cuda:0")
    port = 27500 + (os.getpid() % 2000)
    mp.spawn(_rccl_worker, args=(1, port, str(tmp_path)), nprocs=1, join=True)
    r = torch.load(tmp_path / "n0.pt")
    with _fixed_gemm_configs():
        model = _model(dev)
        losses, params = _trajectory(_Single(model), model, seed=123, data_seed=20, dev=dev)
    assert len(set(losses.tolist())) == STEPS
    for tag in ("", "3"):
        assert torch.equal(r["losses" + tag], losses), (tag, r["losses" + tag], losses)
        for n, p in params.items():
            assert torch.equal(r["params" + tag][n], p), (tag, n)
    assert torch.equal(r["reduced"], losses)


# ---- a comm hook that READS every bucket the way RCCL would: on its own stream, ordered after the hook's current stream by ONE event ----------------
def _hook_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["ACT_GEMM_AUTOTUNE"] = "0"
    os.environ["ACT_OVERLAP_TEACHER"] = "1"
    os.environ["ACT_OVERLAP_DW"] = "1"
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    import act_amd.kernels as K
    import act_amd.models.act as AM
    assert K.OVERLAP_DW and AM._OVERLAP_TEACHER              # auxiliary stream 0 (teacher prefetch) and 1 (weight gradients) are live
    from act_amd.tools import builder
    from act_amd.tools.runner_pretrain import train_step
    report = {}
    for tag, cap in (("25mb", 25), ("50kb", 0.05)):
        model = _model(dev)
        ddp = torch.nn.parallel.DistributedDataParallel(model, device_ids=[0], broadcast_buffers=False, gradient_as_bucket_view=True,
                                                         bucket_cap_mb=cap, find_unused_parameters=False)
        side = torch.cuda.Stream()
        taken = []                                           # (step, bucket index, parameter names, device copy made on `side`)
        names = {id(p): n for n, p in model.named_parameters()}
        step_no = [0]

        def hook(state, bucket):
            buf = bucket.buffer()
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())           # what RCCL does: its stream waits for the stream the hook runs on -- and for nothing else
            side.wait_event(ev)
            with torch.cuda.stream(side):
                snap = buf.clone()
            taken.append((step_no[0], bucket.index(), [names[id(p)] for p in bucket.parameters()], snap))
            fut = torch.futures.Future()
            fut.set_result(buf)
            return fut

        ddp.register_comm_hook(None, hook)
        cfg = _cfg()
        opt, _ = builder.build_opti_sche(ddp, cfg)
        finals = {}

        def before_step(optimizer, args, kwargs):            # every stream drained: these ARE the final gradients of the step
            torch.cuda.synchronize()
            finals[step_no[0]] = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

        opt.register_step_pre_hook(before_step)
        torch.manual_seed(123)
        pts = _batches(20, dev)
        losses = []
        for i in range(STEPS):
            step_no[0] = i
            nxt = pts[i + 1] if i + 1 < STEPS else None
            losses.append(train_step(ddp, opt, pts[i], cfg, next_points=nxt))
        torch.cuda.synchronize()
        bad, nb = [], 0
        for step, idx, pnames, snap in taken:
            want = torch.cat([finals[step][n].reshape(-1) for n in pnames])
            nb += 1
            if snap.numel() != want.numel() or not torch.equal(snap, want):
                bad.append((step, idx, pnames[:3]))
        report[tag] = {"buckets": nb, "bad": bad, "steps": sorted(finals), "losses": torch.stack(losses).cpu(),
                       "params": {n: p.detach().clone().cpu() for n, p in model.named_parameters()}}
    torch.save(report, os.path.join(out_dir, "hook.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_ddp_buckets_are_final_when_a_stream_ordered_reader_takes_them(tmp_path):
    """The hazard the world-1 RCCL test cannot observe.  DDP hands a gradient bucket to its communication hook as soon as autograd has produced
    the bucket's last gradient; RCCL then reads the bucket on ITS stream, ordered after the hook's current stream by one event.  The student's
    weight-gradient GEMMs run on auxiliary stream 1 and the teacher prefetch on auxiliary stream 0 -- if a block's backward returned before
    joining stream 1, the reader would see a stale bucket.  Here the hook is that reader: a device copy of bucket.buffer() on a side stream behind
    one event, the bucket returned unchanged.  Over 4 pipelined AdamW steps (ACT_OVERLAP_TEACHER=1, ACT_OVERLAP_DW=1), with 25 MB and with
    50 KB buckets, every copy must equal the step's final gradients (taken after a device-wide synchronise, before optimizer.step) bit for bit,
    and the trajectory must equal the _Single run (reference: tools/runner_pretrain.py:84-93, utils/dist_utils.py:9-24)."""
    assert torch.cuda.is_available()
    from act_amd.tools.runner_pretrain import _Single
    dev = torch.device("cuda:0")
    port = 25500 + (os.getpid() % 2000)
    mp.spawn(_hook_worker, args=(1, port, str(tmp_path)), nprocs=1, join=True)
    r = torch.load(tmp_path / "hook.pt")
    with _fixed_gemm_configs():
        model = _model(dev)
        losses, params = _trajectory(_Single(model), model, seed=123, data_seed=20, dev=dev)
    for tag in ("25mb", "50kb"):
        assert r[tag]["steps"] == list(range(STEPS))
        assert r[tag]["buckets"] >= STEPS and not r[tag]["bad"], (tag, r[tag]["buckets"], r[tag]["bad"][:5])
        assert torch.equal(r[tag]["losses"], losses), tag
        for n, p in params.items():
            assert torch.equal(r[tag]["params"][n], p), (tag, n)
    assert r["50kb"]["buckets"] > r["25mb"]["buckets"]              # the small cap really produced more buckets per step
