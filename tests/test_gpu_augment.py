"""GPU: the fused augmentation chain (csrc/augment.hip, act_augment_f32) against its host restatement (tests/augment_ref.py, itself pinned to the
reference's transforms by tests/test_augment_host.py) with injected draws, against the reference's recorded outputs, LDS path against global path,
the in-kernel Philox draws against their host restatement, the argument checks, and the ``train_transforms`` key of the two runners.

Bars.  Scale, translate, scale-and-translate, dropout, flip, and jitter with injected normals are one or two correctly rounded fp32 operations
per coordinate: bit-exact.  Rotate: 2e-6 absolute (coordinates at or below 2 in magnitude, two products of ~1.2e-7 relative error each; the device
and the restatement round the sine and cosine differently).  A chain that holds a rotation is held to the same 2e-6 as a whole, and chains without
one stay bit-exact."""
import argparse
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import augment_ref as AR
from tests.golden.fill import clouds, TINY_STAGE2, TINY_FINETUNE
from tests.augment_ref import GOLD, GOLDEN_OPS, ROTATE_ATOL, check_against_golden

pytestmark = pytest.mark.gpu

D3 = (0., 0., 0.)
ST, SC, TR = (AR.SCALE_TRANSLATE, 2. / 3., 1.5, 0.2), (AR.SCALE, 2. / 3., 1.5, 0.), (AR.TRANSLATE, 0.2, 0., 0.)
ROT, JIT, DROP = (AR.ROTATE_Y,) + D3, (AR.JITTER, 0.01, 0.05, 0.), (AR.DROPOUT, 0.5, 0., 0.)
FLIP = lambda axis: (AR.FLIP, float(axis), 0., 0.)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def make_draws(ops, B, N, seed):
    """numpy draws for a chain, in the injectable form (what the reference would draw: uniforms in their ranges, standard normals)"""
    rs = np.random.RandomState(seed)
    f = lambda a: np.asarray(a, dtype=np.float32)
    out = []
    for kind, p0, p1, p2 in ops:
        if kind == AR.SCALE:
            out.append((f(rs.uniform(p0, p1, (B, 3))),))
        elif kind == AR.TRANSLATE:
            out.append((f(rs.uniform(-p0, p0, (B, 3))),))
        elif kind == AR.SCALE_TRANSLATE:
            out.append((f(rs.uniform(p0, p1, (B, 3))), f(rs.uniform(-p2, p2, (B, 3)))))
        elif kind == AR.ROTATE_Y:
            out.append((f(rs.random_sample(B)),))
        elif kind == AR.JITTER:
            out.append((f(rs.standard_normal((B, N, 3))),))
        elif kind == AR.DROPOUT:
            out.append((f(rs.random_sample(B)), f(rs.random_sample((B, N)))))
        elif kind == AR.FLIP:
            out.append((f(rs.random_sample((B, 3)) * [0.9, 1, 1]),))          # gate open: the flip cases have a test of their own
    return out


def run(dev, pc, ops, draws=None, **kw):
    import act_amd.kernels as K
    t = torch.from_numpy(np.ascontiguousarray(pc)).to(dev)
    d = None if draws is None else [tuple(None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in op) for op in draws]
    out = K.augment(t, ops, d, **kw)
    assert out is t
    return t.cpu().numpy()


def chain_atol(ops, draws=None):
    """bit-exact without a rotation, else the rotation's 2e-6"""
    return ROTATE_ATOL if any(op[0] == AR.ROTATE_Y for op in ops) else 0.0


def check(got, want, atol, what=""):
    err = float(np.abs(got.astype(np.float64) - want).max()) if got.size else 0.0
    print(f"{what}: max abs error {err:.3e} (bar {atol:.1e})")
    if atol == 0.0:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what
    else:
        assert err <= atol, what


# ---- each op alone ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1024])
@pytest.mark.parametrize("op", [SC, TR, ST, ROT, JIT, DROP, FLIP(0), FLIP(1), FLIP(2)], ids=lambda o: f"kind{o[0]}_{int(o[1] * 10)}")
def test_each_op_alone(dev, op, N):
    pc = clouds(31, 3, N) if N > 1 else np.array([[[.3, -.2, .9]], [[-1., .5, 0.]], [[.1, .2, .3]]], np.float32)
    draws = make_draws([op], 3, N, 100 + N)
    check(run(dev, pc, [op], draws), AR.apply(pc, [op], draws), chain_atol([op], draws), f"kind {op[0]} N {N}")


@pytest.mark.parametrize("name", sorted(GOLDEN_OPS))
def test_reference_golden(dev, name):
    g = np.load(GOLD)
    op, keys = GOLDEN_OPS[name]
    got = run(dev, g["pc"], [op], [tuple(g[k].astype(np.float32) for k in keys)])
    check_against_golden(name, got, g[name + "_out"])


# ---- order inside a chain -----------------------------------------------------------------------------------------------------------------
def test_flip_takes_its_maximum_at_its_position(dev):
    pc = clouds(32, 3, 257)
    u, fl = np.array([.1, .3, .7], np.float32), np.array([[0., 0., 1.], [0., 0., 0.], [.5, 1., .2]], np.float32)
    a = run(dev, pc, [ROT, FLIP(1)], [(u,), (fl,)])
    b = run(dev, pc, [FLIP(1), ROT], [(fl,), (u,)])
    assert np.abs(a - b).max() > 1e-2
    check(a, AR.apply(pc, [ROT, FLIP(1)], [(u,), (fl,)]), ROTATE_ATOL, "rotate, flip")
    check(b, AR.apply(pc, [FLIP(1), ROT], [(fl,), (u,)]), ROTATE_ATOL, "flip, rotate")


def test_dropout_copies_the_transformed_point_0(dev):
    pc = clouds(33, 2, 65)
    sc, sh = np.array([[1.5, .7, 1.1], [.9, 1.2, .8]], np.float32), np.array([[.1, -.2, .05], [0., .15, -.1]], np.float32)
    ratio, du = np.array([1.9, .5], np.float32), np.full((2, 65), .5, np.float32)      # cloud 0: ratio .95 drops all; cloud 1: ratio .25 drops none
    got = run(dev, pc, [ST, DROP], [(sc, sh), (ratio, du)])
    assert np.array_equal(got[0], np.broadcast_to(pc[0, :1] * sc[0] + sh[0], (65, 3)))
    assert np.array_equal(got[1], pc[1] * sc[1] + sh[1])
    check(got, AR.apply(pc, [ST, DROP], [(sc, sh), (ratio, du)]), 0.0, "scale-translate, dropout")


# ---- dropout edges ----------------------------------------------------------------------------------------------------------------------
def test_dropout_edges(dev):
    B, N = 3, 257
    pc = clouds(34, B, N)
    ratio = np.array([0., .6, 1.98], np.float32)              # cloud 0: ratio == 0; cloud 1: point 0 among the dropped; cloud 2: ratio .99 drops all
    du = np.random.RandomState(3).uniform(.995, 1., (B, N)).astype(np.float32)
    du[0, 200] = 0.0                                          # `<=`: an exact 0.0 under ratio == 0 is dropped, and nothing else is
    du[1, [0, 5, 64, 256]] = [.1, .2, .3, .3]
    du[2] = np.random.RandomState(4).uniform(0., .98, N)
    got = run(dev, pc, [DROP], [(ratio, du)])
    want0 = pc[0].copy(); want0[200] = pc[0, 0]
    want1 = pc[1].copy(); want1[[5, 64, 256]] = pc[1, 0]
    assert np.array_equal(got[0], want0) and np.array_equal(got[1], want1) and np.array_equal(got[2], np.broadcast_to(pc[2, :1], (N, 3)))
    check(got, AR.apply(pc, [DROP], [(ratio, du)]), 0.0, "dropout edges")


# ---- flip -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_flip_cases(dev, axis):
    N = 65
    fl = np.array([[.96, 0., 0.], [.949, .5, .5], [0., .49, .5], [0., .5, .49], [.5, .1, .2], [.95, .1, .1]], np.float32)
    pc = clouds(35, len(fl), N)
    got = run(dev, pc, [FLIP(axis)], [(fl,)])
    h0, h1 = [a for a in range(3) if a != axis]
    flipped = lambda b, ax: pc[b, :, ax].max() - pc[b, :, ax]
    for b, (first, second) in enumerate([(0, 0), (0, 0), (1, 0), (0, 1), (1, 1), (0, 0)]):       # gate closed, neither, first, second, both, gate at 0.95
        assert np.array_equal(got[b, :, axis], pc[b, :, axis])
        assert np.array_equal(got[b, :, h0], flipped(b, h0) if first else pc[b, :, h0]), (b, "first")
        assert np.array_equal(got[b, :, h1], flipped(b, h1) if second else pc[b, :, h1]), (b, "second")
    check(got, AR.apply(pc, [FLIP(axis)], [(fl,)]), 0.0, f"flip upright {axis}")


# ---- whole chains -----------------------------------------------------------------------------------------------------------------------
CHAIN7 = [ST, ROT, JIT, DROP, FLIP(1), SC, TR]
CHAIN8 = [JIT, ST, DROP, FLIP(2), ROT, DROP, FLIP(0), JIT]


@pytest.mark.parametrize("ops", [CHAIN7, CHAIN8], ids=["seven_ops", "eight_ops_repeated"])
def test_full_chains(dev, ops):
    pc = clouds(36, 3, 1024)
    draws = make_draws(ops, 3, 1024, 36)
    check(run(dev, pc, ops, draws), AR.apply(pc, ops, draws), chain_atol(ops, draws), f"{len(ops)} ops")


def test_lds_path_and_global_path(dev):
    """the same chain and draws through both paths at N = 8192 (the largest cloud staged in LDS) are the same bits; N = 8193 takes the global path"""
    pc = clouds(37, 2, 8192)
    draws = make_draws(CHAIN7, 2, 8192, 37)
    a, b = run(dev, pc, CHAIN7, draws), run(dev, pc, CHAIN7, draws, force_global=True)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    check(a, AR.apply(pc, CHAIN7, draws), chain_atol(CHAIN7, draws), "N 8192")
    pc = clouds(38, 2, 8193)
    draws = make_draws(CHAIN7, 2, 8193, 38)
    check(run(dev, pc, CHAIN7, draws), AR.apply(pc, CHAIN7, draws), chain_atol(CHAIN7, draws), "N 8193")
    small = clouds(39, 3, 65)                                  # and the forced global path at a small N, partial waves
    draws = make_draws(CHAIN8, 3, 65, 39)
    assert np.array_equal(run(dev, small, CHAIN8, draws), run(dev, small, CHAIN8, draws, force_global=True))


# ---- Philox -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr", [None, 5])
def test_seeded_run_is_the_host_restated_stream(dev, ctr):
    B, N, seed = 3, 257, 0x1234567890ABCDEF
    pc = clouds(40, B, N)
    seed_dev = None if ctr is None else torch.tensor([ctr], dtype=torch.int64, device=dev)
    for op in (SC, TR, ST, DROP, FLIP(0), FLIP(2), ROT):
        ops = [TR, op]                                         # (position 1: the position is part of the counter)
        host = AR.philox_draws(ops, B, N, seed, ctr)
        check(run(dev, pc, ops, None, seed=seed, seed_dev=seed_dev), AR.apply(pc, ops, host), chain_atol(ops, host), f"seeded kind {op[0]}")
    # jitter: the term itself, on a zero cloud (0 + t == t): 1e-6 for std <= 0.05 (|z| <= 5.9; the device's log / sincospi against float64)
    zero = np.zeros((B, N, 3), np.float32)
    for std, clip in ((0.01, 0.05), (0.05, 1.0)):
        ops = [(AR.JITTER, std, clip, 0.)]
        got = run(dev, zero, ops, None, seed=seed, seed_dev=seed_dev)
        check(got, AR.apply(zero, ops, AR.philox_draws(ops, B, N, seed, ctr)), 1e-6, f"seeded jitter std {std}")
        assert np.abs(got).max() > 2 * std                    # (draws, not zeros)


def test_seed_and_counter(dev):
    B, N = 3, 257
    pc = clouds(41, B, N)
    ctr = torch.tensor([7], dtype=torch.int64, device=dev)
    a = run(dev, pc, CHAIN7, None, seed=11, seed_dev=ctr)
    assert np.array_equal(a, run(dev, pc, CHAIN7, None, seed=11, seed_dev=ctr))
    assert not np.array_equal(a, run(dev, pc, CHAIN7, None, seed=12, seed_dev=ctr))
    assert not np.array_equal(a, run(dev, pc, CHAIN7, None, seed=11, seed_dev=ctr + 1))
    assert not np.array_equal(a, run(dev, pc, CHAIN7, None, seed=11))
    # two jitters of one chain draw different noise (the position is in the counter), and no jitter exceeds its clip
    zero = np.zeros((B, N, 3), np.float32)
    one = run(dev, zero, [(AR.JITTER, .05, .05, 0.)], None, seed=3)
    assert np.abs(one).max() == np.float32(.05) and (np.abs(one) == np.float32(.05)).mean() > .2     # std == clip: a third of the draws are clipped
    two = run(dev, zero, [(AR.JITTER, .05, .05, 0.), (AR.JITTER, .05, .05, 0.)], None, seed=3)
    assert not np.array_equal(two, one + one) and np.abs(two).max() <= np.float32(.1)


def test_capturable_in_a_graph(dev):
    """no allocation, no copy, the table by value: the launch replays from a captured graph, and the device-resident counter renews its draws"""
    import act_amd.kernels as K
    pc0 = torch.from_numpy(clouds(42, 3, 257)).to(dev)
    buf, ctr = pc0.clone(), torch.zeros(1, dtype=torch.int64, device=dev)
    ops = [ST, DROP, FLIP(1), JIT]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.augment(buf, ops, None, seed=9, seed_dev=ctr)       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.augment(buf, ops, None, seed=9, seed_dev=ctr)
    outs = []
    for step in (0, 1):
        buf.copy_(pc0); ctr.fill_(step)
        g.replay()
        outs.append(buf.cpu().numpy())
        check(outs[-1], AR.apply(pc0.cpu().numpy(), ops, AR.philox_draws(ops, 3, 257, 9, step)), 1e-6, f"replay {step}")       # the jitter term's bar; the ops before it are bit-exact
    assert not np.array_equal(outs[0], outs[1])


# ---- the classes ------------------------------------------------------------------------------------------------------------------------
def test_compose_against_the_two_existing_classes(dev):
    from act_amd.datasets import data_transforms as DT
    pc = torch.from_numpy(clouds(43, 3, 257)).to(dev)
    sc = torch.from_numpy(np.random.RandomState(1).uniform(2 / 3, 1.5, (3, 3)).astype(np.float32)).to(dev)
    sh = torch.from_numpy(np.random.RandomState(2).uniform(-.2, .2, (3, 3)).astype(np.float32)).to(dev)
    u = torch.tensor([.1, .45, .8], device=dev)
    a = DT.Compose([DT.PointcloudScaleAndTranslate()])(pc.clone(), draws={"0.scale": sc, "0.shift": sh})
    assert torch.equal(a, DT.PointcloudScaleAndTranslate()(pc.clone(), scale=sc, shift=sh))
    b = DT.Compose([DT.PointcloudRotate()])(pc.clone(), draws={"0.u": u})
    check(b.cpu().numpy(), DT.PointcloudRotate()(pc.clone(), u=u).cpu().numpy(), ROTATE_ATOL, "Compose rotate against PointcloudRotate")
    both = DT.Compose([DT.PointcloudScaleAndTranslate(), DT.PointcloudRotate()])(pc.clone(), draws={"0.scale": sc, "0.shift": sh, "1.u": u})
    check(both.cpu().numpy(), DT.PointcloudRotate()(a.clone(), u=u).cpu().numpy(), ROTATE_ATOL, "Compose of both")
    with pytest.raises(KeyError):
        DT.Compose([DT.PointcloudRotate()])(pc.clone(), draws={"1.u": u})


def test_single_classes_are_one_op_chains(dev):
    from act_amd.datasets import data_transforms as DT
    B, N = 3, 65
    pc = clouds(44, B, N)
    t = lambda a: torch.from_numpy(a).to(dev)
    cases = [(DT.PointcloudJitter(0.02, 0.03), (AR.JITTER, .02, .03, 0.), ("noise",)), (DT.PointcloudScale(.5, 2.), (AR.SCALE, .5, 2., 0.), ("scale",)),
             (DT.PointcloudTranslate(.3), (AR.TRANSLATE, .3, 0., 0.), ("shift",)),
             (DT.PointcloudRandomInputDropout(.7), (AR.DROPOUT, .7, 0., 0.), ("ratio", "drop_u")), (DT.RandomHorizontalFlip('x'), FLIP(0), ("flip_u",))]
    for obj, op, names in cases:
        draws = make_draws([op], B, N, 44)
        x = t(pc)
        out = obj(x, **{n: t(d) for n, d in zip(names, draws[0])})
        assert out is x
        check(out.cpu().numpy(), AR.apply(pc, [op], draws), 0.0, type(obj).__name__)
        torch.manual_seed(5); a = obj(t(pc)).cpu().numpy()            # no draws given: a seed from torch's generator
        torch.manual_seed(5); b = obj(t(pc)).cpu().numpy()
        assert np.array_equal(a, b) and a.shape == pc.shape and np.isfinite(a).all()
    with pytest.raises(RuntimeError):
        DT.PointcloudJitter()(torch.from_numpy(pc))                   # a CPU tensor: no fall-back


# ---- argument checks ------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(dev):
    import act_amd._C as C
    from act_amd._abi import AugmentOp
    pc = torch.from_numpy(clouds(45, 2, 65)).to(dev)
    before = pc.clone()

    def call(ops, B=2, N=65, nops=None, flags=0, p=pc):
        table = (AugmentOp * max(1, len(ops)))()
        for i, (k, a, b, c) in enumerate(ops):
            table[i].kind, table[i].p0, table[i].p1, table[i].p2 = k, a, b, c
        return C.lib.act_augment_f32(C.ptr(p) if p is not None else None, B, N, table, len(ops) if nops is None else nops, 1, None, flags, C.stream())
    bad = [[(0,) + D3], [(8,) + D3], [(-1,) + D3], [(AR.SCALE, 1.5, 1., 0.)], [(AR.SCALE_TRANSLATE, 1.5, 1., .2)], [(AR.SCALE_TRANSLATE, 1., 1.5, -.2)],
           [(AR.TRANSLATE, -.1, 0., 0.)], [(AR.JITTER, -.01, .05, 0.)], [(AR.JITTER, .01, -.05, 0.)], [(AR.DROPOUT, -.1, 0., 0.)],
           [(AR.DROPOUT, 1., 0., 0.)], [(AR.DROPOUT, 1.5, 0., 0.)], [(AR.FLIP, 3., 0., 0.)], [(AR.FLIP, -1., 0., 0.)], [(AR.FLIP, .5, 0., 0.)],
           [TR, (AR.SCALE, float("nan"), 1., 0.)], [TR, TR, TR, TR, TR, TR, TR, (9,) + D3]]
    for ops in bad:
        assert call(ops) == -1, ops                            # ACT_E_BADARG
        assert call(ops, B=0) == -1 and call(ops, p=None) == -1, ops          # arguments first, the empty batch and the pointers after them
    assert call([TR], nops=0) == -1 and call([TR], nops=9) == -1 and call([TR], nops=-1) == -1
    assert call([TR], flags=2) == -1 and call([TR], B=-1) == -1 and call([TR], N=-1) == -1
    assert call([TR], p=None) == -2                            # ACT_E_NULLPTR
    assert call([TR], B=0) == 0 and call([TR], N=0) == 0 and call([TR], B=0, p=None) == 0 and call([TR], N=0, p=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(pc, before)                             # nothing above launched
    assert call([(AR.SCALE, 1., 1., 0.), (AR.DROPOUT, 0., 0., 0.), (AR.JITTER, 0., 0., 0.), (AR.TRANSLATE, 0., 0., 0.)]) == 0    # the closed ends are legal ...
    torch.cuda.synchronize()
    assert torch.equal(pc, before)                             # ... and are the identity (ratio 0 < every 24-bit uniform but an exact 0: none here, seed 1)
    import act_amd.kernels as K
    empty = torch.empty(0, 65, 3, device=dev)
    assert K.augment(empty, [TR]) is empty
    with pytest.raises(C.ActHipError):
        K.augment(pc, [TR], [(torch.zeros(2, 4, device=dev),)])               # a draw of the wrong shape never reaches the kernel


# ---- runners ----------------------------------------------------------------------------------------------------------------------------
def _args(tmp, **kw):
    a = argparse.Namespace(log_name="test_aug", use_gpu=True, local_rank=0, distributed=False, sync_bn=False, resume=False, start_ckpts=None,
                           ckpts=None, experiment_path=str(tmp), num_workers=0, world_size=1, val_freq=1, vote=False)
    a.__dict__.update(kw)
    return a


def _tiny(cfg, model, bs, **base):
    """the recipe as shipped -- its chain, optimizer, scheduler, dataset kinds -- at a size a test can afford: the tiny model of the goldens, a
    small synthetic set"""
    from act_amd.utils.config import EasyDict
    cfg.model = EasyDict(copy.deepcopy(model))
    for split in cfg.dataset.values():
        split._base_.update(NUM_SAMPLES=4 * bs, **base)
        split.others.bs = bs
    cfg.total_bs = bs
    return cfg


def test_run_net_of_the_pretrain_recipe(tmp_path, dev):
    from act_amd.tools import runner_pretrain as RP
    from act_amd.datasets import data_transforms as DT
    from act_amd.utils.config import cfg_from_yaml_file
    assert type(RP.train_transforms) is DT.PointcloudScaleAndTranslate         # the key absent: the module-level object, as before
    cfg = _tiny(cfg_from_yaml_file("cfgs/synthetic/pretrain_act_distill_aug.yaml"), TINY_STAGE2, 8)
    for split in cfg.dataset.values():
        split.others.npoints = 128
    assert len(cfg.train_transforms) == 5
    torch.manual_seed(0)
    log = RP.run_net(_args(tmp_path), cfg, max_steps=3, log_every=1)
    assert len(log) == 3 and np.isfinite(log).all()
    assert type(RP.train_transforms) is DT.PointcloudScaleAndTranslate


def test_run_net_of_the_finetune_recipe(tmp_path, dev):
    from act_amd.tools import runner_finetune as RF
    from act_amd.utils.config import cfg_from_yaml_file
    cfg = _tiny(cfg_from_yaml_file("cfgs/synthetic/finetune_modelnet_aug.yaml"), dict(TINY_FINETUNE, cls_dim=4, num_group=32, group_size=16), 8,
                NUM_CATEGORY=4, N_POINTS=2048)
    assert len(cfg.train_transforms) == 5 and cfg.npoints == 1024
    torch.manual_seed(0); np.random.seed(0)
    log = RF.run_net(_args(tmp_path), cfg, max_steps=3, log_every=1)
    assert len(log) == 3 and np.isfinite(np.array(log)).all()


def test_stage2_step_with_injected_chain_draws_is_deterministic(dev):
    """the same seeded Stage-II step twice, the Compose's draws injected: the loss and the updated weights are the same bits, and another set of
    draws gives another loss (the chain does reach the model)"""
    from act_amd.models import build_model_from_cfg
    from act_amd.tools import builder
    from act_amd.tools.runner_pretrain import train_step, freeze_unused_heads, _Single
    from act_amd.datasets import data_transforms as DT
    from act_amd.utils.config import EasyDict
    from tests.golden.fill import fill_module
    cfg = EasyDict(optimizer=dict(type="AdamW", kwargs=dict(lr=1e-3, weight_decay=0.05)), scheduler=dict(type="CosLR", kwargs=dict(epochs=300, initial_epochs=10)),
                   step_per_update=1)
    chain = DT.Compose([DT.PointcloudScaleAndTranslate(), DT.PointcloudRotate(), DT.PointcloudJitter(), DT.PointcloudRandomInputDropout(),
                        DT.RandomHorizontalFlip('y')])
    B, N = 4, 128
    pts = torch.from_numpy(clouds(46, B, N)).to(dev)
    names = [("scale", "shift"), ("u",), ("noise",), ("ratio", "drop_u"), ("flip_u",)]

    def step(draw_seed):
        d = make_draws([ST, ROT, JIT, DROP, FLIP(1)], B, N, draw_seed)
        inj = {f"{i}.{n}": torch.from_numpy(t).to(dev) for i, (ns, ts) in enumerate(zip(names, d)) for n, t in zip(ns, ts)}
        torch.manual_seed(0)
        model = fill_module(build_model_from_cfg(EasyDict(copy.deepcopy(TINY_STAGE2))), "g4.").to(dev).train()
        freeze_unused_heads(model)
        wrapped = _Single(model)
        opt, _ = builder.build_opti_sche(wrapped, cfg)
        torch.manual_seed(99)
        x = pts.clone()
        loss = train_step(wrapped, opt, x, cfg, transforms=chain, aug_draws=inj)
        assert not torch.equal(x, pts)                         # augmented in place
        return loss.cpu(), x.cpu(), model.ACT_encoder.blocks.blocks[0].attn.qkv.weight.detach().cpu()
    a, b, c = step(1), step(1), step(2)
    assert torch.isfinite(a[0]) and all(torch.equal(p, q) for p, q in zip(a, b))
    assert not torch.equal(a[1], c[1]) and not torch.equal(a[0], c[0])
