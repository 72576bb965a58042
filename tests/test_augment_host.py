"""CPU: the host restatement of the fused augmentation chain (tests/augment_ref.py, which the GPU tests of tests/test_gpu_augment.py lean on)
reproduces the reference's own seven transforms from their recorded draws (tests/golden/g22_transforms.npz, written by
tests/golden/make_golden_transforms.py), its Philox layout never reuses a counter inside a launch, and the Python surface is the reference's."""
import os

import numpy as np
import pytest

from tests import augment_ref as AR

GOLD, GOLDEN_OPS, check_against_golden, D3 = AR.GOLD, AR.GOLDEN_OPS, AR.check_against_golden, (0., 0., 0.)


def test_golden_holds_the_cases_it_was_made_for():
    g = np.load(GOLD)
    u = g["flip_u"]
    opened = (u[:, 0] < 0.95) & ((u[:, 1] < 0.5) != (u[:, 2] < 0.5))
    assert opened.any() and (u[:, 0] >= 0.95).any() and (u[u[:, 0] >= 0.95, 1:] == 1.0).all()
    dropped0 = g["dropout_drop_u"][:, 0] <= g["dropout_ratio"] * np.float32(0.5)
    assert dropped0.any() and not dropped0.all()
    assert g["pc"].shape == (2, 128, 3) and os.path.getsize(GOLD) < 64 * 1024
    for name in GOLDEN_OPS:
        assert not np.array_equal(g[name + "_out"], g["pc"]), name


@pytest.mark.parametrize("name", sorted(GOLDEN_OPS))
def test_restatement_reproduces_the_reference(name):
    g = np.load(GOLD)
    op, keys = GOLDEN_OPS[name]
    got = AR.apply(g["pc"], [op], [tuple(g[k] for k in keys)])
    check_against_golden(name, got, g[name + "_out"])


def test_philox_layout_never_reuses_a_counter():
    """distinct (cloud, position, slot) draw from distinct counters: B = 3, N = 65, a chain of 8 ops holding every kind (and one twice)"""
    B, N = 3, 65
    ops = [(AR.SCALE_TRANSLATE, .5, 2., .1), (AR.ROTATE_Y,) + D3, (AR.JITTER, .01, .05, 0.), (AR.DROPOUT, .5, 0., 0.), (AR.FLIP, 1., 0., 0.),
           (AR.SCALE, .5, 2., 0.), (AR.TRANSLATE, .2, 0., 0.), (AR.JITTER, .02, .05, 0.)]
    log = []
    draws = AR.philox_draws(ops, B, N, seed=1234, log=log)
    # per cloud: 2 + 1 + 0 + 1 + 1 + 1 + 1 + 0 per-cloud counters and N per-point counters for each jitter / dropout
    assert len(log) == B * (7 + 3 * N) and len(set(log)) == len(log)
    assert all(c[2] == 3 for c in log)                                        # the domain word: 0, 1, 2 belong to gumbel noise and the two dropouts
    st, rot, jit, drop, flip, sc, tr, jit2 = draws
    assert st[0].shape == (B, 3) and st[1].shape == (B, 3) and not np.array_equal(st[0], sc[0])
    assert (st[0] >= .5).all() and (st[0] <= 2.).all() and (np.abs(tr[0]) <= .2).all() and (np.abs(st[1]) <= .1).all()
    assert rot[0].shape == (B,) and jit[0].shape == (B, N, 3) and drop[0].shape == (B,) and drop[1].shape == (B, N) and flip[0].shape == (B, 3)
    for u in (rot[0], drop[0], drop[1], flip[0]):
        assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    assert np.abs(jit[0]).max() <= 5.9 and not np.array_equal(jit[0], jit2[0])
    # a large sample of the normals has the moments of N(0, 1)
    z = AR.philox_draws([(AR.JITTER, .01, .05, 0.)], 4, 4096, seed=7)[0][0].astype(np.float64)
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02
    # the step counter and the seed both move the draws
    a = AR.philox_draws(ops[:2], B, N, 5)
    assert not np.array_equal(a[0][0], AR.philox_draws(ops[:2], B, N, 6)[0][0])
    assert not np.array_equal(a[0][0], AR.philox_draws(ops[:2], B, N, 5, ctr=1)[0][0])
    assert np.array_equal(a[0][0], AR.philox_draws(ops[:2], B, N, 5, ctr=0)[0][0])


def test_restatement_order_matters():
    """the flip takes its maximum, and the dropout its point 0, from the cloud as the earlier ops left it"""
    g = np.load(GOLD)
    pc = g["pc"]
    u, fl = np.array([0.1, 0.3], np.float32), np.array([[0., 0., 1.], [0., 0., 0.]], np.float32)
    rot, flip = (AR.ROTATE_Y,) + D3, (AR.FLIP, 1., 0., 0.)
    a, b = AR.apply(pc, [rot, flip], [(u,), (fl,)]), AR.apply(pc, [flip, rot], [(fl,), (u,)])
    assert np.abs(a - b).max() > 1e-2
    st = (AR.SCALE_TRANSLATE, .5, 2., .2)
    sc, sh = np.full((2, 3), 1.5, np.float32), np.full((2, 3), 0.25, np.float32)
    out = AR.apply(pc, [st, (AR.DROPOUT, .5, 0., 0.)], [(sc, sh), (np.array([1.9, 0.], np.float32), np.full((2, 128), .5, np.float32))])
    assert np.array_equal(out[0], np.broadcast_to(pc[0, :1] * np.float32(1.5) + np.float32(0.25), (128, 3)))     # every point of cloud 0: the transformed point 0
    assert np.array_equal(out[1], pc[1] * np.float32(1.5) + np.float32(0.25))                                    # ratio 0, no draw at 0: none


def test_python_surface():
    """the reference's seven names, arguments and defaults; Compose type-checks its members; 4-D temporal coordinates are refused"""
    from act_amd.datasets import data_transforms as DT
    for n in ("PointcloudRotate", "PointcloudScaleAndTranslate", "PointcloudJitter", "PointcloudScale", "PointcloudTranslate",
              "PointcloudRandomInputDropout", "RandomHorizontalFlip", "Compose"):
        assert hasattr(DT, n), n
    j, s, t, d, f = DT.PointcloudJitter(), DT.PointcloudScale(), DT.PointcloudTranslate(), DT.PointcloudRandomInputDropout(), DT.RandomHorizontalFlip()
    assert (j.std, j.clip) == (0.01, 0.05) and (s.scale_low, s.scale_high) == (2. / 3., 3. / 2.) and t.translate_range == 0.2
    assert d.max_dropout_ratio == 0.5 and f.upright_axis == 2 and DT.RandomHorizontalFlip('X').upright_axis == 0
    with pytest.raises(AssertionError):
        DT.PointcloudRandomInputDropout(1.0)
    with pytest.raises(ValueError):
        DT.RandomHorizontalFlip(is_temporal=True)
    chain = DT.Compose([DT.PointcloudScaleAndTranslate(), DT.PointcloudRotate(), j, d, f])
    assert len(chain.transforms) == 5
    with pytest.raises(TypeError):
        DT.Compose([DT.PointcloudRotate(), lambda pc: pc])
    with pytest.raises(ValueError):
        DT.Compose([j] * 9)
    with pytest.raises(ValueError, match="PointcloudJitter.*RandomHorizontalFlip"):
        DT.build_transforms([dict(NAME="PointcloudRotatePerturbation")])
    built = DT.build_transforms([dict(NAME="PointcloudJitter", std=0.02), dict(NAME="RandomHorizontalFlip", upright_axis="y")])
    assert built.transforms[0].std == 0.02 and built.transforms[1].upright_axis == 1


def test_recipes_carry_the_chain_and_the_runners_default_is_unchanged():
    from act_amd.datasets import data_transforms as DT
    from act_amd.tools import runner_pretrain as RP, runner_finetune as RF
    from act_amd.utils.config import cfg_from_yaml_file
    assert type(RP.train_transforms) is DT.PointcloudScaleAndTranslate and type(RF.train_transforms) is DT.PointcloudRotate
    assert RP.transforms_from_config(cfg_from_yaml_file("cfgs/synthetic/pretrain_act_distill.yaml")) is None
    for f in ("cfgs/synthetic/pretrain_act_distill_aug.yaml", "cfgs/synthetic/finetune_modelnet_aug.yaml"):
        chain = RP.transforms_from_config(cfg_from_yaml_file(f))
        assert [type(t).__name__ for t in chain.transforms] == ["PointcloudScaleAndTranslate", "PointcloudRotate", "PointcloudJitter",
                                                                "PointcloudRandomInputDropout", "RandomHorizontalFlip"]
