"""GPU: three-NN feature propagation at any size -- the search, its inverse adjacency and the interpolation with skipped slots (csrc/sa.hip),
the upstream-form ops over them, ``PointNetFeaturePropagationAny`` against the reference's recorded run
(tests/golden/g26_fp.npz), the three PointNet++ networks against their float64 restatement (tests/fp_ref.py) and the runners' model switch.

The search is compared index for index and bit for bit: the clouds sit on the 1/8 lattice, where every squared distance is exact in float32,
so the restatement (checked on the host against the reference's run and against tests/seg_ref.py) is an exact oracle, duplicated points and
equal distances included.  Sizes: one lane per unknown point in blocks of 256 (n = 255, 256, 257), the known cloud in LDS tiles of 1024 points
(m one below, at, one above a tile, and past two tiles), the m < 3 forms, and m on both sides of the switch between the two adjacency builders
(one launch at m <= 256, three launches above; m = 512 / 513 straddled the former limit of the Transformer head's search)."""
import copy
import re

import numpy as np
import pytest
import torch

from tests import fp_ref as R
from tests import sa_ref as SR
from tests.conftest import golden
from tests.golden.fill import fill_module, fill_tensor

pytestmark = pytest.mark.gpu

TOL = 1e-4
TILE = 1024                     # SA_NN_TILE of csrc/sa.hip


def _rel(a, ref):
    a, ref = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return ((a - ref).abs().max() / max(1.0, ref.abs().max())).item()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def K(dev):
    import act_amd.kernels as K
    return K


@pytest.fixture(scope="module")
def pu(dev):
    from act_amd.pointnet2_ops import pointnet2_utils as pu
    return pu


@pytest.fixture(scope="module")
def g():
    return golden("g26_fp")


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _check_search(K, dev, u, k):
    """idx, d2, weights and adjacency of K.three_nn equal to the restatement, bit for bit; the pieces on request agree with the full call"""
    m = k.shape[1]
    idx, w, d2 = R.three_nn(u, k)
    off, ent = R.adjacency(idx, m)
    got = K.three_nn(_d(u, dev), _d(k, dev), want_adj=True, want_d2=True)
    assert [t.dtype for t in got] == [torch.int32, torch.float32, torch.int32, torch.int32, torch.float32]
    assert torch.equal(got[0].cpu(), torch.from_numpy(idx))
    assert torch.equal(_bits(got[4]), _bits(torch.from_numpy(d2)))
    assert torch.equal(_bits(got[1]), _bits(torch.from_numpy(w)))
    assert torch.equal(got[2].cpu(), torch.from_numpy(off)) and torch.equal(got[3].cpu(), torch.from_numpy(ent))
    lean = K.three_nn(_d(u, dev), _d(k, dev), want_adj=False)
    assert len(lean) == 4 and lean[2] is None and lean[3] is None and torch.equal(lean[0], got[0]) and torch.equal(_bits(lean[1]), _bits(got[1]))
    return idx, w, d2, off, ent


# ---- the search ---------------------------------------------------------------------------------------------------------------------------------
SEARCH_CASES = [(1, 1), (5, 2), (7, 3), (300, 4), (257, 64), (1000, 256), (1000, 257), (5, 256), (5, 257), (1000, 512), (1000, 513), (5, 512), (5, 513),
                (70, TILE - 1), (70, TILE), (70, TILE + 1), (70, 2 * TILE + 52), (255, 20), (256, 20), (257, 20)]


@pytest.mark.parametrize("n,m", SEARCH_CASES)
def test_three_nn_any_equals_the_restatement(K, dev, n, m):
    """B = 3 different clouds on the 1/8 lattice in [-1, 1] (4,913 sites: at m >= 1,000 most sites are taken more than once, so equal
    distances and duplicated known points are everywhere).  m = 256 / 257 straddle the two adjacency builders, which must give the same lists:
    the one-launch kernel up to 256 known points, the grouping backward's three-launch builder above (m = 512 / 513: one and two full blocks of
    it, and the former limit of the Transformer head's search); at n = 5 most lists are empty"""
    rs = np.random.RandomState(1000 * n + m)
    u, k = R.lattice_pair(rs, 3, n, m)
    idx, w, d2, _, _ = _check_search(K, dev, u, k)
    if m < 3:
        assert (idx[..., m:] == 0).all() and np.isinf(d2[..., m:]).all() and (w[..., m:] == 0).all()
    if m == 1:
        assert (w[..., 0] == 1).all()


def test_three_nn_any_duplicates_and_coincident_points(K, dev):
    """known points 0 == 2 == 5 and 1 == 4: the lowest index wins every tie; unknown point 0 IS known point 3: d2 = 0 and its weight ~ 1"""
    rs = np.random.RandomState(3)
    k = SR.lattice_cloud(rs, 3, 9, -1.0, 1.0)
    k[:, 2] = k[:, 0]; k[:, 5] = k[:, 0]; k[:, 4] = k[:, 1]
    u = SR.lattice_cloud(rs, 3, 40, -1.0, 1.0)
    u[:, 0] = k[:, 3]
    u[:, 1] = k[:, 0]
    idx, w, d2, _, _ = _check_search(K, dev, u, k)
    assert (d2[:, 0, 0] == 0).all() and (w[:, 0, 0] > 0.999).all()
    assert (idx[:, 1] == np.array([0, 2, 5])).all() and (d2[:, 1] == 0).all() and np.allclose(w[:, 1], 1 / 3)
    assert not np.isin(idx[..., 0], [2, 4, 5]).any()                    # a duplicate is never the nearest: its lower twin is


def test_three_nn_any_on_a_random_float_cloud(K, dev):
    """no lattice: the index SETS equal those of a float64 ranking, leaving out the rows whose third and fourth float64 distances lie within
    a relative 1e-6; at most 1 % of the rows may be left out"""
    rs = np.random.RandomState(11)
    u = rs.uniform(-1, 1, size=(1, 2000, 3)).astype(np.float32)
    k = rs.uniform(-1, 1, size=(1, 700, 3)).astype(np.float32)
    d = ((u[:, :, None, :].astype(np.float64) - k[:, None, :, :].astype(np.float64)) ** 2).sum(-1)
    o = np.argsort(d, axis=-1, kind="stable")
    ds = np.take_along_axis(d, o[..., :4], -1)
    unsafe = (ds[..., 3] - ds[..., 2]) <= 1e-6 * ds[..., 3]
    print("[fp] random cloud: %d of %d rows excluded" % (unsafe.sum(), unsafe.size))
    assert unsafe.mean() <= 0.01
    idx = K.three_nn(_d(u, dev), _d(k, dev), want_adj=False)[0].cpu().numpy()
    assert np.array_equal(np.sort(idx, -1)[~unsafe], np.sort(o[..., :3], -1)[~unsafe])


def test_adjacency_of_a_hub_and_of_unselected_points(K, dev):
    """known point 0 is the nearest of all 5,000 unknown points (its list crosses two 2,048-entry chunks); known points 3.. are selected by
    nobody: empty lists, equal offsets"""
    rs = np.random.RandomState(12)
    n, m = 5000, 300
    k = np.zeros((1, m, 3), np.float32)
    k[0, 1] = [0.5, 0, 0]; k[0, 2] = [0, 0.5, 0]
    k[0, 3:] = 4.0 + SR.lattice_cloud(rs, 1, m - 3, 0.0, 1.0)[0]
    u = (rs.randint(-1, 2, size=(1, n, 3)) / 8.0).astype(np.float32)
    idx, w, d2, off, ent = _check_search(K, dev, u, k)
    assert (idx[0, :, 0] == 0).all() and off[0, 1] - off[0, 0] == n and np.array_equal(ent[0, :n], 3 * np.arange(n))
    assert (off[0, 3:] == 3 * n).all()


# ---- interpolation ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 4, 130])
def test_three_interpolate_with_dyadic_weights_is_exact(pu, dev, C):
    """weights (1/2, 1/4, 1/4) and integer features / cotangents: every product and partial sum is exact in float32, so forward and backward
    EQUAL int64 arithmetic whatever the order"""
    rs = np.random.RandomState(60 + C)
    B, n, m = 2, 300, 50
    feats = rs.randint(-8, 9, size=(B, C, m))
    idx = rs.randint(0, m - 5, size=(B, n, 3))                          # the last five known points are never named
    idx[:, :120] = rs.randint(0, 3, size=(B, 120, 3))                  # three hubs
    cot = rs.randint(-8, 9, size=(B, C, n))
    w = np.broadcast_to(np.array([0.5, 0.25, 0.25], np.float32), (B, n, 3)).copy()
    f = _d(feats.astype(np.float32), dev).requires_grad_(True)
    out = pu.three_interpolate(f, _d(idx.astype(np.int32), dev), _d(w, dev))
    assert out.shape == (B, C, n) and out.dtype == torch.float32
    want4 = np.stack([2 * feats[b][:, idx[b, :, 0]] + feats[b][:, idx[b, :, 1]] + feats[b][:, idx[b, :, 2]] for b in range(B)])    # 4 * out
    assert np.array_equal(out.detach().cpu().numpy().astype(np.float64) * 4, want4.astype(np.float64))
    (gf,) = torch.autograd.grad(out, f, _d(cot.astype(np.float32), dev))
    want4 = np.zeros((B, C, m), np.int64)
    for b in range(B):
        for s, c4 in enumerate((2, 1, 1)):
            np.add.at(want4[b].T, idx[b, :, s], c4 * cot[b].T)
    assert np.array_equal(gf.cpu().numpy().astype(np.float64) * 4, want4.astype(np.float64))
    assert (gf[:, :, m - 5:] == 0).all() and np.bincount(idx[0].ravel()).max() > 100


def test_three_interpolate_past_65535_row_blocks(pu, dev):
    """n = m = 262,200 rows: 65,550 blocks of four rows, more than a grid's y dimension holds (the row blocks are on grid.x), forward over the
    unknown points and backward over the known ones; dyadic weights and integer values, so both EQUAL int64 arithmetic"""
    rs = np.random.RandomState(65)
    n = m = 4 * 65535 + 60
    feats = rs.randint(-8, 9, size=(1, 1, m))
    idx = rs.randint(0, m, size=(1, n, 3))
    idx[0, -1] = [m - 1, 0, m - 2]                                       # the last row of each side is used
    cot = rs.randint(-8, 9, size=(1, 1, n))
    w = np.broadcast_to(np.array([0.5, 0.25, 0.25], np.float32), (1, n, 3)).copy()
    f = _d(feats.astype(np.float32), dev).requires_grad_(True)
    out = pu.three_interpolate(f, _d(idx.astype(np.int32), dev), _d(w, dev))
    want4 = 2 * feats[0, 0][idx[0, :, 0]] + feats[0, 0][idx[0, :, 1]] + feats[0, 0][idx[0, :, 2]]
    assert np.array_equal(out.detach().cpu().numpy()[0, 0].astype(np.float64) * 4, want4.astype(np.float64))
    (gf,) = torch.autograd.grad(out, f, _d(cot.astype(np.float32), dev))
    g4 = np.zeros(m, np.int64)
    for s_, c4 in enumerate((2, 1, 1)):
        np.add.at(g4, idx[0, :, s_], c4 * cot[0, 0])
    assert np.array_equal(gf.cpu().numpy()[0, 0].astype(np.float64) * 4, g4.astype(np.float64))


def test_interpolation_with_the_kernel_weights(K, pu, dev):
    """forward and backward bit-identical twice, and within 2e-7 (relative to the largest magnitude) of float64: three terms per output
    (one rounded product, two fused multiply-adds) and, with 150 known points for 300 unknown ones, six terms on average per gradient row"""
    rs = np.random.RandomState(70)
    B, n, m, C = 2, 300, 150, 8
    u, k = rs.uniform(-1, 1, (B, n, 3)).astype(np.float32), rs.uniform(-1, 1, (B, m, 3)).astype(np.float32)
    feats, cot = rs.standard_normal((B, C, m)).astype(np.float32), rs.standard_normal((B, C, n)).astype(np.float32)
    dist, idx = pu.three_nn(_d(u, dev), _d(k, dev))
    ri, rw, rd2 = R.three_nn(u, k)
    assert torch.equal(idx.cpu(), torch.from_numpy(ri)) and torch.allclose(dist.cpu(), torch.sqrt(torch.from_numpy(rd2)), rtol=3e-7, atol=0)
    w = K.three_nn(_d(u, dev), _d(k, dev), want_adj=False)[1]
    runs = []
    for _ in range(2):
        f = _d(feats, dev).requires_grad_(True)
        out = pu.three_interpolate(f, idx, w)
        (gf,) = torch.autograd.grad(out, f, _d(cot, dev))
        runs.append((out.detach(), gf))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))
    want = R.interp_fwd(feats.transpose(0, 2, 1), ri, rw).transpose(0, 2, 1)
    want_g = R.interp_bwd(cot.transpose(0, 2, 1), ri, rw, m).transpose(0, 2, 1)
    ef = np.abs(runs[0][0].cpu().numpy() - want).max() / np.abs(want).max()
    eb = np.abs(runs[0][1].cpu().numpy() - want_g).max() / np.abs(want_g).max()
    print("[fp] interpolation with kernel weights: forward %.3e, backward %.3e of the largest magnitude" % (ef, eb))
    assert ef <= 2e-7 and eb <= 2e-7
    # the row form that the module uses: the same numbers, through the adjacency of the search
    nn3 = K.three_nn(_d(u, dev), _d(k, dev))
    rows = _d(np.ascontiguousarray(feats.transpose(0, 2, 1)).reshape(B * m, C), dev).requires_grad_(True)
    y = K.interp_rows(rows, nn3, B, n, m)
    (gr,) = torch.autograd.grad(y, rows, _d(np.ascontiguousarray(cot.transpose(0, 2, 1)).reshape(B * n, C), dev))
    assert torch.equal(_bits(y.view(B, n, C).transpose(1, 2)), _bits(runs[0][0]))
    assert torch.equal(_bits(gr.view(B, m, C).transpose(1, 2)), _bits(runs[0][1]))


def test_single_and_double_known_points(K, pu, dev):
    """m = 1: every unknown point gets the single row exactly.  m = 2: the third slot has weight 0 and is skipped, not multiplied -- aimed at a
    row of inf (a row no point selects) the result stays finite and unchanged, forward and backward"""
    rs = np.random.RandomState(80)
    B, n, C = 2, 37, 6
    u = rs.standard_normal((B, n, 3)).astype(np.float32)
    k = rs.standard_normal((B, 3, 3)).astype(np.float32)
    feats = rs.standard_normal((B, C, 3)).astype(np.float32)
    d1, i1 = pu.three_nn(_d(u, dev), _d(k[:, :1], dev))
    w1 = K.three_nn(_d(u, dev), _d(k[:, :1], dev), want_adj=False)[1]
    assert (i1 == 0).all() and torch.isinf(d1[..., 1:]).all() and (w1[..., 0] == 1).all() and (w1[..., 1:] == 0).all()
    out = pu.three_interpolate(_d(feats[:, :, :1], dev), i1, w1)
    assert torch.equal(_bits(out), _bits(_d(feats[:, :, :1], dev).expand(B, C, n)))
    i2, w2, _, _ = K.three_nn(_d(u, dev), _d(k[:, :2], dev), want_adj=False)
    assert (w2[..., 2] == 0).all() and (i2[..., 2] == 0).all() and torch.allclose(w2.sum(-1), torch.ones(B, n, device=dev), atol=1e-6)
    base = pu.three_interpolate(_d(feats[:, :, :2], dev), i2, w2)
    poisoned = feats.copy()
    poisoned[:, :, 2] = np.inf
    aimed = i2.clone()
    aimed[..., 2] = 2
    f = _d(poisoned, dev).requires_grad_(True)
    out = pu.three_interpolate(f, aimed, w2)
    assert torch.isfinite(out).all() and torch.equal(_bits(out), _bits(base))
    (gf,) = torch.autograd.grad(out, f, torch.ones_like(out))
    assert torch.isfinite(gf).all() and (gf[:, :, 2] == 0).all()


# ---- the module ---------------------------------------------------------------------------------------------------------------------------------------
CASES = {"s16": (16, True), "s16np": (16, False), "s2": (2, True), "s1": (1, True)}


def _fp_module(tag, dev):
    from tests.golden.make_golden_fp import D1, D2, MLP
    from act_amd.models import pointnet2 as P
    return fill_module(P.PointNetFeaturePropagationAny((D1 if CASES[tag][1] else 0) + D2, MLP), f"g26.{tag}.").to(dev).train()


@pytest.mark.parametrize("tag", list(CASES))
def test_module_equals_the_reference_run(dev, g, tag):
    """train-mode output, running statistics and every gradient within the project's bar of the reference's float32 run, then eval mode with
    the updated statistics; a second train-mode pass is bit-identical"""
    model = _fp_module(tag, dev)
    t = lambda a: _d(a, dev).transpose(1, 2)
    x1, x2 = t(g[f"{tag}_xyz1"]), t(g[f"{tag}_xyz2"])
    p1 = t(g[f"{tag}_points1"]).clone().requires_grad_(True) if CASES[tag][1] else None
    p2 = t(g[f"{tag}_points2"]).clone().requires_grad_(True)
    out = model(x1, x2, p1, p2)
    assert out.shape == g[f"{tag}.out"].shape
    errs = {"out": _rel(out, g[f"{tag}.out"])}
    (out * _d(g[f"{tag}_cot"], dev)).sum().backward()
    for n, p in model.named_parameters():
        errs["grad." + n] = _rel(p.grad, g[f"{tag}.grad.{n}"])
    errs["grad_points2"] = _rel(p2.grad, g[f"{tag}.grad_points2"])
    if p1 is not None:
        errs["grad_points1"] = _rel(p1.grad, g[f"{tag}.grad_points1"])
    for n, b in model.named_buffers():
        if n.endswith("running_mean") or n.endswith("running_var"):
            errs["buf." + n] = _rel(b, g[f"{tag}.buf.{n}"])
    model.eval()
    with torch.no_grad():
        errs["out_eval"] = _rel(model(x1, x2, p1, p2), g[f"{tag}.out_eval"])
    assert set(errs) == {k[len(tag) + 1:] for k in g.files if k.startswith(tag + ".")}
    print("[fp] %s: worst %s = %.3e" % (tag, max(errs, key=errs.get), max(errs.values())))
    assert max(errs.values()) < TOL, errs
    model.train()
    with torch.no_grad():
        again = model(x1, x2, p1, p2)
    assert torch.equal(_bits(again), _bits(out))


def test_module_loads_a_reference_state_dict_strictly(dev, g):
    model = _fp_module("s16", dev)
    sd = {k: fill_tensor("other." + k, [int(x) for x in s.split(",") if x]) if not k.endswith("num_batches_tracked") else torch.tensor(3)
          for k, s in zip(g["s16_sd_keys"].tolist(), g["s16_sd_shapes"].tolist())}
    sd = {k: v.abs() + 0.5 if k.endswith("running_var") else v for k, v in sd.items()}
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(model.mlp_convs[1].weight.cpu(), sd["mlp_convs.1.weight"])


# ---- the networks -----------------------------------------------------------------------------------------------------------------------------------------
_REF = {}


def _ref_run(name):
    if name not in _REF:
        _REF[name] = R.tiny_run(name, R.TINY_SEEDS[name], torch.float64)
    return _REF[name]


def _device_net(name, dev):
    from act_amd.models import pointnet2_nets as M
    c = R.TINY[name]
    cls = {"cls": M.pointnet2_cls_ssg, "part": M.pointnet2_part_seg_msg, "sem": M.pointnet2_sem_seg}[name]
    return fill_module(cls(*c["args"], **c["sa"]), f"fp.tiny.{name}.{R.TINY_SEEDS[name]}.").to(dev)


@pytest.mark.parametrize("name", ["cls", "part", "sem"])
def test_network_equals_the_float64_restatement(dev, name):
    """B = 2, N = 128, levels of 32 / 8 centres (32 / 16 / 8 / 4 for the four-level network) and 8 samples: train-mode output with injected
    dropout masks and every parameter gradient within 1e-4 of the float64 restatement in the project's measure, |err| / max(1, |ref|)
    (tests/test_fp_host.py shows that no FPS, ball-query, three-NN or arg-max decision is near a tie at this seed).  That measure is absolute
    for small tensors -- and behind the classifier's two saturated B = 2 BatchNorm layers the backbone's gradients are 1e-7 ... 2e-5 -- so every
    gradient is also held to its own largest magnitude: 2e-2 for the classifier, 2e-4 for the segmentation networks, four times what the
    restatement's own float32 run differs from float64 (tests/fp_ref.py OWN_SCALE_BAR).  Eval mode is bit-identical twice"""
    from act_amd.utils.draws import Draws
    pts, extra, keep, cot = R.tiny_inputs(name, R.TINY_SEEDS[name])
    want, want_g, _ = _ref_run(name)
    model = _device_net(name, dev).train()
    draws = Draws(table={k: v.clone() for k, v in keep.items()}, device=dev)
    out = model(pts.to(dev), *[e.to(dev) for e in extra], draws=draws)
    assert out.shape == want.shape
    errs = {"out": _rel(out, want)}
    (out * cot.to(dev)).sum().backward()
    got_g = {n: p.grad for n, p in model.named_parameters()}
    assert set(got_g) == set(want_g) and all(v is not None for v in got_g.values())
    errs.update({"grad." + n: _rel(got_g[n], want_g[n]) for n in want_g})
    worst = sorted(errs, key=errs.get)[-3:]
    print("[fp] %s: " % name + ", ".join("%s %.3e" % (k, errs[k]) for k in worst))
    own = R.own_scale_errors(got_g, want_g)                            # every gradient against its own largest magnitude: fails on zeros
    print("[fp] %s on their own scale: " % name + ", ".join("%s %.3e" % (k, own[k]) for k in sorted(own, key=own.get)[-3:]))
    assert max(errs.values()) < TOL, {k: errs[k] for k in worst}
    assert max(own.values()) < R.OWN_SCALE_BAR[name], {k: own[k] for k in sorted(own, key=own.get)[-3:]}
    model.eval()
    with torch.no_grad():
        a = model(pts.to(dev), *[e.to(dev) for e in extra])
        b = model(pts.to(dev), *[e.to(dev) for e in extra])
    assert torch.equal(_bits(a), _bits(b)) and torch.isfinite(a).all()
    if name != "cls":
        assert torch.allclose(a.exp().sum(-1), torch.ones(a.shape[:2], device=dev), atol=1e-5)          # log-probabilities, [B, N, classes]


# ---- the runners ------------------------------------------------------------------------------------------------------------------------------------------
def test_runner_finetune_on_the_pointnet2_yaml(tmp_path):
    from tests.test_gpu_cloud_loader import _args
    from act_amd.tools import runner_finetune as RF
    from act_amd.models import pointnet2_nets as M
    from act_amd.tools import builder
    from act_amd.utils.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file("cfgs/synthetic/finetune_modelnet_pointnet2.yaml")
    assert cfg.model.NAME == "PointNet2_SSG" and cfg.model.cls_dim == 40 and not cfg.model.normal_channel
    assert isinstance(builder.model_builder(copy.deepcopy(cfg.model)), M.pointnet2_cls_ssg)
    cfg.model.update(cls_dim=4, sa1=[128, 0.2, 16], sa2=[32, 0.4, 16])
    for split in cfg.dataset.values():
        split._base_.update(NUM_SAMPLES=16, NUM_CATEGORY=4, N_POINTS=2048)
        split.others.bs = 8
    cfg.total_bs = 8
    torch.manual_seed(0)
    log = RF.run_net(_args(tmp_path), cfg, max_steps=2, log_every=1)
    assert len(log) == 2 and np.isfinite(np.array(log)).all()


def _run_main(main, argv, capsys):
    torch.manual_seed(0)
    main(argv)
    out = capsys.readouterr().out
    losses = [float(x) for x in re.findall(r"step \d+: loss ([0-9.naninf]+)", out)]
    assert len(losses) == 2 and np.all(np.isfinite(losses)), out[-2000:]
    return out


def test_runner_partseg_with_the_msg_network(tmp_path, capsys):
    from act_amd.tools import runner_partseg as RP
    out = _run_main(RP.main, ["--synthetic", "--model", "pointnet2_part_seg_msg", "--max_steps", "2", "--batch_size", "4", "--npoint", "1024",
                              "--log_every", "1", "--eval_batches", "1", "--num_workers", "0", "--log_dir", str(tmp_path)], capsys)
    assert re.search(r"best instance mIoU ([0-9.]+)", out)


def test_runner_semseg_with_the_ssg_network(tmp_path, capsys):
    from act_amd.tools import runner_semseg as RS
    out = _run_main(RS.main, ["--synthetic", "--model", "pointnet2_sem_seg", "--max_steps", "2", "--batch_size", "4", "--npoint", "1024",
                              "--log_every", "1", "--eval_batches", "1", "--num_workers", "0", "--log_dir", str(tmp_path)], capsys)
    assert re.search(r"best mIoU ([0-9.]+)", out)


def test_model_switch_keeps_the_transformer_as_the_default():
    from act_amd.tools import runner_partseg as RP, runner_semseg as RS
    from act_amd.models import partseg, semseg, pointnet2_nets as M
    assert RP.parse_args([]).model == "pt" and RS.parse_args([]).model == "pt"
    assert type(RP.build_model(RP.parse_args(["--model", "pt"]))) is partseg.get_model
    assert type(RS.build_model(RS.parse_args(["--model", "anything"]))) is semseg.get_model
    assert type(RP.build_model(RP.parse_args(["--model", "pointnet2_part_seg_msg"]))) is M.pointnet2_part_seg_msg
    sem = RS.build_model(RS.parse_args(["--model", "pointnet2_sem_seg"]))
    assert type(sem) is M.pointnet2_sem_seg and sem.in_channel == 3


# ---- errors: raised on the host before any launch, outputs untouched ------------------------------------------------------------------------------------------
def test_argument_checks(K, pu, dev):
    from act_amd import _C
    from act_amd.models import pointnet2 as P
    u, k = torch.zeros(2, 8, 3, device=dev), torch.zeros(2, 4, 3, device=dev)
    with pytest.raises(RuntimeError, match="unknown"):
        K.three_nn(u[0], k)                                             # wrong rank
    with pytest.raises(RuntimeError, match="known"):
        K.three_nn(u, k[:1])                                            # mismatched B
    with pytest.raises(RuntimeError, match="empty"):
        K.three_nn(u, k[:, :0])                                         # m = 0
    with pytest.raises(RuntimeError, match="known"):
        K.three_nn(u, k.cpu())
    with pytest.raises(RuntimeError, match="float32"):
        K.three_nn(u.double(), k)
    with pytest.raises(ValueError, match="empty"):
        pu.three_nn(u, k[:, :0])
    with pytest.raises(RuntimeError, match="contiguous"):
        pu.three_nn(u.transpose(0, 1).contiguous().transpose(0, 1), k)  # upstream's rule: no silent copy
    # the C entry points refuse bad sizes and null pointers and leave the outputs as they were
    idx = torch.full((2, 8, 3), -7, dtype=torch.int32, device=dev)
    w = torch.full((2, 8, 3), -7.0, device=dev)
    lib, ptr, st = _C.lib, _C.ptr, _C.stream()
    assert lib.act_three_nn_f32(ptr(u), ptr(k), 2, 8, 0, ptr(idx), ptr(w), None, None, None, st) != 0
    assert lib.act_three_nn_f32(ptr(u), ptr(k), 0, 8, 4, ptr(idx), ptr(w), None, None, None, st) != 0
    assert lib.act_three_nn_f32(ptr(u), None, 2, 8, 4, ptr(idx), ptr(w), None, None, None, st) != 0
    off = torch.full((2, 5), -7, dtype=torch.int32, device=dev)
    assert lib.act_three_nn_f32(ptr(u), ptr(k), 2, 8, 4, ptr(idx), ptr(w), None, ptr(off), None, st) != 0       # half an adjacency
    assert lib.act_interp_rows_fwd_f32(ptr(w), ptr(idx), ptr(w), None, None, None, 2, 8, 4, 0, ptr(w), st) != 0
    torch.cuda.synchronize()
    assert (idx == -7).all() and (w == -7).all() and (off == -7).all()
    feats = torch.zeros(2, 5, 4, device=dev)
    i3, w3 = torch.zeros(2, 8, 3, dtype=torch.int32, device=dev), torch.zeros(2, 8, 3, device=dev)
    with pytest.raises(RuntimeError, match="idx"):
        pu.three_interpolate(feats, i3.long(), w3)
    with pytest.raises(RuntimeError, match="weight"):
        pu.three_interpolate(feats, i3, w3.cpu())
    with pytest.raises(ValueError, match="weight"):
        pu.three_interpolate(feats, i3, w3[:1])
    out = pu.three_interpolate(feats + 1, torch.full_like(i3, 9), w3 + 1)           # an index outside [0, m) contributes nothing, reads nothing
    assert (out == 0).all()
    dY, wq = torch.zeros(16, 4, device=dev), torch.zeros(2, 8, 3, device=dev)      # the backward's adjacency is validated before it is touched
    off, ent = K.three_adjacency(i3, 4)
    for bad_off, bad_ent, word in ((None, ent, "adj_off"), (off.cpu(), ent, "adj_off"), (off, None, "adj_ent"), (off, ent[:, :-1], "adj_ent"),
                                   (off.float(), ent, "adj_off")):
        with pytest.raises(_C.ActHipError, match=word):
            K.interp_rows_bwd(dY, bad_off, bad_ent, wq, 2, 8, 4)
    assert lib.act_interp_rows_fwd_f32(ptr(wq), ptr(i3), ptr(wq), None, None, None, 1 << 14, 1 << 14, 4, 4, ptr(wq), st) != 0       # 2^28 rows: refused
    fp = P.PointNetFeaturePropagationAny(5 + 7, [8]).to(dev)
    x1, x2 = torch.zeros(2, 3, 8, device=dev), torch.zeros(2, 3, 4, device=dev)
    with pytest.raises(RuntimeError, match="in_channel"):
        fp(x1, x2, None, torch.zeros(2, 7, 4, device=dev))
    with pytest.raises(RuntimeError, match="points"):
        fp(x1, x2, torch.zeros(2, 5, 9, device=dev), torch.zeros(2, 7, 4, device=dev))
    with pytest.raises(RuntimeError, match="points2"):
        fp(x1, x2, torch.zeros(2, 5, 8, device=dev), None)
    with pytest.raises(RuntimeError, match="xyz"):
        fp(x1.cpu(), x2, torch.zeros(2, 5, 8, device=dev), torch.zeros(2, 7, 4, device=dev))
