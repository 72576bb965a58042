"""GPU: the PointMLP kernels (csrc/pointmlp.hip) and network (models/pointmlp.py) against tests/pointmlp_ref.py.

Grouper forward: sigma within 4 float32 ulps of float64, and GIVEN that sigma the output equal bit for bit to the float32 restatement of the
three-rounding rule.  Gradients, train-mode BatchNorm and the tiny network: within the project's 1e-4 of float64 in |err| / max(1, |ref|), and every
gradient within four times the float32 restatement's own error on its own scale (the two bars of tests/test_gpu_edge_mlp2.py)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import pointmlp_ref as P

pytestmark = pytest.mark.gpu

TOL = 1e-4
FWD_SHAPES = [(1, 2, 1, 2, 1), (2, 9, 4, 3, 8), (3, 70, 33, 24, 67), (2, 40, 5, 40, 130), (1, 300, 257, 3, 512)]
BWD_SHAPES = [(1, 2, 1, 2, 1), (2, 9, 4, 3, 8), (3, 70, 33, 24, 67), (2, 40, 5, 40, 130), (2, 300, 70, 5, 64)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def K(dev):
    import act_amd.kernels as K
    return K


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _two_bars(tag, got, want, f32, grads):
    errs = {n: P.rel(got[n], want[n]) for n in got}
    print(f"[pointmlp] {tag}: " + ", ".join("%s %.2e" % kv for kv in errs.items()))
    yards = {n: (P.own(f32[n], want[n]), P.own(got[n], want[n])) for n in grads}
    for n, (yard, mine) in yards.items():
        print("[pointmlp]   %s on its own scale: float32 restatement %.2e, kernel %.2e" % (n, yard, mine))
    assert max(errs.values()) < TOL, errs
    for n, (yard, mine) in yards.items():
        if yard == yard:                                   # nan: the exact gradient is zero, held by the absolute bar alone
            assert mine <= 4 * yard, (n, mine, yard)


def _group(K, c, dev, cat=False, want_aux=True, offset=0.0, **kw):
    feat = (c["feat"] + offset).float().to(dev)
    return K.geo_affine_group(feat, c["fps"].to(dev), c["idx"].to(dev), c["alpha"].float().to(dev), c["beta"].float().to(dev), cat=cat, want_aux=want_aux, **kw)


# ---- grouper: forward ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("B,N,S,k,D", FWD_SHAPES)
def test_grouper_forward_sigma_and_the_three_rounding_rule(K, dev, B, N, S, k, D, offset):
    c = P.grouper_case(B, N, S, k, D, hub=True)
    feat32 = (c["feat"] + offset).float()
    with torch.no_grad():
        out, sigma = _group(K, c, dev, cat=True, offset=offset)
    assert tuple(out.shape) == (B * S * k, 2 * D) and tuple(sigma.shape) == (B,)
    _, want_sigma = P.geo_affine(feat32.double(), c["fps"], c["idx"], c["alpha"], c["beta"])           # float64 on the float32 operands
    ulp = torch.from_numpy(np.spacing(want_sigma.float().numpy())).double()
    assert bool(((sigma.cpu().double() - want_sigma).abs() <= 4 * ulp).all()), (sigma.cpu(), want_sigma)
    want, _ = P.geo_affine(feat32, c["fps"], c["idx"], c["alpha"].float(), c["beta"].float(), cat=True, sigma=sigma.cpu())
    assert torch.equal(_bits(out.cpu().view(B, S, k, 2 * D)), _bits(want))                            # the anchor columns are bitwise copies too
    with torch.no_grad():
        half = _group(K, c, dev, cat=False, want_aux=False, offset=offset)
    assert torch.equal(_bits(half), _bits(out[:, :D]))


@pytest.mark.parametrize("B,N,S,k,D", FWD_SHAPES[1:])
def test_a_common_offset_changes_nothing_beyond_the_rounding_of_e(K, dev, B, N, S, k, D):
    """features on a 1/64 grid: e is exact with and without the offset of 1000, so the two runs must agree bit for bit"""
    c = P.grouper_case(B, N, S, k, D)
    c["feat"] = torch.round(c["feat"] * 64) / 64
    with torch.no_grad():
        a, sa = _group(K, c, dev)
        b, sb = _group(K, c, dev, offset=1000.0)
    assert torch.equal(_bits(sa), _bits(sb)) and torch.equal(_bits(a), _bits(b))


def test_a_cloud_without_spread_returns_beta(K, dev):
    feat = torch.tensor([[[3.5, -2.0]]], device=dev)
    z = torch.zeros(1, 1, dtype=torch.int64, device=dev)
    alpha, beta = torch.tensor([2.0, -3.0], device=dev), torch.tensor([0.25, 7.0], device=dev)
    out, sigma = K.geo_affine_group(feat, z, z.view(1, 1, 1), alpha, beta, want_aux=True)
    assert float(sigma) == 0.0 and torch.equal(out, beta.view(1, 2))
    feat.requires_grad_(True)
    K.geo_affine_group(feat, z, z.view(1, 1, 1), alpha, beta).sum().backward()
    assert torch.equal(feat.grad, torch.zeros_like(feat))                                             # torch.std's NaN is the stated difference


def test_a_batch_equals_its_clouds_run_alone(K, dev):
    B, N, S, k, D = 3, 70, 33, 24, 67
    c = P.grouper_case(B, N, S, k, D)
    with torch.no_grad():
        out, sigma = _group(K, c, dev, cat=True)
        for b in range(B):
            one = {n: (v[b:b + 1] if n in ("feat", "fps", "idx") else v) for n, v in c.items()}
            o1, s1 = _group(K, one, dev, cat=True)
            assert torch.equal(_bits(o1), _bits(out[b * S * k:(b + 1) * S * k])) and torch.equal(_bits(s1), _bits(sigma[b:b + 1]))


# ---- grouper: backward -----------------------------------------------------------------------------------------------------------------------------------
def _grouper_grads(K, c, dev, cat):
    feat = c["feat"].float().to(dev).requires_grad_(True)
    alpha, beta = c["alpha"].float().to(dev).requires_grad_(True), c["beta"].float().to(dev).requires_grad_(True)
    out = K.geo_affine_group(feat, c["fps"].to(dev), c["idx"].to(dev), alpha, beta, cat=cat)
    B, S, k, D = c["g"].shape
    cot = (torch.cat((c["g"], c["h"]), dim=-1) if cat else c["g"]).float().reshape(B * S * k, -1).to(dev)
    out.backward(cot)
    return dict(dfeat=feat.grad, dalpha=alpha.grad, dbeta=beta.grad)


@pytest.mark.parametrize("cat", [False, True])
@pytest.mark.parametrize("B,N,S,k,D", BWD_SHAPES)
def test_grouper_backward_equals_float64_autograd(K, dev, B, N, S, k, D, cat):
    c = P.grouper_case(B, N, S, k, D, seed=1, hub=True)
    c = {n: (v.float().double() if v.dtype == torch.float64 else v) for n, v in c.items()}           # the float32 operands, in float64
    want, f32 = P.grouper_run(c, torch.float64, cat), P.grouper_run(c, torch.float32, cat)
    got = _grouper_grads(K, c, dev, cat)
    grads = ("dfeat", "dalpha", "dbeta")
    _two_bars(f"grouper {(B, N, S, k, D)} cat={cat}", got, {n: want[n] for n in grads}, f32, grads)
    again = _grouper_grads(K, c, dev, cat)
    assert all(torch.equal(_bits(got[n]), _bits(again[n])) for n in grads) and float(got["dfeat"].abs().sum()) > 0


def test_grouper_refusals_leave_the_outputs_untouched(K, dev):
    from act_amd import _C
    B, N, S, k, D = 2, 9, 4, 3, 8
    c = P.grouper_case(B, N, S, k, D)
    feat, alpha, beta = c["feat"].float().to(dev), c["alpha"].float().to(dev), c["beta"].float().to(dev)
    for name, bad in (("idx", N), ("idx", -1), ("fps", N)):
        t = {n: c[n].clone() for n in ("fps", "idx")}
        t[name].view(-1)[-1] = bad
        for dtype in (torch.int64, torch.int32):
            with pytest.raises(ValueError):
                K.geo_affine_group(feat, t["fps"].to(dev, dtype), t["idx"].to(dev, dtype), alpha, beta)
    with pytest.raises(ValueError):
        K.geo_affine_group(feat, c["fps"].to(dev), c["idx"].to(dev).repeat(1, 1, 4), alpha, beta)      # k > N
    with pytest.raises(ValueError):
        K.geo_affine_group(feat[:, :, :1], c["fps"].to(dev)[:, :1], c["idx"].to(dev)[:, :1, :1], alpha[:1], beta[:1])      # S*k*D = 1
    # the C entry itself: an out-of-range index or a refused shape returns its code and writes nothing
    idx = c["idx"].to(dev, torch.int32)
    fps = c["fps"].to(dev, torch.int32)
    bad_idx = idx.clone()
    bad_idx[1, 2, 1] = N
    out = torch.full((B * S * k, D), -7.0, device=dev)
    sigma, mean = torch.full((B,), -7.0, device=dev), torch.full((B,), -7.0, device=dev)
    ws = K.workspace(dev, _C.lib.act_geo_affine_fwd_workspace(B, N, S, k, D))

    def call(ix, kk, validate=1):
        return _C.lib.act_geo_affine_group_fwd_f32(_C.ptr(feat), _C.ptr(fps), _C.ptr(ix), _C.ptr(alpha), _C.ptr(beta), 1e-5, B, N, S, kk, D, 0, validate,
                                                   _C.ptr(out), _C.ptr(sigma), _C.ptr(mean), _C.ptr(ws), ws.numel() * 4, _C.stream())
    assert call(bad_idx, k) == -4 and call(idx, N + 1) == -1 and call(idx, 0) == -1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((sigma == -7.0).all()) and bool((mean == -7.0).all())
    assert call(idx, k) == 0 and call(bad_idx, k, validate=0) == 0                                      # unchecked: clamped into the cloud
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


# ---- the residual tail -----------------------------------------------------------------------------------------------------------------------------------
def _bn(c, dev, eps=1e-5):
    bn = nn.BatchNorm1d(c["gamma"].numel(), eps=eps)
    with torch.no_grad():
        bn.weight.copy_(c["gamma"]); bn.bias.copy_(c["beta"]); bn.running_mean.copy_(c["rm"]); bn.running_var.copy_(c["rv"])
    return bn.to(dev)


@pytest.mark.parametrize("R,C", P.TAIL_EVAL_ROWS)
def test_tail_eval_mode_is_exact_on_dyadic_inputs(K, dev, R, C):
    c = P.tail_exact_case(R, C)
    want = P.tail(c["y"], c["res"], c["gamma"], c["beta"], c["rm"], c["rv"], False, eps=0.0)[0]
    bn = _bn(c, dev, eps=0.0).eval()
    with torch.no_grad():
        out = K.batch_norm_add_relu(c["y"].float().to(dev), c["res"].float().to(dev), bn, False)
    assert torch.equal(out.cpu().double(), want) and int(bn.num_batches_tracked) == 0
    assert torch.equal(bn.running_mean.cpu().double(), c["rm"])


def _tail_train(K, c, dev):
    bn = _bn(c, dev).train()
    y, res = c["y"].float().to(dev).requires_grad_(True), c["res"].float().to(dev).requires_grad_(True)
    out = K.batch_norm_add_relu(y, res, bn, True)
    out.backward(c["dout"].float().to(dev))
    return dict(out=out.detach(), running_mean=bn.running_mean, running_var=bn.running_var, dy=y.grad, dres=res.grad, dgamma=bn.weight.grad,
                dbeta=bn.bias.grad), bn


@pytest.mark.parametrize("R,C", P.TAIL_TRAIN_ROWS)
def test_tail_train_mode_equals_float64(K, dev, R, C):
    c = P.tail_train_case(R, C)
    c = {n: v.float().double() for n, v in c.items()}
    want, f32 = P.tail_run(c, torch.float64), P.tail_run(c, torch.float32)
    assert float(want["z"].abs().min()) > P.MARGIN / 2                                                 # (the float32 cast moved nothing across zero)
    got, bn = _tail_train(K, c, dev)
    assert int(bn.num_batches_tracked) == 1
    _two_bars(f"tail {(R, C)}", got, {n: want[n] for n in got}, f32, ("dy", "dres", "dgamma", "dbeta"))
    again, _ = _tail_train(K, c, dev)
    assert all(torch.equal(_bits(got[n]), _bits(again[n])) for n in got)


def test_tail_eval_mode_backward_raises_and_shapes_are_checked(K, dev):
    c = P.tail_train_case(5, 6)
    bn = _bn(c, dev).eval()
    y = c["y"].float().to(dev).requires_grad_(True)
    out = K.batch_norm_add_relu(y, c["res"].float().to(dev), bn, False)
    with pytest.raises(NotImplementedError):
        out.sum().backward()
    with pytest.raises(ValueError):
        K.batch_norm_add_relu(y, c["res"].float().to(dev)[:, :4], bn, False)


# ---- the network -----------------------------------------------------------------------------------------------------------------------------------------
def _device_net(variant, dev):
    from act_amd.models import pointmlp as M
    ref, cfg = P.tiny_net(variant)
    make = M.pointmlp if variant == "pointmlp" else M.pointmlp_elite
    net = make(P.TINY_CLS, **P.TINY)
    net.load_state_dict(ref.state_dict(), strict=True)
    return ref, net.float().to(dev)


def _project_draws(net, pts, masks, dev):
    """the anchors and neighbour lists of the project's own FPS and kNN, stage by stage, plus the injected dropout masks"""
    from act_amd.utils.draws import Draws
    d = Draws({n: m.float() for n, m in masks.items()}, record=True, device=dev)
    with torch.no_grad():
        copy.deepcopy(net).train()(pts.float().to(dev), d)
    assert all(f"fps.{i}" in d.table and f"knn.{i}" in d.table for i in range(1, 5))
    return d


@pytest.mark.parametrize("variant", ["pointmlp", "elite"])
def test_tiny_network_equals_the_float64_restatement(K, dev, variant):
    ref, net = _device_net(variant, dev)
    assert sorted(net.state_dict()) == sorted(P.layer_table(P.config(variant, **P.TINY), P.TINY_CLS))
    pts, masks, cot = P.tiny_inputs(variant)
    draws = _project_draws(net, pts, masks, dev)
    host = {n: t.cpu() for n, t in draws.table.items()}
    want, f32 = P.net_run(ref, pts, dict(host), cot, torch.float64), P.net_run(ref, pts, dict(host), cot, torch.float32)
    net.train()
    logits = net(pts.float().to(dev), draws)
    logits.backward(cot.float().to(dev))
    got = {"logits": logits.detach()}
    got.update({"grad:" + n: p.grad for n, p in net.named_parameters()})
    assert sorted(got) == sorted(want)
    _two_bars(f"tiny {variant}", got, want, f32, [n for n in got if n != "logits"])
    # eval mode twice, and the state_dict goes back into the restatement
    net.eval()
    with torch.no_grad():
        a, b = net(pts.float().to(dev)), net(pts.float().to(dev))
    assert torch.equal(_bits(a), _bits(b))
    back = copy.deepcopy(ref)
    back.load_state_dict({n: v.cpu().double() for n, v in net.state_dict().items()}, strict=True)


def test_local_grouper_forward_returns_upstreams_shapes(K, dev):
    from act_amd.models import pointmlp as M
    rs = np.random.default_rng(3)
    xyz = torch.from_numpy(rs.uniform(-1, 1, (2, 64, 3)).astype(np.float32)).to(dev)
    points = torch.from_numpy(rs.standard_normal((2, 64, 8)).astype(np.float32)).to(dev)
    for use_xyz, width in ((False, 16), (True, 19)):
        g = M.LocalGrouper(8, 16, 4, use_xyz=use_xyz, normalize="anchor").to(dev)
        new_xyz, new_points = g(xyz, points)
        assert tuple(new_xyz.shape) == (2, 16, 3) and tuple(new_points.shape) == (2, 16, 4, width)
        fps_idx, _, idx = g.choose(xyz)
        table = torch.cat((points, xyz), dim=-1) if use_xyz else points
        want, _ = P.geo_affine(table.cpu().double(), fps_idx.cpu(), idx.cpu(), g.affine_alpha.detach().cpu().double().view(-1),
                               g.affine_beta.detach().cpu().double().view(-1))
        assert P.rel(new_points[..., :width - 8], want) < 1e-5
        assert torch.equal(new_points[..., width - 8:], P.index_points(points, fps_idx).unsqueeze(2).expand(-1, -1, 4, -1))
    for normalize in ("center", None):
        with pytest.raises(ValueError):
            M.LocalGrouper(8, 16, 4, use_xyz=False, normalize=normalize)


def test_runner_finetune_on_the_pointmlp_yaml(tmp_path):
    from tests.test_gpu_cloud_loader import _args
    from act_amd.tools import runner_finetune as RF
    from act_amd.models import pointmlp as M
    from act_amd.tools import builder
    from act_amd.utils.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file("cfgs/synthetic/finetune_modelnet_pointmlp.yaml")
    assert cfg.model.NAME == "PointMLP" and cfg.model.cls_dim == 40 and cfg.model.variant == "pointmlp" and cfg.npoints == 1024
    cfg.model.update(cls_dim=4, embed_dim=8, k_neighbors=[4, 4, 4, 4])
    assert isinstance(builder.model_builder(copy.deepcopy(cfg.model)), M.Model)
    for split in cfg.dataset.values():
        split._base_.update(NUM_SAMPLES=16, NUM_CATEGORY=4, N_POINTS=2048)
        split.others.bs = 8
    cfg.total_bs = 8
    seen = []
    step = M.Model.forward_features

    def spy(self, pts, draws=None):
        seen.append((self, {n: p.detach().clone() for n, p in self.named_parameters()}) if not seen else None)
        return step(self, pts, draws)

    M.Model.forward_features = spy
    try:
        torch.manual_seed(0)
        log = RF.run_net(_args(tmp_path), cfg, max_steps=2, log_every=1)
    finally:
        M.Model.forward_features = step
    assert len(log) == 2 and np.isfinite(np.array(log)).all()
    model, before = seen[0]
    moved = [n for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert len(moved) > 20, moved                                               # the parameters move
