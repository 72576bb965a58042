"""CPU: the restatements of tests/edgeconv_ref.py against brute force and against torch's own modules, the two identities the fused EdgeConv
rests on, and the host-side surface of the DGCNN classifier (state_dict, config, C ABI table).  No GPU."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import edgeconv_ref as R


# ---- the search ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,k", [(1, 3, 1), (20, 3, 20), (65, 4, 20), (130, 40, 33)])
def test_knn_restatement_equals_the_float64_ranking_on_a_lattice(N, C, k):
    """on multiples of 1/8 every float32 distance is exact, so the float32 restatement and the float64 brute force rank identically, ties and all"""
    x = R.lattice(np.random.default_rng(N), (2, N, C), half=1.0)
    idx, d2 = R.knn(x, k)
    want, want_d, _ = R.knn_f64(x, k)
    assert idx.dtype == np.int32 and np.array_equal(idx, want) and np.array_equal(d2.astype(np.float64), want_d)
    assert (d2[:, :, 0] == 0).all()                                         # the query (or a duplicate of lower index) leads its own list
    ties = sum(len(np.unique(row)) < len(row) for row in d2.reshape(-1, k))
    assert k == 1 or ties > 0                                               # the lattice does produce ties
    for b in range(2):
        assert np.array_equal(R.sqdist_feat(x[b]), R.sqdist_feat(x[b]).T)


def test_knn_restatement_orders_nan_last_and_ties_by_index():
    x = np.zeros((1, 6, 2), np.float32)
    x[0, 2] = np.nan
    idx, d2 = R.knn(x, 6)
    assert idx[0, 0].tolist() == [0, 1, 3, 4, 5, 2] and np.isnan(d2[0, 0, 5]) and not np.isnan(d2[0, 0, :5]).any()
    assert sorted(idx[0, 2].tolist()) == [0, 1, 2, 3, 4, 5]                 # a NaN query: every distance NaN, index order


# ---- the materialised EdgeConv ---------------------------------------------------------------------------------------------------------------------------
def _edge_case(seed, B, N, k, C, out):
    rs = np.random.default_rng(seed)
    x = torch.from_numpy(rs.standard_normal((B, N, C)))
    idx = torch.from_numpy(rs.integers(0, N, size=(B, N, k)))
    W = torch.from_numpy(rs.standard_normal((out, 2 * C)) / np.sqrt(2 * C))
    gamma = torch.from_numpy(rs.standard_normal(out))
    gamma[0] = 0.0
    beta = torch.from_numpy(rs.standard_normal(out))
    return x, idx, W, gamma, beta


@pytest.mark.parametrize("training", [True, False])
def test_materialised_edgeconv_equals_torch_modules(training):
    B, N, k, C, out = 2, 9, 5, 3, 8
    x, idx, W, gamma, beta = _edge_case(0, B, N, k, C, out)
    conv, bn, act = nn.Conv2d(2 * C, out, 1, bias=False).double(), nn.BatchNorm2d(out).double(), nn.LeakyReLU(0.2)
    with torch.no_grad():
        conv.weight.copy_(W.view(out, 2 * C, 1, 1)); bn.weight.copy_(gamma); bn.bias.copy_(beta)
        bn.running_mean.copy_(torch.linspace(-1, 1, out)); bn.running_var.copy_(torch.linspace(0.5, 2, out))
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    bn.train(training)
    xj = x[R._bidx(B), idx]
    feat = torch.cat((xj - x[:, :, None, :], x[:, :, None, :].expand_as(xj)), dim=3).permute(0, 3, 1, 2)     # upstream's get_graph_feature layout
    want = act(bn(conv(feat))).max(dim=-1).values.permute(0, 2, 1)                                            # [B,N,out]
    r = R.edge_conv(x, idx, W, gamma, beta, rm, rv, training=training, momentum=bn.momentum, eps=bn.eps)
    assert float((r["out"] - want.detach()).abs().max()) < 1e-12
    assert float((r["running_mean"] - bn.running_mean).abs().max()) < 1e-12 and float((r["running_var"] - bn.running_var).abs().max()) < 1e-12
    if training:
        assert not torch.equal(bn.running_mean, rm)


def test_per_point_identity_and_monotone_selection():
    """W . cat(x_j - x_i, x_i) = W1 x_j + (W2 - W1) x_i, and max_j LeakyReLU(scale v + shift) = LeakyReLU(scale v* + shift) with v* the largest v
    where scale >= 0 and the smallest elsewhere -- with negative and zero gamma"""
    B, N, k, C, out = 2, 11, 6, 5, 12
    x, idx, W, gamma, beta = _edge_case(1, B, N, k, C, out)
    assert (gamma < 0).any() and (gamma == 0).any() and (gamma > 0).any()
    full = R.edge_conv(x, idx, W, gamma, beta)
    P, Q = x @ W[:, :C].t(), x @ (W[:, C:] - W[:, :C]).t()
    tail = R.edge_tail(P, Q, idx, gamma, beta)
    assert float((tail["v"] - full["v"]).abs().max()) < 1e-12 and float((tail["out"] - full["out"]).abs().max()) < 1e-12
    v, scale = tail["v"], tail["scale"]
    shift = beta - tail["mean"] * scale
    vstar = torch.where(scale >= 0, v.max(dim=2).values, v.min(dim=2).values)
    z = vstar * scale + shift
    assert torch.equal(torch.where(z > 0, z, 0.2 * z), tail["out"])          # exactly: the same operations on the selected element
    picked = np.take_along_axis(v.numpy(), tail["arg"][:, :, None, :].astype(np.int64), axis=2)[:, :, 0]
    assert np.array_equal(picked, vstar.numpy())
    assert np.allclose(tail["vsum"], v.sum(dim=2).numpy(), rtol=0, atol=1e-12)


def test_edge_tail_gradients_equal_the_closed_form():
    """the backward the kernel implements (dQ, dP over the inverse adjacency) against autograd of the materialised form, in float64"""
    B, N, k, C, out = 2, 7, 4, 3, 8
    x, idx, W, gamma, beta = _edge_case(2, B, N, k, C, out)
    idx[:, :, 0] = 0                                                        # point 0 named by every row; some points by none
    P = (x @ W[:, :C].t()).requires_grad_(True)
    Q = (x @ (W[:, C:] - W[:, :C]).t()).requires_grad_(True)
    g, b_ = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    r = R.edge_tail(P, Q, idx, g, b_)
    dout = torch.from_numpy(np.random.default_rng(3).standard_normal((B, N, out)))
    (r["out"] * dout).sum().backward()
    with torch.no_grad():
        M = B * N * k
        mean, rstd, scale, arg = r["mean"], r["rstd"], r["scale"], torch.from_numpy(r["arg"]).long()
        v = r["v"]
        vstar = torch.gather(v, 2, arg[:, :, None, :])[:, :, 0]
        z = vstar * scale + (b_ - mean * scale)
        dy = torch.where(z > 0, dout, 0.2 * dout)
        dbeta, dgamma = dy.sum((0, 1)), (dy * (vstar - mean) * rstd).sum((0, 1))
        m1, m2 = dbeta / M, dgamma / M
        dQ = scale * (dy - k * m1 - m2 * rstd * (torch.from_numpy(r["vsum"]) - k * mean))
        dP = torch.zeros_like(P)
        for b in range(B):
            for i in range(N):
                for j in range(k):
                    m = int(idx[b, i, j])
                    dP[b, m] += scale * ((arg[b, i] == j) * dy[b, i] - m1 - m2 * rstd * (P[b, m] + Q[b, i] - mean))
    for got, want in ((dQ, Q.grad), (dP, P.grad), (dgamma, g.grad), (dbeta, b_.grad)):
        assert float((got - want).abs().max()) < 1e-10


# ---- the network's host side -----------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_has_upstreams_keys_and_shapes():
    from act_amd.models.dgcnn_nets import dgcnn_cls
    sd = dgcnn_cls().state_dict()
    want = R.upstream_state_dict_shapes()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want and len(want) == 70
    assert sd["conv3.1.running_var"].data_ptr() == sd["bn3.running_var"].data_ptr()          # the shared modules, listed twice
    ref = R.DgcnnRef()
    assert [(k, tuple(v.shape)) for k, v in ref.state_dict().items()] == want
    res = dgcnn_cls().load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    tiny = dgcnn_cls(**R.TINY).state_dict()
    assert [(k, tuple(v.shape)) for k, v in tiny.items()] == R.upstream_state_dict_shapes(R.TINY["cls_dim"], R.TINY["emb_dims"], R.TINY["widths"])
    with pytest.raises(ValueError):
        dgcnn_cls(widths=(64, 64, 126, 256))


def test_yaml_builds_the_registered_model():
    from act_amd.models import dgcnn_nets as M
    from act_amd.tools import builder
    from act_amd.utils.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file("cfgs/synthetic/finetune_modelnet_dgcnn.yaml")
    assert cfg.model.NAME == "DGCNN_cls" and (cfg.model.cls_dim, cfg.model.k, cfg.model.emb_dims, cfg.model.dropout) == (40, 20, 1024, 0.5)
    ref = cfg_from_yaml_file("cfgs/synthetic/finetune_modelnet_pointnet2.yaml")
    for section in ("optimizer", "scheduler", "dataset", "npoints", "total_bs", "step_per_update", "max_epoch", "grad_norm_clip"):
        assert cfg[section] == ref[section], section
    model = builder.model_builder(copy.deepcopy(cfg.model))
    assert isinstance(model, M.dgcnn_cls) and isinstance(model, M.DGCNN_cls) and model.k == 20 and model.linear3.out_features == 40
    assert model.dp1.p == 0.5 and callable(model.get_loss_acc) and callable(model.load_model_from_ckpt) and callable(model.forward_features)


def test_abi_table_names_the_new_entries():
    import ctypes
    from act_amd import _abi
    names = ("act_knn_feat_f32", "act_edge_bn_workspace", "act_edge_bn_lrelu_max_fwd_f32", "act_edge_bn_lrelu_max_bwd_f32", "act_affine_lrelu_f32",
             "act_bn_lrelu_bwd_workspace", "act_bn_lrelu_bwd_f32")
    for n in names:
        assert n in _abi.SIGNATURES, n
    assert _abi.SIGNATURES["act_edge_bn_workspace"][0] is ctypes.c_size_t and len(_abi.SIGNATURES["act_knn_feat_f32"][1]) == 8
    import act_amd._C as C
    assert all(hasattr(C.lib, n) for n in names)


def test_wrappers_refuse_bad_arguments_before_any_launch():
    import act_amd.kernels as K
    with pytest.raises(RuntimeError):
        K.knn_features(torch.zeros(1, 8, 3), 4)                             # a CPU tensor
    with pytest.raises(RuntimeError):
        K.edge_conv_bn(torch.zeros(8, 8), 4, torch.zeros(1, 8, 2, dtype=torch.int32), 1, 8, 2, 4, nn.BatchNorm2d(4), True)


def test_tiny_network_seed_leaves_no_maximum_near_a_tie():
    """the seed of the device test: in float64 every EdgeConv maximum and every max-pooled channel leads its runner-up by more than LEAD, the float32
    restatement searches the same neighbour lists, and its outputs and gradients sit well inside the device test's bars"""
    draws, (out64, g64, trace, _), (out32, g32, _, _) = R.tiny_host(R.TINY_SEED)
    assert len(trace) == 5 and min(trace) > R.LEAD, trace
    for key in ("head.dp1", "head.dp2"):
        assert 0.2 < float(draws[key].mean()) < 0.8                         # the conditioning has not emptied the masks
    assert R.rel(out32, out64) < 1e-4
    assert max(R.rel(g32[n], g64[n]) for n in g64) < 1e-4
