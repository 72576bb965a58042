"""Host: the restatement of the feature-propagation kernels and modules (tests/fp_ref.py) against the reference's recorded run
(tests/golden/g26_fp.npz) and against torch float64 autograd, the CPU-side argument checks of the upstream-form ops, the state-dict names of the
three PointNet++ networks, and the seeds of the GPU network tests.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import fp_ref as R
from tests.conftest import golden
from tests.golden.fill import fill_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
SYMBOLS = ("act_three_nn_f32", "act_three_adj_i32", "act_interp_rows_fwd_f32", "act_interp_rows_bwd_f32")
CASES = {"s16": (16, True), "s16np": (16, False), "s2": (2, True), "s1": (1, True)}


@pytest.fixture(scope="module")
def g():
    return golden("g26_fp")


def _rel(a, ref):
    a, ref = torch.as_tensor(a).detach().double(), torch.as_tensor(ref).detach().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return ((a - ref).abs().max() / max(1.0, ref.abs().max())).item()


# ---- the search ---------------------------------------------------------------------------------------------------------------------------------
def test_three_nn_ref_rules():
    """stable (distance, index) order, ties to the lower index, d2 = 0 for a point that is a known point, the m < 3 forms"""
    known = np.array([[[1, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0]]], np.float32)        # 0 == 2 and 1 == 4 are duplicates
    unknown = np.array([[[0, 0, 0], [1, 0, 0], [0.5, 0.5, 0]]], np.float32)
    idx, w, d2 = R.three_nn(unknown, known)
    assert idx[0].tolist() == [[1, 4, 0], [0, 2, 1], [0, 1, 2]]
    assert d2[0, 0].tolist() == [0.0, 0.0, 1.0] and d2[0, 1].tolist() == [0.0, 0.0, 1.0] and d2[0, 2].tolist() == [0.5, 0.5, 0.5]
    assert w.dtype == np.float32 and np.allclose(w[0, 2], 1 / 3) and abs(w[0, 0].sum() - 1) < 1e-6 and w[0, 0, 2] < 1e-7
    idx, w, d2 = R.three_nn(unknown, known[:, :2])                      # m == 2
    assert idx[0].tolist() == [[1, 0, 0], [0, 1, 0], [0, 1, 0]] and np.isinf(d2[..., 2]).all() and (w[..., 2] == 0).all()
    assert np.allclose(w[0, 2, :2], 0.5) and w[0, 0, 0] > 0.99999
    idx, w, d2 = R.three_nn(unknown, known[:, :1])                      # m == 1
    assert (idx == 0).all() and (w[..., 0] == 1).all() and (w[..., 1:] == 0).all() and np.isinf(d2[..., 1:]).all()


@pytest.mark.parametrize("tag", list(CASES))
def test_three_nn_ref_agrees_with_seg_ref_and_the_fixture_has_no_third_fourth_tie(g, tag):
    from tests import seg_ref as GR
    u, k = g[f"{tag}_xyz1"], g[f"{tag}_xyz2"]
    assert not R.third_fourth_tie(u, k).any()
    idx, w, d2 = R.three_nn(u, k)
    if k.shape[1] >= 3:                                                 # the two restatements are one rule where both apply
        i2, w2, off2, ent2, d3 = GR.three_nn_f32(u, k)
        assert np.array_equal(idx, i2) and np.array_equal(w.view(np.int32), w2.view(np.int32)) and np.array_equal(d2, d3)
        off, ent = R.adjacency(idx, k.shape[1])
        assert np.array_equal(off, off2) and np.array_equal(ent, ent2)
    d64 = ((u[:, :, None, :].astype(np.float64) - k[:, None, :, :].astype(np.float64)) ** 2).sum(-1)      # the lattice: float32 is exact
    kk = min(3, k.shape[1])
    assert np.array_equal(np.sort(d64, axis=-1)[:, :, :kk], d2[:, :, :kk].astype(np.float64))


@pytest.mark.parametrize("m", [1, 2, 3, 64, 128, 512])
def test_the_two_restatements_of_the_search_agree_bit_for_bit(m):
    """tests/seg_ref.py and tests/fp_ref.py restate ONE kernel family independently (the GPU files of the Transformer head and of the PointNet++
    networks each hold it to their own): idx, weights, distances, off and ent are the same on the lattice (ties) and on a float cloud (the
    weights' arithmetic order), at the sizes where two kernels used to be compared on the device and at m < 3 (idx 0 / d2 inf / weight 0)"""
    from tests import seg_ref as GR
    rs = np.random.RandomState(50 + m)
    for u, k in (R.lattice_pair(rs, 2, 700, m), (rs.uniform(-1, 1, (2, 700, 3)).astype(np.float32), rs.uniform(-1, 1, (2, m, 3)).astype(np.float32))):
        idx, w, d2 = R.three_nn(u, k)
        off, ent = R.adjacency(idx, m)
        i2, w2, off2, ent2, d3 = GR.three_nn_f32(u, k)
        assert i2.dtype == idx.dtype and w2.dtype == w.dtype == np.float32
        assert np.array_equal(idx, i2) and np.array_equal(w.view(np.int32), w2.view(np.int32)) and np.array_equal(d2.view(np.int32), d3.view(np.int32))
        assert np.array_equal(off, off2) and np.array_equal(ent, ent2)
        if m < 3:
            assert (i2[..., m:] == 0).all() and np.isinf(d3[..., m:]).all() and (w2[..., m:] == 0).all()


def test_adjacency_ref_lists_every_entry_once_in_ascending_order():
    rs = np.random.RandomState(5)
    u, k = R.lattice_pair(rs, 2, 50, 7)
    idx, _, _ = R.three_nn(u, k)
    off, ent = R.adjacency(idx, 7)
    for b in range(2):
        assert off[b, 0] == 0 and off[b, -1] == 150 and sorted(ent[b].tolist()) == list(range(150))
        for j in range(7):
            e = ent[b, off[b, j]:off[b, j + 1]]
            assert (np.diff(e) > 0).all() and (idx[b].ravel()[e] == j).all()


def test_interp_ref_equals_torch_autograd_and_skips_weight_zero():
    rs = np.random.RandomState(6)
    B, n, m, C = 2, 40, 9, 5
    u, k = rs.randn(B, n, 3).astype(np.float32), rs.randn(B, m, 3).astype(np.float32)
    idx, w, _ = R.three_nn(u, k)
    feat, dout = rs.randn(B, m, C), rs.randn(B, n, C)
    f = torch.from_numpy(feat).requires_grad_(True)
    bi = torch.arange(B)[:, None, None]
    out = (f[bi, torch.from_numpy(idx).long()] * torch.from_numpy(w).double().unsqueeze(-1)).sum(dim=2)
    (gf,) = torch.autograd.grad(out, f, torch.from_numpy(dout))
    assert np.allclose(R.interp_fwd(feat, idx, w), out.detach().numpy(), rtol=0, atol=1e-13)
    assert np.allclose(R.interp_bwd(dout, idx, w, m), gf.numpy(), rtol=0, atol=1e-13)
    idx, w, _ = R.three_nn(u, k[:, :2])                                 # m == 2: slot 2 has weight 0; aim it at a row of inf -- nothing leaks
    feat3 = feat[:, :3].copy()
    feat3[:, 2] = np.inf
    idx3 = idx.copy()
    idx3[..., 2] = 2
    out = R.interp_fwd(feat3, idx3, w)
    assert np.isfinite(out).all() and np.array_equal(out, R.interp_fwd(feat[:, :2], idx, w))
    assert np.array_equal(R.interp_bwd(dout, idx3, w, 3)[:, 2], np.zeros((B, C)))
    idx1, w1, _ = R.three_nn(u, k[:, :1])
    assert np.array_equal(R.interp_fwd(feat[:, :1], idx1, w1), np.broadcast_to(feat[:, :1], (B, n, C)))


# ---- the module -----------------------------------------------------------------------------------------------------------------------------------
def _fp_ref_run(g, tag, dtype):
    from tests.golden.make_golden_fp import D1, D2, MLP
    S, with_p1 = CASES[tag]
    model = fill_module(R.FPRef((D1 if with_p1 else 0) + D2, MLP), f"g26.{tag}.").to(dtype).train()
    t = lambda a: torch.from_numpy(a).to(dtype).transpose(1, 2)
    p1 = t(g[f"{tag}_points1"]).clone().requires_grad_(True) if with_p1 else None
    p2 = t(g[f"{tag}_points2"]).clone().requires_grad_(True)
    out = model(t(g[f"{tag}_xyz1"]), t(g[f"{tag}_xyz2"]), p1, p2)
    (out * torch.from_numpy(g[f"{tag}_cot"]).to(dtype)).sum().backward()
    rec = {"out": out.detach(), "grad_points2": p2.grad}
    if with_p1:
        rec["grad_points1"] = p1.grad
    rec.update({"grad." + n: q.grad for n, q in model.named_parameters()})
    rec.update({"buf." + n: b.clone() for n, b in model.named_buffers() if n.endswith("running_mean") or n.endswith("running_var")})
    model.eval()
    with torch.no_grad():
        rec["out_eval"] = model(t(g[f"{tag}_xyz1"]), t(g[f"{tag}_xyz2"]), None if p1 is None else p1.detach(), p2.detach())
    return rec, model


@pytest.mark.parametrize("tag", list(CASES))
def test_fp_ref_equals_the_reference_run(g, tag):
    """the restated module in float64 against the reference's float32 run: every recorded tensor within the project's bar"""
    rec, model = _fp_ref_run(g, tag, torch.float64)
    want = {k[len(tag) + 1:] for k in g.files if k.startswith(tag + ".")}
    assert set(rec) == want
    errs = {k: _rel(v, g[f"{tag}.{k}"]) for k, v in rec.items()}
    print("[fp] %s: worst %s = %.3e" % (tag, max(errs, key=errs.get), max(errs.values())))
    assert max(errs.values()) < TOL, errs
    sd = model.state_dict()
    assert list(sd.keys()) == g[f"{tag}_sd_keys"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == g[f"{tag}_sd_shapes"].tolist()


def test_device_module_has_the_reference_state_dict(g):
    from tests.golden.make_golden_fp import D1, D2, MLP
    from act_amd.models import pointnet2 as P
    from act_amd.models import semseg
    assert P.PointNetFeaturePropagation is semseg.PointNetFeaturePropagation           # the existing class is still re-exported
    sd = P.PointNetFeaturePropagationAny(D1 + D2, MLP).state_dict()
    assert list(sd.keys()) == g["s16_sd_keys"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == g["s16_sd_shapes"].tolist()
    with pytest.raises(ValueError, match="mlp"):
        P.PointNetFeaturePropagationAny(8, [6])


# ---- the upstream-form ops: argument checks that need no GPU ------------------------------------------------------------------------------------------
def test_upstream_ops_check_shapes_dtypes_and_devices():
    from act_amd import kernels as K
    from act_amd.pointnet2_ops import pointnet2_utils as pu
    u, k = torch.zeros(2, 8, 3), torch.zeros(2, 4, 3)
    with pytest.raises(ValueError, match="unknown"):
        pu.three_nn(u[0], k)
    with pytest.raises(ValueError, match="known"):
        pu.three_nn(u, torch.zeros(2, 4, 2))
    with pytest.raises(ValueError, match="clouds"):
        pu.three_nn(u, k[:1])
    with pytest.raises(RuntimeError, match="unknown"):
        pu.three_nn(u, k)                                               # CPU tensors
    with pytest.raises(RuntimeError, match="unknown"):
        K.three_nn(u, k)
    feats, idx, w = torch.zeros(2, 5, 4), torch.zeros(2, 8, 3, dtype=torch.int32), torch.zeros(2, 8, 3)
    with pytest.raises(ValueError, match="features"):
        pu.three_interpolate(feats[0], idx, w)
    with pytest.raises(ValueError, match="idx"):
        pu.three_interpolate(feats, idx[:, :, :2], w)
    with pytest.raises(ValueError, match="weight"):
        pu.three_interpolate(feats, idx, w[:1])
    with pytest.raises(ValueError, match="points"):
        pu.three_interpolate(feats, idx, w[:, :7])
    with pytest.raises(RuntimeError, match="features"):
        pu.three_interpolate(feats, idx, w)                             # CPU tensors
    with pytest.raises(RuntimeError, match="idx"):
        K.three_adjacency(idx, 4)


def test_library_exports_and_binding_declares_the_new_symbols():
    import __graft_entry__ as ge
    ge.build()
    from act_amd import _abi
    lib = ctypes.CDLL(os.path.join(ROOT, "act_amd", "lib", "libact_hip.so"))
    header = open(os.path.join(ROOT, "include", "act_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES, name
        assert name + "(" in header, name


# ---- the networks ---------------------------------------------------------------------------------------------------------------------------------------
def _sa_names(prefix, widths, conv="mlp_convs", bn="mlp_bns"):
    out = []
    for i in range(len(widths)):
        out += [f"{prefix}.{conv}.{i}.weight", f"{prefix}.{conv}.{i}.bias"]
    for i in range(len(widths)):
        out += [f"{prefix}.{bn}.{i}.{leaf}" for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    return out


def _msg_names(prefix, mlp_list):
    out = []
    for k, mlp in enumerate(mlp_list):
        for i in range(len(mlp)):
            out += [f"{prefix}.conv_blocks.{k}.{i}.weight", f"{prefix}.conv_blocks.{k}.{i}.bias"]
    for k, mlp in enumerate(mlp_list):
        for i in range(len(mlp)):
            out += [f"{prefix}.bn_blocks.{k}.{i}.{leaf}" for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    return out


def _bn(name):
    return [f"{name}.{leaf}" for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]


def _wb(name):
    return [f"{name}.weight", f"{name}.bias"]


NAMES = {
    "cls": _sa_names("sa1", [64, 64, 128]) + _sa_names("sa2", [128, 128, 256]) + _sa_names("sa3", [256, 512, 1024]) + _wb("fc1") + _bn("bn1")
    + _wb("fc2") + _bn("bn2") + _wb("fc3"),
    "part": _msg_names("sa1", [[32, 32, 64], [64, 64, 128], [64, 96, 128]]) + _msg_names("sa2", [[128, 128, 256], [128, 196, 256]])
    + _sa_names("sa3", [256, 512, 1024]) + _sa_names("fp3", [256, 256]) + _sa_names("fp2", [256, 128]) + _sa_names("fp1", [128, 128])
    + _wb("conv1") + _bn("bn1") + _wb("conv2"),
    "sem": _sa_names("sa1", [32, 32, 64]) + _sa_names("sa2", [64, 64, 128]) + _sa_names("sa3", [128, 128, 256]) + _sa_names("sa4", [256, 256, 512])
    + _sa_names("fp4", [256, 256]) + _sa_names("fp3", [256, 256]) + _sa_names("fp2", [256, 128]) + _sa_names("fp1", [128, 128, 128])
    + _wb("conv1") + _bn("bn1") + _wb("conv2"),
}
FIRST_LAST = {"cls": ((64, 3, 1, 1), (10, 256)), "part": ((32, 6, 1, 1), (50, 128, 1)), "sem": ((32, 12, 1, 1), (13, 128, 1))}


@pytest.mark.parametrize("name", ["cls", "part", "sem"])
def test_network_state_dict_names(name):
    """the restated and the device networks carry exactly the names of the issue's tables, with equal shapes"""
    from act_amd.models import pointnet2_nets as M
    c = R.TINY[name]
    ref = c["ref"](*c["args"], **c["sa"])
    dev = {"cls": M.pointnet2_cls_ssg, "part": M.pointnet2_part_seg_msg, "sem": M.pointnet2_sem_seg}[name](*c["args"], **c["sa"])
    sd_r, sd_d = ref.state_dict(), dev.state_dict()
    assert list(sd_r.keys()) == NAMES[name] and list(sd_d.keys()) == NAMES[name]
    assert [tuple(v.shape) for v in sd_r.values()] == [tuple(v.shape) for v in sd_d.values()]
    first, last = FIRST_LAST[name]
    assert tuple(next(iter(sd_d.values())).shape) == first and tuple(sd_d[NAMES[name][-2]].shape) == last
    full = {"cls": M.pointnet2_cls_ssg, "part": M.pointnet2_part_seg_msg, "sem": M.pointnet2_sem_seg}[name](*c["args"])       # published sizes
    assert list(full.state_dict().keys()) == NAMES[name]
    with pytest.raises(ValueError, match="sa9"):
        type(full)(*c["args"], sa9=(1, 1.0, 1))


def test_classifier_is_registered_and_normals_widen_the_first_conv():
    from act_amd.models import build_model_from_cfg, pointnet2_nets as M
    from act_amd.utils.config import EasyDict
    m = build_model_from_cfg(EasyDict(NAME="PointNet2_SSG", cls_dim=7, normal_channel=True, sa1=[16, 0.3, 4]))
    assert isinstance(m, M.pointnet2_cls_ssg) and m.sa1.mlp_convs[0].in_channels == 6 and m.fc3.out_features == 7 and m.sa1.npoint == 16
    assert M.pointnet2_part_seg_msg(50, normal_channel=True).fp1.mlp_convs[0].in_channels == 153
    assert M.pointnet2_sem_seg(13, in_channel=3).sa1.mlp_convs[0].in_channels == 6


@pytest.mark.parametrize("name", ["cls", "part", "sem"])
def test_network_seeds_leave_no_decision_near_a_tie(name):
    """at the seed of the GPU test the float32 and the float64 restatement agree on every FPS index, ball-query hit list, three-NN neighbour
    set and live max-pool arg-max, and every arg-max margin exceeds 1e-4: the GPU gradient checks need no allowance for flips"""
    seed = R.TINY_SEEDS[name]
    o32, g32, t32 = R.tiny_run(name, seed, torch.float32)
    o64, g64, t64 = R.tiny_run(name, seed, torch.float64)
    assert R.traces_agree(t32, t64)
    margin = min(t["margin"] for t in t64 if "margin" in t)
    errs = {k: _rel(g32[k], g64[k]) for k in g64}
    print("[fp] %s seed %d: margin %.3e, float32 vs float64 out %.3e, worst grad %s %.3e" % (name, seed, margin, _rel(o32, o64),
                                                                                             max(errs, key=errs.get), max(errs.values())))
    assert margin > 1e-4
    assert all(torch.isfinite(v).all() for v in g64.values())
    # on its own scale every gradient is a signal (above a floor, except the biases whose exact gradient is zero: those are below 1e-12), and the
    # restatement's own float32 run reproduces it to OWN_SCALE_REF -- the figure the GPU test's own-scale bar is four times of
    zero = [k for k in g64 if R.exact_zero_gradient(k)]
    assert len(zero) == {"cls": 11, "part": 25, "sem": 22}[name] and all(float(g64[k].abs().max()) < 1e-12 for k in zero)
    sizes = {k: float(v.abs().max()) for k, v in g64.items() if k not in zero}
    own = R.own_scale_errors(g32, g64)
    print("[fp] %s: smallest gradient %s %.3e, own-scale float32 vs float64 worst %s %.3e" % (name, min(sizes, key=sizes.get), min(sizes.values()),
                                                                                           max(own, key=own.get), max(own.values())))
    assert set(own) == set(sizes) and min(sizes.values()) > R.GRAD_FLOOR
    assert max(own.values()) <= R.OWN_SCALE_REF[name]
    if name == "cls":
        keep = R.tiny_inputs(name, seed)[2]
        assert all(0.2 < float(v.mean()) < 0.8 for v in keep.values())    # the conditioning leaves a real dropout pattern
    else:
        assert min(sizes.values()) > 1e-2                               # the segmentation networks' gradients are all of ordinary size
