"""CPU: the restatements of tests/pct_ref.py against plain torch autograd and the layer table -- the yardsticks the GPU tests of
tests/test_gpu_pct.py measure with -- and the host side of act_amd/models/pct.py (keys, shapes, the tied weight, the YAML)."""
import os

import pytest
import torch

from tests import pct_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))


# (the unattended family needs a column 3 and rows to ignore it)
HOST_CASES = [s + (f,) for s in P.OP_SHAPES if s[1] <= 257 for f in ("plain", "large", "unattended") if f != "unattended" or s[1] >= 5]


@pytest.mark.parametrize("B,N,Dq,C,family", HOST_CASES)
def test_hand_written_backward_equals_float64_autograd(B, N, Dq, C, family):
    c = P.op_case(B, N, Dq, C, family)
    for fused in (False, True):
        want = P.op_run(c, torch.float64, fused=fused)
        dq, dk, dv, dx = P.offset_attention_backward(c["q"], c["k"], c["v"], c["dout"], fused)
        for got, name in ((dq, "dq"), (dk, "dk"), (dv, "dv")):
            assert P.rel(got, want[name]) < 1e-12, (name, fused)
        if fused:
            assert torch.equal(dx, want["dx"])
    tied = P.op_run(c, torch.float64, tied=True)                           # one tensor for both: autograd adds the two gradients
    dq, dk, _, _ = P.offset_attention_backward(c["q"], c["q"], c["v"], c["dout"], False)
    assert P.rel(dq + dk, tied["dq"]) < 1e-12


def test_the_limit_shape_backward_equals_float64_autograd():
    B, N, Dq, C = P.OP_SHAPES[-1]
    c = P.op_case(B, N, Dq, C)
    want = P.op_run(c, torch.float64)
    dq, dk, dv, _ = P.offset_attention_backward(c["q"], c["k"], c["v"], c["dout"], False)
    assert max(P.rel(dq, want["dq"]), P.rel(dk, want["dk"]), P.rel(dv, want["dv"])) < 1e-12


def test_families_are_what_they_say():
    c = P.op_case(2, 64, 16, 8, "large")
    E = torch.bmm(c["q"], c["k"].transpose(1, 2))
    assert c["k"] is not None and torch.equal(c["q"], c["k"]) and float((torch.diagonal(E, dim1=1, dim2=2) - 144).abs().max()) < 1e-3
    assert not bool(torch.isfinite(torch.exp(E.float())).all())            # exp overflows in float32 without the row maximum
    c = P.op_case(1, 64, 16, 8, "unattended")
    out, _, colsum = P.offset_attention(c["q"], c["k"], c["v"])
    assert 1e-15 < float(colsum[0, 3]) < 1e-11
    mean_v = float(c["v"].abs().mean())
    assert float(out[0, 3].abs().max()) < 1e-2 * mean_v                    # the 1e-9 sits beside the sum: about 1e-4 of an average, not the average


@pytest.mark.parametrize("name", ["full", "tiny", "ragged"])
def test_restatement_and_network_have_the_keys_and_shapes_of_the_layer_table(name):
    from act_amd.models.pct import pct
    cfg = P.PCT if name == "full" else P.TINY_CFG[name]
    classes = 40 if name == "full" else P.TINY_CLS
    table = P.layer_table(cfg, classes)
    for net in (P.Pct(classes, **cfg), pct(classes, **cfg)):
        sd = net.state_dict()
        assert sorted(sd) == sorted(table)
        assert all(tuple(sd[n].shape) == tuple(table[n]) for n in table)
        for i in (1, 2, 3, 4):                                             # one Parameter under two keys
            assert sd[f"pt_last.sa{i}.q_conv.weight"].data_ptr() == sd[f"pt_last.sa{i}.k_conv.weight"].data_ptr()
            sa = getattr(net.pt_last, f"sa{i}")
            assert sa.q_conv.weight is sa.k_conv.weight
        if name == "full":
            assert sum(p.numel() for p in net.parameters()) == P.PCT_PARAMETERS == 2876136


def test_state_dicts_load_both_ways_strictly():
    from act_amd.models.pct import pct
    ref, cfg = P.tiny_net("tiny")
    net = pct(P.TINY_CLS, **cfg)
    net.load_state_dict(ref.state_dict(), strict=True)
    back = P.Pct(P.TINY_CLS, **cfg).double()
    back.load_state_dict({n: v.double() for n, v in net.state_dict().items()}, strict=True)
    assert all(torch.equal(a.to(b.dtype), b) for a, b in zip(ref.state_dict().values(), net.state_dict().values()))
    assert net.pt_last.sa1.q_conv.weight is net.pt_last.sa1.k_conv.weight


def test_yaml_builds_pct_through_the_registry():
    from act_amd.models import build_model_from_cfg
    from act_amd.models.pct import PCT, Pct
    from act_amd.utils.config import cfg_from_yaml_file
    here = os.getcwd()
    os.chdir(os.path.join(os.path.dirname(HERE), "act_amd"))
    try:
        cfg = cfg_from_yaml_file("cfgs/synthetic/finetune_modelnet_pct.yaml")
        mlp = cfg_from_yaml_file("cfgs/synthetic/finetune_modelnet_pointmlp.yaml")
    finally:
        os.chdir(here)
    assert cfg.model.NAME == "PCT" and cfg.model.cls_dim == 40 and cfg.npoints == 1024
    for section in ("optimizer", "scheduler", "dataset", "total_bs", "max_epoch", "grad_norm_clip", "step_per_update"):
        assert cfg[section] == mlp[section], section                      # the PointMLP recipe
    model = build_model_from_cfg(cfg.model)
    assert isinstance(model, PCT) and isinstance(model, Pct)
    assert sum(p.numel() for p in model.parameters()) == P.PCT_PARAMETERS
    assert all(hasattr(model, m) for m in ("get_loss_acc", "build_loss_func", "load_model_from_ckpt"))


def test_constructor_refuses_what_the_kernels_do_not_take():
    from act_amd.models.pct import pct
    for kw in (dict(width=6), dict(points=64, npoint=(128, 16)), dict(points=64, npoint=(32, 16), nsample=33), dict(points=4096, npoint=(2048, 1025))):
        with pytest.raises(ValueError):
            pct(4, **kw)


@pytest.mark.parametrize("which", ["tiny", "ragged"])
def test_tiny_network_float32_restatement_stays_close_to_float64(which):
    """the seeds used on the GPU keep the restatement's own float32 run within 2.5e-5 of float64 (B = 8: at B = 4, bn6 and bn7 see 4 rows and the
    gradients of the float32 run are off by up to 3e-4), so the GPU case measures the kernels and not the case"""
    model, _ = P.tiny_net(which)
    pts, masks, cot = P.tiny_inputs(which)
    draws = dict(masks)
    want = P.net_run(model, pts, draws, cot, torch.float64)
    assert all(f"fps.{i}" in draws and f"knn.{i}" in draws for i in (1, 2))
    f32 = P.net_run(model, pts, draws, cot, torch.float32)
    errs = {n: P.rel(f32[n], want[n]) for n in want}
    worst = max(errs, key=errs.get)
    assert errs[worst] < 2.5e-5, (worst, errs[worst])
    assert all(float(want[n].abs().max()) > 0 for n in want if not n.startswith("stat:"))
    yards = [P.own(f32[n], want[n]) for n in want if n.startswith("grad:") and n not in P.FEW_TERMS]
    assert min(y for y in yards if y == y) > 1.5e-6                        # no gradient's yardstick is a lucky float32 run
    assert sum(n.endswith("q_conv.weight") for n in want) == 4 and not any(n.endswith("k_conv.weight") and n.startswith("grad:") for n in want)
