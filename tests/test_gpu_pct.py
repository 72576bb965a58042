"""GPU: PCT's offset attention (csrc/offset_attn.hip, K.offset_attention) and network (models/pct.py) against tests/pct_ref.py.

The bars are the project's two: |err| / max(1, |ref|) < 1e-4 against float64, and every gradient within four times the float32 restatement's own
error on its own scale (the bars of tests/test_gpu_edge_mlp2.py and tests/test_gpu_pointmlp.py)."""
import copy

import numpy as np
import pytest
import torch

from tests import pct_ref as P

pytestmark = pytest.mark.gpu

TOL = 1e-4
GRADS = ("dq", "dk", "dv")


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
    print(f"[pct] {tag}: " + ", ".join("%s %.2e" % kv for kv in errs.items()))
    yards = {n: (P.own(f32[n], want[n]), P.own(got[n], want[n])) for n in grads}
    for n, (yard, mine) in yards.items():
        print("[pct]   %s on its own scale: float32 restatement %.2e, kernel %.2e" % (n, yard, mine))
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in got.values())
    assert max(errs.values()) < TOL, errs
    for n, (yard, mine) in yards.items():
        if yard == yard:                                   # nan: the exact gradient is zero, held by the absolute bar alone
            assert mine <= 4 * yard, (n, mine, yard)


def _run(K, c, dev, fused=False, tied=False):
    """the kernel on the case -> what P.op_run returns"""
    B, N = c["q"].shape[:2]
    flat = lambda t: t.float().reshape(B * N, -1).to(dev)
    q = flat(c["q"]).requires_grad_(True)
    k = q if tied else flat(c["k"]).requires_grad_(True)
    v = flat(c["v"]).requires_grad_(True)
    x = flat(c["x"]).requires_grad_(True) if fused else None
    out, lse, colsum = K.offset_attention(q, k, v, B, N, x=x, want_aux=True)
    out.backward(flat(c["dout"]))
    r = dict(out=out.detach().view(B, N, -1), lse=lse.view(B, N), colsum=colsum.view(B, N), dq=q.grad.view(B, N, -1), dv=v.grad.view(B, N, -1))
    if not tied:
        r["dk"] = k.grad.view(B, N, -1)
    if fused:
        r["dx"] = x.grad.view(B, N, -1)
    return r


_REFS = {}


def _refs(shape, family, tied):
    """float64 and float32 runs of the restatement, computed once per case"""
    key = (shape, family, tied)
    if key not in _REFS:
        c = P.op_case(*shape, family)
        _REFS[key] = (c, P.op_run(c, torch.float64, tied=tied), P.op_run(c, torch.float32, tied=tied))
    return _REFS[key]


# ---- the operator ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("B,N,Dq,C", P.OP_SHAPES)
def test_forward_and_backward_equal_float64(K, dev, B, N, Dq, C, tied):
    c, want, f32 = _refs((B, N, Dq, C), "plain", tied)
    got = _run(K, c, dev, tied=tied)
    assert sorted(got) == sorted(want)
    _two_bars(f"plain {(B, N, Dq, C)} tied={tied}", got, want, f32, [g for g in GRADS if g in got])
    if N == 1:
        assert torch.equal(got["out"].cpu().double(), c["v"])                                      # one point attends itself: x_r = v


@pytest.mark.parametrize("B,N,Dq,C", [(2, 5, 4, 8), (1, 33, 8, 12), (1, 130, 4, 4), (2, 257, 64, 256)])
def test_large_energies_need_the_row_maximum(K, dev, B, N, Dq, C):
    """rows of q = k of norm 12: E_ii = 144, exp(144) overflows float32"""
    c, want, f32 = _refs((B, N, Dq, C), "large", False)
    assert float(torch.bmm(c["q"], c["k"].transpose(1, 2)).max()) > 143
    got = _run(K, c, dev)
    _two_bars(f"large {(B, N, Dq, C)}", got, want, f32, GRADS)
    c, want, f32 = _refs((B, N, Dq, C), "large", True)
    _two_bars(f"large {(B, N, Dq, C)} tied", _run(K, c, dev, tied=True), want, f32, ("dq", "dv"))


@pytest.mark.parametrize("B,N,Dq,C", [(1, 33, 8, 12), (3, 70, 16, 36), (1, 64, 64, 256), (2, 257, 64, 256)])
def test_a_column_nobody_attends_holds_the_place_of_the_constant(K, dev, B, N, Dq, C):
    c, want, f32 = _refs((B, N, Dq, C), "unattended", False)
    assert float(want["colsum"][:, 3].max()) < 1e-11                                                # far below the 1e-9 beside it
    got = _run(K, c, dev)
    _two_bars(f"unattended {(B, N, Dq, C)}", got, want, f32, GRADS)
    mean_v = float(c["v"].abs().mean())
    assert float(got["out"][:, 3].abs().max()) < 1e-2 * mean_v                                      # about 1e-4 of an average of v, not the average


def test_a_column_whose_sum_underflows_gives_zero(K, dev):
    B, N, Dq, C = 1, 40, 8, 12
    c = P.op_case(B, N, Dq, C, "unattended")
    c["k"][:, 3] *= 10.0                                                                            # k_3 = -300 u: exp(-300 - max) is 0 in float32
    got = _run(K, c, dev)
    assert float(got["colsum"][0, 3]) == 0.0 and bool((got["out"][0, 3] == 0).all())
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    want = P.op_run(c, torch.float64)
    assert max(P.rel(got[n], want[n]) for n in got) < TOL


def test_zero_queries_give_the_exact_mean(K, dev):
    B, N, Dq, C = 2, 64, 16, 36
    rs = np.random.default_rng(5)
    v = torch.from_numpy(rs.integers(-16, 17, size=(B, N, C)) / 8.0).float()
    k = torch.from_numpy(rs.standard_normal((B * N, Dq))).float().to(dev)
    out, lse, colsum = K.offset_attention(torch.zeros(B * N, Dq, device=dev), k, v.reshape(B * N, C).to(dev), B, N, want_aux=True)
    mean = v.double().mean(dim=1, keepdim=True).expand(B, N, C)                                     # exact: a sum of 64 multiples of 1/8, over 64
    assert torch.equal(out.cpu().double().view(B, N, C), mean)
    assert bool((colsum == 1.0).all()) and P.rel(lse, torch.full((B * N,), float(np.log(64.0)))) < 1e-6


@pytest.mark.parametrize("B,N,Dq,C", [(3, 70, 16, 36), (2, 257, 64, 256)])
def test_fused_offset_is_the_subtraction_of_the_unfused_result(K, dev, B, N, Dq, C):
    c, want, f32 = _refs((B, N, Dq, C), "plain", False)
    plain, fused = _run(K, c, dev), _run(K, c, dev, fused=True)
    x = c["x"].float().to(dev)
    assert torch.equal(_bits(fused["out"]), _bits(x - plain["out"]))
    assert torch.equal(fused["dx"].cpu().double(), c["dout"])
    for n in GRADS:                                                                                 # g = -dout: every gradient changes sign, bit for bit
        assert torch.equal(_bits(fused[n]), _bits(-plain[n])), n
    assert all(torch.equal(_bits(fused[n]), _bits(plain[n])) for n in ("lse", "colsum"))
    wf = P.op_run(c, torch.float64, fused=True)
    assert max(P.rel(fused[n], wf[n]) for n in fused) < TOL
    # x alone wants a gradient: dx = dout and nothing else is computed
    flat = lambda t: t.float().reshape(B * N, -1).to(dev)
    xg = flat(c["x"]).requires_grad_(True)
    K.offset_attention(flat(c["q"]), flat(c["k"]), flat(c["v"]), B, N, x=xg).backward(flat(c["dout"]))
    assert torch.equal(xg.grad, flat(c["dout"]))


def test_two_runs_are_bit_identical_and_a_batch_equals_its_clouds(K, dev):
    B, N, Dq, C = 3, 70, 16, 36
    c, _, _ = _refs((B, N, Dq, C), "plain", False)
    a, b = _run(K, c, dev, fused=True), _run(K, c, dev, fused=True)
    assert all(torch.equal(_bits(a[n]), _bits(b[n])) for n in a)
    for i in range(B):
        one = {n: (t[i:i + 1] if torch.is_tensor(t) else t) for n, t in c.items()}
        o = _run(K, one, dev, fused=True)
        assert all(torch.equal(_bits(o[n]), _bits(a[n][i:i + 1])) for n in a), i


def test_refusals_leave_the_outputs_untouched(K, dev):
    from act_amd import _C
    B, N, Dq, C = 2, 8, 8, 8
    mk = lambda n, w: torch.randn(n, w, device=dev)
    # the wrapper
    for n, dq, cc in ((0, 8, 8), (1025, 8, 8), (8, 6, 8), (8, 68, 8), (8, 8, 260), (8, 8, 6), (8, 2, 8)):
        with pytest.raises(ValueError):
            K.offset_attention(mk(n, dq), mk(n, dq), mk(n, cc), 1, n)
    with pytest.raises(ValueError):
        K.offset_attention(mk(16, 8), mk(16, 8), mk(16, 8), 2, 9)                                    # rows != B * N
    with pytest.raises(_C.ActHipError):
        K.offset_attention(torch.zeros(16, 8), mk(16, 8), mk(16, 8), 2, 8)                           # a CPU tensor
    # the C entries: a refused shape returns its code and writes nothing
    q, k, v = mk(B * 1025, 68), mk(B * 1025, 68), mk(B * 1025, 260)
    out, xr, dv = (torch.full((B * 1025, 260), -7.0, device=dev) for _ in range(3))
    dq, dk = torch.full((B * 1025, 68), -7.0, device=dev), torch.full((B * 1025, 68), -7.0, device=dev)
    lse, colsum = torch.full((B * 1025,), -7.0, device=dev), torch.full((B * 1025,), -7.0, device=dev)
    ws = K.workspace(dev, _C.lib.act_offset_attn_workspace(B, 1024, 64, 256))

    def fwd(n, d, cc):
        return _C.lib.act_offset_attn_fwd_f32(_C.ptr(q), _C.ptr(k), _C.ptr(v), None, B, n, d, cc, _C.ptr(out), _C.ptr(lse), _C.ptr(colsum), _C.ptr(xr),
                                              _C.ptr(ws), ws.numel() * 4, _C.stream())

    def bwd(n, d, cc, dkk=None):
        return _C.lib.act_offset_attn_bwd_f32(_C.ptr(q), _C.ptr(k), _C.ptr(v), _C.ptr(colsum), _C.ptr(xr), _C.ptr(out), 0, B, n, d, cc,
                                              _C.ptr(dq), _C.ptr(dk if dkk is None else dkk), _C.ptr(dv), _C.ptr(ws), ws.numel() * 4, _C.stream())
    for n, d, cc in ((0, 8, 8), (1025, 8, 8), (8, 6, 8), (8, 68, 8), (8, 8, 260), (8, 0, 8), (8, 8, 0)):
        assert _C.lib.act_offset_attn_workspace(B, n, d, cc) == 0
        assert fwd(n, d, cc) == -1 and bwd(n, d, cc) == -1, (n, d, cc)
    assert bwd(8, 8, 8, dkk=dq) == -1                                                                # dq and dk are written separately
    with pytest.raises(_C.ActHipError):
        _C.ptr(torch.zeros(16, 8))                                                                   # a CPU tensor never reaches a C entry
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in (out, xr, dv, dq, dk, lse, colsum))
    assert fwd(8, 8, 8) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((lse[:B * 8] == -7.0).any()) and bool((lse[B * 8:] == -7.0).all())


# ---- the network -----------------------------------------------------------------------------------------------------------------------------------------
def _device_net(which, dev):
    from act_amd.models.pct import pct
    ref, cfg = P.tiny_net(which)
    net = pct(P.TINY_CLS, **cfg)
    net.load_state_dict(ref.state_dict(), strict=True)
    return ref, net.float().to(dev)


def _project_draws(net, pts, masks, dev):
    """the centres and neighbour lists of the project's own FPS and kNN, stage by stage, plus the injected dropout masks"""
    from act_amd.utils.draws import Draws
    d = Draws({n: m.float() for n, m in masks.items()}, record=True, device=dev)
    with torch.no_grad():
        copy.deepcopy(net).train()(pts.float().to(dev), d)
    assert all(f"fps.{i}" in d.table and f"knn.{i}" in d.table for i in (1, 2))
    return d


@pytest.mark.parametrize("which", ["tiny", "ragged"])
def test_tiny_network_equals_the_float64_restatement(K, dev, which):
    ref, net = _device_net(which, dev)
    assert sorted(net.state_dict()) == sorted(P.layer_table(P.TINY_CFG[which], P.TINY_CLS))
    assert all(getattr(net.pt_last, f"sa{i}").q_conv.weight is getattr(net.pt_last, f"sa{i}").k_conv.weight for i in (1, 2, 3, 4))
    pts, masks, cot = P.tiny_inputs(which)
    draws = _project_draws(net, pts, masks, dev)
    host = {n: t.cpu() for n, t in draws.table.items()}
    want, f32 = P.net_run(ref, pts, dict(host), cot, torch.float64), P.net_run(ref, pts, dict(host), cot, torch.float32)
    net.train()
    logits = net(pts.float().to(dev), draws)
    logits.backward(cot.float().to(dev))
    got = {"logits": logits.detach()}
    got.update({"grad:" + n: p.grad for n, p in net.named_parameters()})
    got.update({"stat:" + n: b.detach() for n, b in net.named_buffers() if "running" in n})
    assert sorted(got) == sorted(want)
    assert sum(n.startswith("grad:") and n.endswith("q_conv.weight") for n in got) == 4              # the tied weight's gradient, once
    _two_bars(f"net {which}", got, want, f32, [n for n in got if n.startswith("grad:")])
    assert all(int(b) == 1 for n, b in net.named_buffers() if n.endswith("num_batches_tracked"))
    # eval mode twice, and the state_dict goes back into the restatement
    net.eval()
    with torch.no_grad():
        a, b = net(pts.float().to(dev)), net(pts.float().to(dev))
    assert torch.equal(_bits(a), _bits(b)) and bool(torch.isfinite(a).all())
    back = copy.deepcopy(ref)
    back.load_state_dict({n: v.cpu().double() for n, v in net.state_dict().items()}, strict=True)


def test_runner_finetune_on_the_pct_yaml(tmp_path):
    from tests.test_gpu_cloud_loader import _args
    from act_amd.tools import runner_finetune as RF
    from act_amd.models import pct as M
    from act_amd.tools import builder
    from act_amd.utils.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file("cfgs/synthetic/finetune_modelnet_pct.yaml")
    assert cfg.model.NAME == "PCT" and cfg.model.cls_dim == 40 and cfg.npoints == 1024
    cfg.model.update(cls_dim=4, width=8, fuse=64, nsample=8)
    assert isinstance(builder.model_builder(copy.deepcopy(cfg.model)), M.Pct)
    for split in cfg.dataset.values():
        split._base_.update(NUM_SAMPLES=16, NUM_CATEGORY=4, N_POINTS=2048)
        split.others.bs = 8
    cfg.total_bs = 8
    seen = []
    step = M.Pct.forward_features

    def spy(self, pts, draws=None):
        seen.append((self, {n: p.detach().clone() for n, p in self.named_parameters()}) if not seen else None)
        return step(self, pts, draws)

    M.Pct.forward_features = spy
    try:
        torch.manual_seed(0)
        log = RF.run_net(_args(tmp_path), cfg, max_steps=2, log_every=1)
    finally:
        M.Pct.forward_features = step
    assert len(log) == 2 and np.isfinite(np.array(log)).all()
    model, before = seen[0]
    moved = [n for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert len(moved) > 20, moved                                               # the parameters move
