"""GPU: the two-layer EdgeConv tail and the 3x3 cloud transform (csrc/edge_mlp2.hip) against tests/edge_mlp2_ref.py.

Exact: on dyadic inputs every y is exact in float32 under any order of the sum, so out and arg EQUAL the float64 restatement -- the check of the
MFMA operand layout, the zero padding and the epilogue's routing.  Train mode: outputs, both sets of running statistics and the six gradients
within the project's 1e-4 of the materialised float64 form, and every gradient within four times the float32 restatement's own error on its own
scale; the cases are those of edge_mlp2_ref.train_case, whose maxima tests/test_edge_mlp2_host.py holds clear of their runners-up."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import edge_mlp2_ref as M
from tests import edgeconv_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4


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


def _bn(g, b, rm, rv, dev, eps=1e-5):
    bn = nn.BatchNorm2d(g.numel(), eps=eps)
    with torch.no_grad():
        bn.weight.copy_(g); bn.bias.copy_(b); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    return bn.to(dev)


def _pq(c, dev):
    B, N, C1 = c["P"].shape
    return torch.cat((c["P"], c["Q"]), dim=2).float().view(B * N, 2 * C1).to(dev)


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("B,N,k,C1,C2", M.SHAPES)
def test_tail_is_exact_on_dyadic_inputs(K, dev, B, N, k, C1, C2, kind):
    c = M.exact_case(B, N, k, C1, C2, kind)
    want = M.tail(c["P"], c["Q"], c["idx"], c["g1"], c["b1"], c["w2"], c["g2"], c["b2"], c["rm1"], c["rv1"], c["rm2"], c["rv2"], False, eps=0.0,
                  slope=0.25)
    bn1, bn2 = _bn(c["g1"], c["b1"], c["rm1"], c["rv1"], dev, 0.0).eval(), _bn(c["g2"], c["b2"], c["rm2"], c["rv2"], dev, 0.0).eval()
    if kind == "search" and k <= N:
        assert np.array_equal(K.knn_features(c["P"].float().to(dev), k).cpu().numpy(), c["idx"])
    with torch.no_grad():
        out, arg = K.edge_mlp2_bn(_pq(c, dev), C1, torch.from_numpy(c["idx"]).to(dev), B, N, k, C1, bn1, c["w2"].float().to(dev), bn2, False, slope=0.25,
                                  want_aux=True)
    assert tuple(out.shape) == (B * N, C2) and arg.dtype == torch.int32
    assert torch.equal(out.cpu().view(B, N, C2).double(), want["out"])
    assert np.array_equal(arg.cpu().numpy().reshape(B, N, C2), want["arg"])
    assert torch.equal(bn1.running_mean.cpu().double(), c["rm1"]) and int(bn2.num_batches_tracked) == 0


@pytest.mark.parametrize("offset", M.OFFSETS)
@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("B,N,k,C1,C2", M.SHAPES)
def test_tail_train_mode_equals_the_materialised_float64_form(K, dev, B, N, k, C1, C2, kind, offset):
    c = M.train_case(B, N, k, C1, C2, kind, offset)
    want, _ = M.train_run(c, torch.float64)
    f32, _ = M.train_run(c, torch.float32)
    bn1, bn2 = _bn(c["g1"], c["b1"], c["rm1"], c["rv1"], dev).train(), _bn(c["g2"], c["b2"], c["rm2"], c["rv2"], dev).train()
    pq = _pq(c, dev).requires_grad_(True)
    w2 = c["w2"].float().to(dev).requires_grad_(True)
    out = K.edge_mlp2_bn(pq, C1, torch.from_numpy(c["idx"]).to(dev), B, N, k, C1, bn1, w2, bn2, True)
    out.backward(c["dout"].float().to(dev))
    got = dict(out=out, running_mean1=bn1.running_mean, running_var1=bn1.running_var, running_mean2=bn2.running_mean, running_var2=bn2.running_var,
               dpq=pq.grad, dgamma1=bn1.weight.grad, dbeta1=bn1.bias.grad, dw2=w2.grad, dgamma2=bn2.weight.grad, dbeta2=bn2.bias.grad)
    assert int(bn1.num_batches_tracked) == 1 and int(bn2.num_batches_tracked) == 1
    errs = {n: R.rel(got[n], want[n]) for n in want}
    print("[edge_mlp2] tail %s %s +%g: " % ((B, N, k, C1, C2), kind, offset) + ", ".join("%s %.2e" % kv for kv in errs.items()))
    yards = {n: (R.own(f32[n], want[n]), R.own(got[n], want[n])) for n in M.GRADS}
    for n, (yard, mine) in yards.items():
        print("[edge_mlp2]   %s on its own scale: float32 restatement %.2e, kernel %.2e" % (n, yard, mine))
    assert max(errs.values()) < TOL, errs
    for n, (yard, mine) in yards.items():
        if yard == yard:                                                  # nan: the exact gradient is zero (M = 1), held by the absolute bar alone
            assert mine <= 4 * yard, (n, mine, yard)


def test_tail_backward_is_repeatable(K, dev):
    B, N, k, C1, C2 = 2, 70, 20, 64, 64
    c = M.train_case(B, N, k, C1, C2, "made", 0.0)
    idx = torch.from_numpy(c["idx"]).to(dev)
    runs = []
    for _ in range(2):
        bn1, bn2 = _bn(c["g1"], c["b1"], c["rm1"], c["rv1"], dev).train(), _bn(c["g2"], c["b2"], c["rm2"], c["rv2"], dev).train()
        pq, w2 = _pq(c, dev).requires_grad_(True), c["w2"].float().to(dev).requires_grad_(True)
        out = K.edge_mlp2_bn(pq, C1, idx, B, N, k, C1, bn1, w2, bn2, True)
        out.backward(c["dout"].float().to(dev))
        runs.append((out, pq.grad, bn1.weight.grad, bn1.bias.grad, w2.grad, bn2.weight.grad, bn2.bias.grad, bn1.running_var, bn2.running_var))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*runs)) and runs[0][1].abs().sum() > 0 and runs[0][4].abs().sum() > 0


def test_tail_of_a_batch_equals_its_clouds_run_alone(K, dev):
    B, N, k, C1, C2 = 3, 33, 7, 36, 68
    c = M.train_case(B, N, k, C1, C2, "made", 0.0)
    bn1, bn2 = _bn(c["g1"], c["b1"], c["rm1"], c["rv1"], dev).eval(), _bn(c["g2"], c["b2"], c["rm2"], c["rv2"], dev).eval()
    idx, pq, w2 = torch.from_numpy(c["idx"]).to(dev), _pq(c, dev), c["w2"].float().to(dev)
    with torch.no_grad():
        out, arg = K.edge_mlp2_bn(pq, C1, idx, B, N, k, C1, bn1, w2, bn2, False, want_aux=True)
        for b in range(B):
            one, a1 = K.edge_mlp2_bn(pq[b * N:(b + 1) * N].contiguous(), C1, idx[b:b + 1].contiguous(), 1, N, k, C1, bn1, w2, bn2, False, want_aux=True)
            assert torch.equal(_bits(one), _bits(out[b * N:(b + 1) * N])) and torch.equal(a1, arg[b * N:(b + 1) * N])


def test_tail_refuses_what_it_does_not_take_and_leaves_its_outputs_alone(K, dev):
    B, N, k, C1, C2 = 2, 9, 4, 8, 12
    rs = np.random.default_rng(1)
    pq = torch.from_numpy(rs.standard_normal((B * N, 2 * C1))).float().to(dev)
    idx = torch.from_numpy(rs.integers(0, N, size=(B, N, k)).astype(np.int32)).to(dev)
    w2 = torch.from_numpy(rs.standard_normal((C2, C1))).float().to(dev)
    bn1, bn2 = nn.BatchNorm2d(C1).to(dev), nn.BatchNorm2d(C2).to(dev)
    for kw in (dict(k=65), dict(k=0), dict(C1=6), dict(C1=132), dict(w2=torch.zeros(6, C1, device=dev)), dict(w2=torch.zeros(132, C1, device=dev)),
               dict(slope=-0.1), dict(B=0)):
        a = dict(B=B, N=N, k=k, C1=C1, w2=w2, slope=0.2)
        a.update(kw)
        with pytest.raises(ValueError):
            K.edge_mlp2_bn(pq, C1, idx, a["B"], N, a["k"], a["C1"], bn1, a["w2"], bn2, True, slope=a["slope"])
    bad = idx.clone()
    bad[1, 3, 2] = N
    with pytest.raises(ValueError):
        K.edge_mlp2_bn(pq, C1, bad, B, N, k, C1, bn1, w2, bn2, True)
    good = K.edge_mlp2_bn(pq, C1, idx, B, N, k, C1, bn1, w2, bn2, True)
    bad[1, 3, 2] = -1                                                       # the kernel clamps: -1 reads point 0
    fixed = idx.clone()
    fixed[1, 3, 2] = 0
    assert torch.equal(K.edge_mlp2_bn(pq, C1, bad, B, N, k, C1, bn1, w2, bn2, True, validate=False), K.edge_mlp2_bn(pq, C1, fixed, B, N, k, C1, bn1, w2, bn2, True))
    with pytest.raises(NotImplementedError):
        K.edge_mlp2_bn(pq.clone().requires_grad_(True), C1, idx, B, N, k, C1, bn1.eval(), w2, bn2.eval(), False).sum().backward()
    with pytest.raises(RuntimeError):
        K.edge_mlp2_bn(pq.cpu(), C1, idx, B, N, k, C1, bn1, w2, bn2, True)
    assert int(bn1.num_batches_tracked) == 3 and torch.isfinite(good).all()
    # the C entries: every refusal returns its code before anything is launched
    R_ = B * N
    ws = torch.zeros(max(1, K.lib.act_edge_mlp2_workspace(B, N, k, C1, C2)) // 4 + 1, device=dev)
    out, ysel = torch.full((R_, C2), 7.0, device=dev), torch.full((R_, C2), 7.0, device=dev)
    arg = torch.full((R_, C2), 7, dtype=torch.int32, device=dev)
    st1, st2 = torch.full((3, C1), 7.0, device=dev), torch.full((3, C2), 7.0, device=dev)
    rm1, rv1, rm2, rv2 = (t.clone() for t in (bn1.running_mean, bn1.running_var, bn2.running_mean, bn2.running_var))
    p = K.ptr

    def fwd(k_=k, c1=C1, c2=C2, slope=0.2, wsb=None, b_=B):
        return K.lib.act_edge_mlp2_fwd_f32(p(pq), 2 * C1, C1, p(idx), b_, N, k_, c1, c2, p(bn1.weight), p(bn1.bias), p(rm1), p(rv1), p(w2), p(bn2.weight),
                                           p(bn2.bias), p(rm2), p(rv2), 1, 0.1, 1e-5, 0.1, 1e-5, slope, p(out), p(arg), p(ysel), p(st1), p(st2), p(ws),
                                           ws.numel() * 4 if wsb is None else wsb, K.stream())

    assert K.lib.act_edge_mlp2_workspace(B, N, 65, C1, C2) == 0 and K.lib.act_edge_mlp2_workspace(B, N, k, 132, C2) == 0
    for rc in (fwd(k_=65), fwd(k_=0), fwd(c1=2), fwd(c2=6), fwd(c2=132), fwd(slope=-1.0), fwd(wsb=16), fwd(b_=0)):
        assert rc == -1
    dpq = torch.full((R_, 2 * C1), 7.0, device=dev)
    d1, d2, dw = torch.full((2, C1), 7.0, device=dev), torch.full((2, C2), 7.0, device=dev), torch.full((C2, C1), 7.0, device=dev)
    dout = torch.ones(R_, C2, device=dev)

    def bwd(k_=k, qoff=C1, ldd=C2, wsb=None):
        return K.lib.act_edge_mlp2_bwd_f32(p(pq), 2 * C1, qoff, p(idx), B, N, k_, C1, C2, p(bn1.weight), p(bn1.bias), p(w2), p(bn2.weight), p(bn2.bias), p(st1),
                                           p(st2), 0.2, p(arg), p(ysel), p(dout), ldd, p(dpq), p(d1[0]), p(d1[1]), p(dw), p(d2[0]), p(d2[1]), p(ws),
                                           ws.numel() * 4 if wsb is None else wsb, K.stream())

    for rc in (bwd(k_=65), bwd(qoff=0), bwd(ldd=C2 - 1), bwd(wsb=16)):
        assert rc == -1
    torch.cuda.synchronize()
    for t in (out, ysel, st1, st2, dpq, d1, d2, dw):
        assert bool((t == 7.0).all())
    assert bool((arg == 7).all()) and not ws.any()
    assert torch.equal(rm1, bn1.running_mean) and torch.equal(rv2, bn2.running_var)


# ---- the 3x3 transform ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1025])
def test_cloud_transform3_equals_integer_arithmetic(K, dev, N):
    rs = np.random.default_rng(N)
    B = 3
    x, T, dy = rs.integers(-50, 51, size=(B, N, 3)), rs.integers(-9, 10, size=(B, 3, 3)), rs.integers(-50, 51, size=(B, N, 3))
    y, dx, dT = M.transform3(x, T, dy)                                       # int64; |dT| <= 1025 * 2500 < 2^24
    xd, Td = torch.from_numpy(x).float().to(dev).requires_grad_(True), torch.from_numpy(T).float().to(dev).requires_grad_(True)
    yd = K.cloud_transform3(xd, Td)
    yd.backward(torch.from_numpy(dy).float().to(dev))
    assert np.array_equal(yd.detach().cpu().numpy().astype(np.int64), y) and np.array_equal(xd.grad.cpu().numpy().astype(np.int64), dx)
    assert np.array_equal(Td.grad.cpu().numpy().astype(np.int64), dT)


def test_cloud_transform3_on_gaussian_inputs_and_twice(K, dev):
    rs = np.random.default_rng(0)
    B, N = 4, 1025
    x, T, dy = rs.standard_normal((B, N, 3)), rs.standard_normal((B, 3, 3)), rs.standard_normal((B, N, 3))
    x, T, dy = (t.astype(np.float32).astype(np.float64) for t in (x, T, dy))
    want = M.transform3(x, T, dy)
    runs = []
    for _ in range(2):
        xd, Td = torch.from_numpy(x).float().to(dev).requires_grad_(True), torch.from_numpy(T).float().to(dev).requires_grad_(True)
        yd = K.cloud_transform3(xd, Td)
        yd.backward(torch.from_numpy(dy).float().to(dev))
        runs.append((yd, xd.grad, Td.grad))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*runs))
    # 2e-7 of float64 on the scale of the terms that are summed: three products for y and dx, N for dT
    scale = (np.einsum("bni,bij->bnj", np.abs(x), np.abs(T)), np.einsum("bnj,bij->bni", np.abs(dy), np.abs(T)), np.einsum("bni,bnj->bij", np.abs(x), np.abs(dy)))
    for got, ref, sc in zip(runs[0], want, scale):
        err = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref) / sc
        print("[edge_mlp2] transform3: %.2e" % err.max())
        assert err.max() <= 2e-7
    with pytest.raises(ValueError):
        K.cloud_transform3(torch.zeros(2, 5, 3, device=dev), torch.zeros(3, 3, 3, device=dev))
    with pytest.raises(RuntimeError):
        K.cloud_transform3(torch.zeros(2, 5, 3), torch.zeros(2, 3, 3, device=dev))


# ---- the networks -----------------------------------------------------------------------------------------------------------------------------------------
def _device_net(name, dev):
    from act_amd.models import dgcnn_nets as D
    model = D.dgcnn_partseg(**M.TINY_PART) if name == "part" else D.dgcnn_semseg(**M.TINY_SEM)
    model.load_state_dict(M.net_ref(name, torch.float32).state_dict(), strict=True)
    return model.to(dev)


@pytest.mark.parametrize("name", ["part", "sem"])
def test_network_equals_the_float64_modules(K, dev, name):
    """B = 2, N = 64, k = 8, train mode.  The device searches and records its neighbour lists; they and the dropout masks are replayed into torch's
    own modules at float64 and float32.  In float64 every selected maximum leads its runner-up by more than LEAD."""
    from act_amd.utils.draws import Draws
    pts, onehot, keep, cot = M.net_inputs(name)
    args = (pts.to(dev), onehot.to(dev)) if name == "part" else (pts.to(dev),)
    keys = (("knn.t",) if name == "part" else ()) + ("knn.1", "knn.2", "knn.3")
    model = _device_net(name, dev).train()
    rec = Draws(table={k: v.clone() for k, v in keep.items()}, record=True, device=dev)
    with torch.no_grad():
        copy.deepcopy(model)(*args, draws=rec)
    lists = {k: rec.table[k].cpu() for k in keys}
    assert all(v.dtype == torch.int32 and tuple(v.shape) == (M.NET_B, M.NET_N, 8) for v in lists.values())
    draws = {**keep, **lists}
    want, want_g, trace = M.net_run(name, torch.float64, draws)
    f32, f32_g, _ = M.net_run(name, torch.float32, draws)
    assert min(trace) > M.LEAD, trace
    logp = model(*args, draws=Draws(table={k: v.clone() for k, v in draws.items()}, device=dev))
    assert tuple(logp.shape) == tuple(want.shape)
    (logp * cot.to(dev)).sum().backward()
    got_g = {n: p.grad for n, p in model.named_parameters()}
    assert set(got_g) == set(want_g) and all(v is not None for v in got_g.values())
    errs = {"logp": R.rel(logp, want)}
    errs.update({"grad." + n: R.rel(got_g[n], want_g[n]) for n in want_g})
    worst = sorted(errs, key=errs.get)[-3:]
    print("[edge_mlp2] network %s: " % name + ", ".join("%s %.3e" % (k, errs[k]) for k in worst))
    yards = {n: (R.own(f32_g[n], want_g[n]), R.own(got_g[n], want_g[n])) for n in want_g}
    over = {n: v for n, v in yards.items() if v[0] == v[0] and v[1] > 4 * v[0]}
    print("[edge_mlp2] network %s, own scale (float32 modules, device): " % name + ", ".join("%s %.2e %.2e" % (n, a, b) for n, (a, b) in yards.items()))
    assert max(errs.values()) < TOL, {k: errs[k] for k in worst}
    assert not over, over
    model.eval()
    with torch.no_grad():
        a, b = model(*args), model(*args)
    assert torch.equal(_bits(a), _bits(b)) and torch.isfinite(a).all()


def _run_main(main, argv, capsys):
    import re
    torch.manual_seed(0)
    main(argv)
    out = capsys.readouterr().out
    losses = [float(x) for x in re.findall(r"step \d+: loss ([0-9.naninf]+)", out)]
    assert len(losses) == 2 and np.all(np.isfinite(losses)), out[-2000:]
    return out


def test_runner_partseg_with_the_dgcnn_network(tmp_path, capsys):
    import re
    from act_amd.tools import runner_partseg as RP
    out = _run_main(RP.main, ["--synthetic", "--model", "dgcnn_partseg", "--max_steps", "2", "--batch_size", "4", "--npoint", "512", "--log_every", "1",
                              "--eval_batches", "1", "--num_workers", "0", "--log_dir", str(tmp_path)], capsys)
    assert re.search(r"best instance mIoU ([0-9.]+)", out)


def test_runner_semseg_with_the_dgcnn_network(tmp_path, capsys):
    import re
    from act_amd.tools import runner_semseg as RS
    out = _run_main(RS.main, ["--synthetic", "--model", "dgcnn_semseg", "--max_steps", "2", "--batch_size", "4", "--npoint", "512", "--log_every", "1",
                              "--eval_batches", "1", "--num_workers", "0", "--log_dir", str(tmp_path)], capsys)
    assert re.search(r"best mIoU ([0-9.]+)", out)
