"""Composed mini-PointNet (csrc/composite.hip, ACT_PN_COMPOSE): on the fused schedule the 128 -> 256 conv is folded into the local half of the
512 -> 512 conv,  h3 = (a1 . (W3b W2)^T + W3b b2) + gw,  and the backward products of the pair contract over 128 channels instead of 256.  Exact in real
arithmetic, not bit-identical to the sequential form, so the composed path (the default) is held against

  * the sequential path (ACT_PN_COMPOSE=0; the switch is read once per process, so that side runs in ONE child process for all cases) at the bars of
    test_gpu_composite.py::test_encoder_fused_schedule_matches_plain,
  * the same module in float64 on the CPU: the composed forward may be at most twice as far from it as the sequential forward on the same input,
  * itself: two runs are bit-identical, and W32 = W3b W2 is rebuilt from the weights of every call (never stale).

Shapes: the smallest that reach each code path of the fused schedule (n in {32, 64}, rows % 128 == 0, C % 64 == 0)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (C, bs, g, n, listed): one 128-row tile (one partial of the tile statistics) | 64-point groups, pool-backward-on-load | C % 128 != 0: dense conv4
# backward | the bench channel count, dense dout | ... dout zero outside 4 listed groups together with need=
CASES = [(64, 1, 4, 32, False), (128, 2, 3, 64, False), (192, 3, 8, 32, False), (384, 2, 16, 32, False), (384, 2, 16, 32, True)]
ZERO_GRAD_BIASES = ("first_conv.0.bias", "first_conv.3.bias", "second_conv.0.bias")


def _inputs(case, dev):
    C, bs, g, n, listed = case
    gen = torch.Generator().manual_seed(1000 + C + 7 * n + bs)
    nb = 0.2 * torch.randn(bs, g, n, 3, generator=gen)
    dout = torch.randn(bs, g, C, generator=gen)
    need = None
    if listed:                                                  # 2 groups per cloud = 4 listed groups = one 128-row tile
        need = torch.stack([torch.randperm(g, generator=gen)[:2].sort().values for _ in range(bs)])
        keep = torch.zeros(bs, g, 1).scatter_(1, need.unsqueeze(-1), 1.0)
        dout = dout * keep
    return nb.to(dev), dout.to(dev), (need.to(dev) if need is not None else None)


def _encoder(C, dev):
    from act_amd.models.dvae import Encoder
    from tests.golden.fill import fill_module
    with torch.no_grad():
        return fill_module(Encoder(C), "cmp32.enc.").to(dev).train()


def _run(enc, nb, dout, need):
    """train forward + backward, then the eval forward -> every tensor the comparison looks at"""
    enc.train()
    enc.zero_grad(set_to_none=True)
    y = enc(nb, need=need)
    y.backward(dout)
    enc.eval()
    with torch.no_grad():
        ye = enc(nb, need=need)
    enc.train()
    torch.cuda.synchronize()
    return dict([("y", y.detach().clone()), ("y_eval", ye.clone())] + [(k, p.grad.clone()) for k, p in enc.named_parameters()] +
                [("buf." + k, b.clone().float()) for k, b in enc.named_buffers()])


def _run_case(case, dev):
    nb, dout, need = _inputs(case, dev)
    return _run(_encoder(case[0], dev), nb, dout, need)


def _ref64(case):
    """Encoder.forward (train, then eval on the updated running statistics) in float64 on the CPU, plain torch ops -> (y, y_eval); with ``need`` only the
    listed tokens are non-zero"""
    C, bs, g, n, _ = case
    F = torch.nn.functional
    nb, _, need = _inputs(case, torch.device("cpu"))
    enc = _encoder(C, torch.device("cpu")).double()
    p = {k: v.detach() for k, v in enc.named_parameters()}
    w = lambda k: p[k + ".weight"].reshape(p[k + ".weight"].shape[0], -1)
    bn1, bn2 = enc.first_conv[1], enc.second_conv[1]
    x = nb.double().reshape(bs * g * n, 3)

    def fwd(training):
        h = x @ w("first_conv.0").T + p["first_conv.0.bias"]
        h = F.relu(F.batch_norm(h, bn1.running_mean, bn1.running_var, bn1.weight, bn1.bias, training, bn1.momentum, bn1.eps))
        h2 = h @ w("first_conv.3").T + p["first_conv.3.bias"]
        fg = h2.reshape(bs * g, n, 256).max(1).values
        h3 = torch.cat([fg.repeat_interleave(n, 0), h2], 1) @ w("second_conv.0").T + p["second_conv.0.bias"]
        h3 = F.relu(F.batch_norm(h3, bn2.running_mean, bn2.running_var, bn2.weight, bn2.bias, training, bn2.momentum, bn2.eps))
        y = (h3 @ w("second_conv.3").T + p["second_conv.3.bias"]).reshape(bs * g, n, C).max(1).values.reshape(bs, g, C)
        if need is not None:
            y = y * torch.zeros(bs, g, 1, dtype=y.dtype).scatter_(1, need.unsqueeze(-1), 1.0)
        return y
    with torch.no_grad():
        return fwd(True), fwd(False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sequential(tmp_path_factory):
    """every case on the sequential path: one child process with ACT_PN_COMPOSE=0 (this file run as a script)"""
    out = str(tmp_path_factory.mktemp("pn_compose") / "sequential.pt")
    env = dict(os.environ, ACT_PN_COMPOSE="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(out, weights_only=False)


@pytest.fixture(scope="module")
def composed(dev):
    assert os.environ.get("ACT_PN_COMPOSE", "1") != "0", "this file checks the default (composed) path of the process it runs in"
    return [{k: v.cpu() for k, v in _run_case(case, dev).items()} for case in CASES]


def _saved_floats(C, bg, n):
    import ctypes
    import act_amd.composite as CP
    d = CP.PointnetDims(bg, n, C, 1e-5, 1e-5, 0.1, 0.1)
    return int(CP.lib.act_pointnet_saved_floats(ctypes.byref(d)))


def test_saved_area_drops_h2(dev, sequential):
    """h2 [R, 256] leaves the saved area, W32 [512, 128] and b32 [512] join it"""
    for C, bs, g, n, _ in CASES[:4]:
        R = bs * g * n
        assert _saved_floats(C, bs * g, n) == sequential["saved_floats"][(C, bs * g, n)] - R * 256 + 512 * 128 + 512


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_composed_matches_sequential(composed, sequential, ci):
    on, off = composed[ci], sequential["cases"][ci]
    rel = lambda a, b: ((a.double() - b.double()).abs().max() / max(1.0, b.double().abs().max().item())).item()
    l2 = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()
    assert set(on) == set(off)
    for k, a in off.items():
        r, q = rel(on[k], a), l2(on[k], a)
        print("case %d %-28s rel %.3e  l2 %.3e" % (ci, k, r, q))
        if k in ("y", "y_eval") or k.startswith("buf."):
            assert r <= 2e-5, (k, r)
        elif k in ZERO_GRAD_BIASES:                 # exactly-zero true gradient: both paths return cancellation noise
            assert r <= 2e-3, (k, r)
        else:                                       # element-wise, or L2 when a max-pool winner / ReLU sign flips between the two forms
            assert r <= 2e-5 or q <= 5e-3, (k, r, q)


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_composed_forward_error_against_float64(composed, sequential, ci):
    y64, ye64 = _ref64(CASES[ci])
    err = lambda a, b: ((a.double() - b).abs().max() / b.abs().max()).item()
    for k, ref in (("y", y64), ("y_eval", ye64)):
        e_on, e_off = err(composed[ci][k], ref), err(sequential["cases"][ci][k], ref)
        print("case %d %-6s forward error vs float64: composed %.3e  sequential %.3e" % (ci, k, e_on, e_off))
        assert e_on <= 2.0 * e_off, (k, e_on, e_off)


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_composed_is_run_to_run_identical(dev, composed, ci):
    again = _run_case(CASES[ci], dev)
    for k, a in composed[ci].items():
        assert torch.equal(again[k].cpu(), a), k


def test_w32_is_never_stale(dev):
    """forward + backward, change the two composed weights in place, run again: the bits of a fresh module that holds the changed weights"""
    case = CASES[1]
    nb, dout, need = _inputs(case, dev)
    enc = _encoder(case[0], dev)
    _run(enc, nb, dout, need)
    gen = torch.Generator().manual_seed(5)
    d2 = (0.05 * torch.randn(256, 128, 1, generator=gen)).to(dev)
    d3 = (0.05 * torch.randn(512, 512, 1, generator=gen)).to(dev)

    def change(m):
        with torch.no_grad():
            m.first_conv[3].weight.add_(d2)
            m.second_conv[0].weight.mul_(0.5).add_(d3)
    change(enc)
    fresh = _encoder(case[0], dev)
    with torch.no_grad():                                       # (the first run moved the running statistics: the fresh module starts from the same)
        for b, f in zip(enc.buffers(), fresh.buffers()):
            f.copy_(b)
    change(fresh)
    a, b = _run(enc, nb, dout, need), _run(fresh, nb, dout, need)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("n,G", [(32, 5), (64, 3), (8, 9)])
def test_pool_backward_row_walk_at_128_columns(dev, n, G):
    """act_group_max_bwd_matmul_f32 at N = 128 (the term S . W2 of the composed backward: eight parts of 32 threads per workgroup) against the dense
    product in float64 -- strided operands, padding untouched, a group with every channel on one row, a second run bit-identical; n % 8 != 0 refused"""
    import act_amd.kernels as K
    C, N = 256, 128
    gen = torch.Generator().manual_seed(n + G)
    R = G * n
    dout = torch.randn(G, C, generator=gen).to(dev)
    arg = torch.randint(0, n, (G, C), generator=gen, dtype=torch.int32)
    arg[0] = n - 1
    arg[1, : C // 2] = 0
    arg = arg.to(dev)
    dense = torch.zeros(G, n, C, device=dev).scatter_(1, arg.long().unsqueeze(1), dout.unsqueeze(1)).reshape(R, C)
    wide = (0.1 * torch.randn(C, N + 64, generator=gen)).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    for W, ldw in ((wide[:, :N].contiguous(), N), (wide, N + 64)):
        out = torch.full((R, N + 4), 7.0, device=dev)
        assert K.lib.act_group_max_bwd_matmul_f32(dout.data_ptr(), arg.data_ptr(), G, n, C, W.data_ptr(), ldw, N, out.data_ptr(), N + 4, st) == 0
        ref = dense.double() @ W[:, :N].double()
        assert ((out[:, :N].double() - ref).abs().max() / max(1.0, ref.abs().max().item())).item() <= 2e-6     # (the bar of the 256 .. 1024-column forms)
        assert (out[:, N:] == 7.0).all()
        again = torch.empty(R, N + 4, device=dev)
        assert K.lib.act_group_max_bwd_matmul_f32(dout.data_ptr(), arg.data_ptr(), G, n, C, W.data_ptr(), ldw, N, again.data_ptr(), N + 4, st) == 0
        assert torch.equal(again[:, :N], out[:, :N])
    out = torch.empty(G * 4, N, device=dev)
    assert K.lib.act_group_max_bwd_matmul_f32(dout.data_ptr(), arg.data_ptr(), G, 4, C, wide.data_ptr(), N + 64, N, out.data_ptr(), N, st) != 0


if __name__ == "__main__":                                      # the child of the ``sequential`` fixture
    sys.path.insert(0, ROOT)
    assert os.environ.get("ACT_PN_COMPOSE") == "0"
    device = torch.device("cuda:0")
    torch.save({"cases": [{k: v.cpu() for k, v in _run_case(case, device).items()} for case in CASES],
                "saved_floats": {(C, bs * g, n): _saved_floats(C, bs * g, n) for C, bs, g, n, _ in CASES}}, sys.argv[1])
