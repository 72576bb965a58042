"""GPU: the language teacher's four kernels (csrc/bert.hip) where tests/test_gpu_bert.py does not reach: sequence lengths around a 32-row tile and a
128-row workgroup, odd B*H, every LayerNorm dispatch width, large logits, an ill-conditioned recovered xhat, the bad-argument returns, and the
Philox keep masks -- recovered at any S / head_dim, compared with the kernels' stream restated on the host (tests/philox_ref.py), and required to
be the ones the forward, the dQ kernel and the dK/dV kernel all use.  Everything is synthetic with fixed seeds; the references are float64 torch on the CPU."""
import pytest
import torch

from tests import bert_ref as BR
from tests.philox_ref import host_ln_mask as _host_ln_mask, host_attn_mask as _host_attn_mask
from tests.test_gpu_bert import TOL, _rel, _gen, _ln_ref, _attn_ref, _layer_weights

pytestmark = pytest.mark.gpu
assert TOL == 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def K():
    import act_amd.kernels as K
    return K


def _residue_rates_ok(m, p, axis_len):
    """keep rate of each residue (index % 4) along the last axis, separately: all four words of a Philox call are used"""
    m = m.double()
    for r in range(min(4, axis_len)):
        part = m[..., r::4]
        n = part.numel()
        rate = part.mean().item()
        assert abs(rate - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5, (r, rate, n)


# ---------------------------------------------------------------------------------------------- 1. attention with dropout, injected mask
def _lse_ref(qkv):
    B, S, _, H, hd = qkv.shape
    q, k = qkv[:, :, 0].transpose(1, 2).double(), qkv[:, :, 1].transpose(1, 2).double()
    return torch.logsumexp(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1)               # [B,H,S], over the UNDROPPED probabilities


def _attn_errs(K, dev, qkv, mask, p, dout, out_ref, dqkv_ref, seed=0):
    B, S, _, H, hd = qkv.shape
    qd, dd = qkv.to(dev), dout.to(dev)
    md = mask.to(dev) if mask is not None else None
    out, lse = K.attention_dropout_fwd(qd, B, S, H, hd, p, seed, md)
    dqkv = K.attention_dropout_bwd(qd, out, dd, lse, B, S, H, hd, p, seed, md)
    assert torch.isfinite(out).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all()
    errs = dict(out=_rel(out, out_ref), lse=_rel(lse, _lse_ref(qkv)), dq=_rel(dqkv[:, :, 0], dqkv_ref[:, :, 0]),
                dk=_rel(dqkv[:, :, 1], dqkv_ref[:, :, 1]), dv=_rel(dqkv[:, :, 2], dqkv_ref[:, :, 2]))
    return out, lse, dqkv, errs


# S: 1, and one short of / at / one past a 32-row tile, two tiles, a 128-row workgroup; 65 and 127 leave a partial workgroup with three and four
# live waves, 129 and 160 a second workgroup.  (B, H): B*H odd, H = 1 and H = 3 (the bh -> (b, h) split and the head stride), both head dims.
ATTN_EDGES = [
    (1, 1, 1, 32, 0.1), (2, 1, 3, 64, 0.5), (3, 31, 1, 64, 0.5), (1, 31, 3, 32, 0.1), (1, 32, 3, 32, 0.5), (3, 32, 1, 64, 0.1),
    (2, 33, 3, 64, 0.5), (1, 33, 1, 32, 0.1), (1, 63, 1, 64, 0.1), (3, 64, 1, 32, 0.5), (1, 64, 3, 64, 0.1), (1, 65, 3, 64, 0.5),
    (3, 65, 1, 32, 0.1), (2, 127, 3, 32, 0.5), (1, 127, 1, 64, 0.1), (1, 129, 3, 64, 0.1), (3, 129, 1, 32, 0.5), (2, 160, 3, 32, 0.1),
    (1, 160, 1, 64, 0.5),
]


@pytest.mark.parametrize("B,S,H,hd,p", ATTN_EDGES)
def test_attention_dropout_edges_against_float64(dev, K, B, S, H, hd, p):
    g = _gen(1000 * B + 10 * S + H + hd)
    qkv = torch.randn(B, S, 3, H, hd, generator=g)
    dout = torch.randn(B * S, H * hd, generator=g)
    mask = (torch.rand(B, H, S, S, generator=g) >= p).to(torch.uint8)
    bq, hq, qz = B - 1, H - 1, S // 2                               # a query whose every key is dropped: exact zeros, not NaN
    bk, hk, kz = 0, 0, (2 * S) // 3                                 # a key no query keeps: it receives no dV
    mask[bq, hq, qz] = 0
    mask[bk, hk, :, kz] = 0
    out_ref, dqkv_ref = _attn_ref(qkv, mask, p, dout)
    out, lse, dqkv, errs = _attn_errs(K, dev, qkv, mask, p, dout, out_ref, dqkv_ref)
    print(errs)
    assert out.view(B, S, H, hd)[bq, qz, hq].abs().max().item() == 0.0
    assert dqkv[bk, kz, 2, hk].abs().max().item() == 0.0
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("B,S,H,hd", [(2, 33, 3, 64), (3, 129, 1, 32), (1, 1, 1, 64)])
def test_attention_dropout_entry_at_p0(dev, K, B, S, H, hd):
    """the layer routes p = 0 to act_attention_fwd_f32 / _bwd_f32, but the ABI takes it: float64 parity, and parity with those kernels"""
    g = _gen(77 + S)
    qkv = torch.randn(B, S, 3, H, hd, generator=g)
    dout = torch.randn(B * S, H * hd, generator=g)
    out_ref, dqkv_ref = _attn_ref(qkv, torch.ones(B, H, S, S), 0.0, dout)
    out, lse, dqkv, errs = _attn_errs(K, dev, qkv, None, 0.0, dout, out_ref, dqkv_ref, seed=5)
    qd, dd = qkv.to(dev), dout.to(dev)
    out0, lse0 = K.attention_fwd(qd, B, S, H, hd)
    dqkv0 = K.attention_bwd(qd, out0, dd, lse0, B, S, H, hd)
    errs.update(out_vs_plain=_rel(out, out0), dqkv_vs_plain=_rel(dqkv, dqkv0))
    print(errs)
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("B,S,H,hd", [(2, 64, 2, 64), (1, 100, 2, 32)])
def test_attention_dropout_large_logits(dev, K, B, S, H, hd):
    """qkv * 6: logits of a few hundred.  lse is stored in natural-log units and multiplied back by log2 e in the backward; that round trip
    and the fp32 scores themselves are the error here, estimated at a few 1e-5.
    Measured on an MI355X (maxima over the two shapes): out 4.6e-6, lse 2.2e-7, dq 8.6e-6, dk 9.0e-6, dv 4.2e-6."""
    p = 0.1
    g = _gen(600 + S)
    qkv = 6.0 * torch.randn(B, S, 3, H, hd, generator=g)
    dout = torch.randn(B * S, H * hd, generator=g)
    mask = (torch.rand(B, H, S, S, generator=g) >= p).to(torch.uint8)
    out_ref, dqkv_ref = _attn_ref(qkv, mask, p, dout)
    _, _, _, errs = _attn_errs(K, dev, qkv, mask, p, dout, out_ref, dqkv_ref)
    print(errs)
    assert max(errs.values()) <= TOL, errs


# ---------------------------------------------------------------------------------------------- 2. the Philox mask of the attention
def _recover_attn_mask(K, dev, B, S, H, hd, p, seed, ctr=None, gen_seed=21):
    """the keep bit of (row, key) does not depend on v: for each chunk of hd keys, v = that chunk's identity, and out (1-p) / P is the chunk of
    the mask the forward used.  q, k = 0.5 randn keeps every P far above fp32 noise."""
    g = _gen(gen_seed)
    qkv = torch.zeros(B, S, 3, H, hd)
    qkv[:, :, :2] = 0.5 * torch.randn(B, S, 2, H, hd, generator=g)
    q, k = qkv[:, :, 0].transpose(1, 2).double(), qkv[:, :, 1].transpose(1, 2).double()
    probs = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1)
    m = torch.zeros(B, H, S, S, dtype=torch.uint8)
    for c0 in range(0, S, hd):
        n = min(hd, S - c0)
        v = torch.zeros(S, hd)
        v[c0 + torch.arange(n), torch.arange(n)] = 1.0
        qkv[:, :, 2] = v.view(1, S, 1, hd)
        out, _ = K.attention_dropout_fwd(qkv.to(dev), B, S, H, hd, p, seed, None, ctr)
        ratio = out.view(B, S, H, hd).transpose(1, 2).double().cpu()[..., :n] * (1 - p) / probs[..., c0:c0 + n]
        assert ((ratio - ratio.round()).abs() < 1e-3).all() and ratio.round().min() >= 0 and ratio.round().max() <= 1
        m[..., c0:c0 + n] = ratio.round().to(torch.uint8)
    return m


PHILOX_SHAPES = [(2, 33, 3, 64), (1, 100, 2, 32), (1, 129, 1, 64), (2, 200, 1, 32), (3, 5, 1, 64)]


@pytest.mark.parametrize("B,S,H,hd", PHILOX_SHAPES)
def test_attention_philox_mask_is_shared_by_all_three_kernels(dev, K, B, S, H, hd):
    """forward (four keeps per call), dQ (the same) and dK/dV (one keep per call, for a fixed key column) regenerate the mask independently: with
    the forward's mask injected instead, out, lse and dqkv must not change by a bit -- at keys >= 32, in a second workgroup, on clamped tail rows"""
    p, seed = 0.1, 99
    m = _recover_attn_mask(K, dev, B, S, H, hd, p, seed)
    assert torch.equal(m, _host_attn_mask(B, S, H, p, seed))             # and it is the stream of tests/philox_ref.py
    g = _gen(31 + S)
    qkv = torch.randn(B, S, 3, H, hd, generator=g).to(dev)
    dout = torch.randn(B * S, H * hd, generator=g).to(dev)
    md = m.to(dev)
    out, lse = K.attention_dropout_fwd(qkv, B, S, H, hd, p, seed)
    out_m, lse_m = K.attention_dropout_fwd(qkv, B, S, H, hd, p, 0, md)
    assert torch.equal(out, out_m) and torch.equal(lse, lse_m)
    dqkv = K.attention_dropout_bwd(qkv, out, dout, lse, B, S, H, hd, p, seed)
    dqkv_m = K.attention_dropout_bwd(qkv, out, dout, lse, B, S, H, hd, p, 0, md)
    for i, name in enumerate(("dq", "dk", "dv")):
        assert torch.equal(dqkv[:, :, i], dqkv_m[:, :, i]), name


def test_attention_philox_mask_statistics_seeds_and_counter(dev, K):
    B, S, H, hd, p, seed = 2, 200, 1, 32, 0.1, 99
    m = _recover_attn_mask(K, dev, B, S, H, hd, p, seed)
    _residue_rates_ok(m, p, S)                                            # n = 20000 per residue: +- 0.0106
    assert not torch.equal(m[0, 0], m[1, 0])
    assert not torch.equal(m, _recover_attn_mask(K, dev, B, S, H, hd, p, seed + 1))
    c0, c1 = torch.zeros(1, dtype=torch.int64, device=dev), torch.ones(1, dtype=torch.int64, device=dev)
    assert torch.equal(m, _recover_attn_mask(K, dev, B, S, H, hd, p, seed, c0))
    m1 = _recover_attn_mask(K, dev, B, S, H, hd, p, seed, c1)
    assert not torch.equal(m, m1) and torch.equal(m1, _host_attn_mask(B, S, H, p, seed, 1))


# ---------------------------------------------------------------------------------------------- 3. dropout + residual + LayerNorm
def _ln_errs(K, dev, t, res, mask, gamma, beta, p, eps, dy):
    y_ref, dt_ref, dres_ref = _ln_ref(t, res, mask, gamma, beta, p, eps, dy)
    d = lambda v: v.to(dev)        # noqa: E731
    y, rstd = K.dropout_add_layernorm_fwd(d(t), d(res), d(gamma), d(beta), eps, p, 0, d(mask) if p > 0 else None)
    dt, dres = K.dropout_add_layernorm_bwd(d(dy), y, d(gamma), d(beta), rstd, p, 0, d(mask) if p > 0 else None)
    assert torch.isfinite(y).all() and torch.isfinite(dt).all() and torch.isfinite(dres).all()
    return dict(y=_rel(y, y_ref), dt=_rel(dt, dt_ref), dres=_rel(dres, dres_ref))


# D: a row narrower than a wave (1 and 15 float4), one float4 per lane, and each side of the 512 / 1024 dispatch edges up to the widest row;
# T: a lone row, and row counts that leave one workgroup (four rows) partly empty
@pytest.mark.parametrize("D", [4, 60, 256, 260, 512, 516, 1024, 1028, 2048])
@pytest.mark.parametrize("T", [1, 5, 9])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_dropout_add_layernorm_widths_against_float64(dev, K, T, D, p):
    g = _gen(100 * T + D)
    t, res, dy = (torch.randn(T, D, generator=g) for _ in range(3))
    gamma, beta = 1.0 + 0.1 * torch.randn(D, generator=g), 0.05 * torch.randn(D, generator=g)
    mask = (torch.rand(T, D, generator=g) >= p).float()
    errs = _ln_errs(K, dev, t, res, mask, gamma, beta, p, 1e-12, dy)
    print(errs)
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("T,D", [(5, 60), (7, 768), (6, 2048)])
def test_dropout_add_layernorm_philox_widths(dev, K, T, D):
    """the probe of test_dropout_add_layernorm_philox (t = 1, res = 0, gamma = 1, beta = 0: kept entries normalise to positive values, dropped
    ones to negative) at a row narrower than a wave, at three float4 per lane and at the widest row"""
    p, seed = 0.1, 1234
    want = _host_ln_mask(T, D, p, seed)
    assert ((want.sum(1) > 0) & (want.sum(1) < D)).all()                 # the probe needs a kept and a dropped entry in every row
    one, zero = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    probe, _ = K.dropout_add_layernorm_fwd(torch.ones(T, D, device=dev), torch.zeros(T, D, device=dev), one, zero, 1e-12, p, seed)
    m = (probe > 0).float()
    assert torch.equal(m.cpu(), want)                                     # the stream of tests/philox_ref.py
    _residue_rates_ok(m.cpu(), p, D)
    g = _gen(5 + D)
    t, res, dy = (torch.randn(T, D, generator=g).to(dev) for _ in range(3))
    gamma, beta = (1.0 + 0.1 * torch.randn(D, generator=g)).to(dev), (0.05 * torch.randn(D, generator=g)).to(dev)
    y, rstd = K.dropout_add_layernorm_fwd(t, res, gamma, beta, 1e-12, p, seed)
    y_m, rstd_m = K.dropout_add_layernorm_fwd(t, res, gamma, beta, 1e-12, p, 0, m)
    assert torch.equal(y, y_m) and torch.equal(rstd, rstd_m)
    dt, dres = K.dropout_add_layernorm_bwd(dy, y, gamma, beta, rstd, p, seed)
    dt_m, dres_m = K.dropout_add_layernorm_bwd(dy, y, gamma, beta, rstd, p, 0, m)
    assert torch.equal(dt, dt_m) and torch.equal(dres, dres_m)


def test_dropout_add_layernorm_backward_with_small_gamma(dev, K):
    """the backward recovers xhat = (y - beta) / gamma from the forward's output.  |gamma| log-uniform in [2^-5, 2] with random sign and beta
    uniform in [-2, 2]: delta xhat ~ 2^-23 (|y| + |beta|) / |gamma| ~ 1e-5 at the smallest gamma, entering dres through xhat mean(dy gamma xhat).
    That is about 1e-6 in dres.  Measured on an MI355X: y 1.1e-7, dt 1.6e-7, dres 1.8e-7."""
    T, D, p = 64, 768, 0.1
    g = _gen(768)
    t, res, dy = (torch.randn(T, D, generator=g) for _ in range(3))
    sign = torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)
    gamma = sign * torch.exp2(-5.0 + 6.0 * torch.rand(D, generator=g))
    beta = 4.0 * torch.rand(D, generator=g) - 2.0
    assert gamma.abs().min() < 2 ** -4.9 and gamma.abs().max() > 1.9
    mask = (torch.rand(T, D, generator=g) >= p).float()
    errs = _ln_errs(K, dev, t, res, mask, gamma, beta, p, 1e-12, dy)
    print(errs)
    assert max(errs.values()) <= TOL, errs


def test_bad_arguments_are_refused_before_any_launch(dev, K):
    E = K._C.ActHipError
    z = lambda *s: torch.zeros(*s, device=dev)        # noqa: E731

    def ln(T, D, p):
        y, rstd = z(T, D), z(T)
        with pytest.raises(E):
            K.dropout_add_layernorm_fwd(z(T, D), z(T, D), z(D) + 1, z(D), 1e-12, p, 1)
        with pytest.raises(E):
            K.dropout_add_layernorm_bwd(z(T, D), y, z(D) + 1, z(D), rstd, p, 1)
    ln(2, 6, 0.1)
    ln(2, 2052, 0.1)
    ln(2, 64, 1.0)
    ln(2, 64, -0.1)

    def attn(B, S, H, hd, p, mask=None):
        qkv = z(B, S, 3, H, hd)
        with pytest.raises(E):
            K.attention_dropout_fwd(qkv, B, S, H, hd, p, 1, mask)
        with pytest.raises(E):
            K.attention_dropout_bwd(qkv, z(B * S, H * hd), z(B * S, H * hd), z(B, H, S), B, S, H, hd, p, 1, mask)
    attn(1, 4, 1, 48, 0.1)
    attn(65536, 1, 1, 32, 0.1)
    attn(1, 4, 1, 32, 1.0)
    attn(0, 4, 1, 48, 0.1)                                                              # an empty batch is validated too
    attn(1, 4, 2, 32, 0.1, torch.ones(1, 2, 4, 4, device=dev))                          # a float mask
    attn(1, 4, 2, 32, 0.1, torch.ones(1, 2, 4, 4, dtype=torch.bool, device=dev))
    attn(1, 4, 2, 32, 0.1, torch.ones(2, 1, 4, 4, dtype=torch.uint8, device=dev))       # [H, B, S, S]
    attn(1, 4, 2, 32, 0.1, torch.ones(1, 2, 4, 5, dtype=torch.uint8, device=dev))


def test_empty_batches_return_empty_tensors(dev, K):
    z = lambda *s: torch.zeros(*s, device=dev)        # noqa: E731
    D = 64
    y, rstd = K.dropout_add_layernorm_fwd(z(0, D), z(0, D), z(D) + 1, z(D), 1e-12, 0.1, 1)
    assert y.shape == (0, D) and rstd.shape == (0,)
    dt, dres = K.dropout_add_layernorm_bwd(z(0, D), y, z(D) + 1, z(D), rstd, 0.1, 1)
    assert dt.shape == (0, D) and dres.shape == (0, D)
    B, S, H, hd = 0, 5, 2, 32
    out, lse = K.attention_dropout_fwd(z(B, S, 3, H, hd), B, S, H, hd, 0.1, 1)
    assert out.shape == (0, H * hd) and lse.shape == (0, H, S)
    dqkv = K.attention_dropout_bwd(z(B, S, 3, H, hd), out, z(0, H * hd), lse, B, S, H, hd, 0.1, 1)
    assert dqkv.shape == (0, S, 3, H, hd)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 4. the layer
LAYER = dict(B=2, S=37, D=192, H=3, inter=384, p=0.1)


def _layer_state_dict(w, D):
    cpu = {k: v.detach().cpu() for k, v in w.items()}
    sd = {}
    for i, n in enumerate(("query", "key", "value")):
        sd[f"attention.self.{n}.weight"], sd[f"attention.self.{n}.bias"] = cpu["wqkv"][i * D:(i + 1) * D], cpu["bqkv"][i * D:(i + 1) * D]
    for n, (wk, bk) in {"attention.output.dense": ("wo", "bo"), "attention.output.LayerNorm": ("g1", "b1"), "intermediate.dense": ("wi", "bi"),
                        "output.dense": ("wo2", "bo2"), "output.LayerNorm": ("g2", "b2")}.items():
        sd[n + ".weight"], sd[n + ".bias"] = cpu[wk], cpu[bk]
    return sd


def _run_layer(K, w, x, dy, H, p, seeds=(0, 0, 0), masks=None):
    x = x.detach().clone().requires_grad_(True)
    y = K.bert_layer(x, *w.values(), H, 1e-12, p, p, seeds, masks)
    y.backward(dy)
    return y.detach(), x.grad


def test_layer_with_injected_masks_against_float64(dev, K):
    B, S, D, H, inter, p = (LAYER[k] for k in ("B", "S", "D", "H", "inter", "p"))
    w = _layer_weights(dev, D, inter, 7)
    g = _gen(8)
    x, dy = torch.randn(B, S, D, generator=g), torch.randn(B, S, D, generator=g)
    m_attn = (torch.rand(B, H, S, S, generator=g) >= p).to(torch.uint8)
    m_h1, m_h2 = ((torch.rand(B, S, D, generator=g) >= p).float() for _ in range(2))
    xr = x.double().requires_grad_(True)
    y_ref = BR.bert_layer(xr, _layer_state_dict(w, D), "", H, m_attn, m_h1, m_h2, p, 1e-12)
    y_ref.backward(dy.double())
    y, dx = _run_layer(K, w, x.to(dev), dy.to(dev), H, p, masks=(m_attn.to(dev), m_h1.to(dev), m_h2.to(dev)))
    errs = dict(y=_rel(y, y_ref), dx=_rel(dx, xr.grad))
    print(errs)
    assert max(errs.values()) <= TOL, errs


def test_layer_with_seeds_backward_uses_the_forward_masks(dev, K):
    """the training path: nothing is stored, so the backward regenerates all three masks.  The masks of seeds (11, 12, 13) are recovered at
    kernel level; the layer with those masks injected must give the seeded run's y and dx bit for bit."""
    B, S, D, H, inter, p = (LAYER[k] for k in ("B", "S", "D", "H", "inter", "p"))
    seeds = (11, 12, 13)
    w = _layer_weights(dev, D, inter, 7)
    g = _gen(9)
    x, dy = torch.randn(B, S, D, generator=g).to(dev), torch.randn(B, S, D, generator=g).to(dev)
    y, dx = _run_layer(K, w, x, dy, H, p, seeds)
    y2, dx2 = _run_layer(K, w, x, dy, H, p, seeds)
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    m_attn = _recover_attn_mask(K, dev, B, S, H, D // H, p, seeds[0])
    T = B * S
    one, zero = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    hidden = []
    for s in seeds[1:]:
        probe, _ = K.dropout_add_layernorm_fwd(torch.ones(T, D, device=dev), torch.zeros(T, D, device=dev), one, zero, 1e-12, p, s)
        hidden.append((probe > 0).float().view(B, S, D))
        assert torch.equal(hidden[-1].cpu().view(T, D), _host_ln_mask(T, D, p, s))
    assert not torch.equal(hidden[0], hidden[1])
    y_m, dx_m = _run_layer(K, w, x, dy, H, p, masks=(m_attn.to(dev), hidden[0], hidden[1]))
    assert torch.equal(y, y_m), _rel(y, y_m)
    assert torch.equal(dx, dx_m), _rel(dx, dx_m)
