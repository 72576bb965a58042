"""The prompt kernels (csrc/norm.hip, csrc/prompt_kv.hip) against the host stream of tests/philox_ref.py: every dense-row user draws the domain-1
mask of csrc/dropout.h, so host_ln_mask is the mask of prompt_rows, prompt_layernorm and prompt_kv bit for bit, device counter included.
Probe: tok = 1, ppos = 0 (gamma = 1, beta = 0): a kept entry is 1 / (1 - p) and normalises to a positive value, a dropped one is 0 and normalises
to a negative value.  D: narrower than a wave, a one-lane tail in the second float4 chunk, the model width, the widest row."""
import pytest
import torch

from tests.philox_ref import host_ln_mask
from tests.test_gpu_prompt_kv import BAR, _rel

pytestmark = pytest.mark.gpu

B, P, DROP, SEED, CTR = 3, 5, 0.1, 1234, 3
T = B * P
EPS = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def K():
    import act_amd.kernels as K
    return K


_MASKS = {}


def _want(D, ctr=None):
    """the host mask [T, D], computed once per (D, ctr); the probe needs a kept and a dropped entry in every row"""
    if (D, ctr) not in _MASKS:
        m = host_ln_mask(T, D, DROP, SEED, ctr)
        assert ((m.sum(1) > 0) & (m.sum(1) < D)).all()
        _MASKS[(D, ctr)] = m
    return _MASKS[(D, ctr)]


def _probe(D, dev):
    return torch.ones(P, D, device=dev), torch.zeros(P, D, device=dev), torch.ones(D, device=dev), torch.zeros(D, device=dev)


@pytest.mark.parametrize("D", [60, 260, 768, 2048])
def test_prompt_rows_draws_the_host_stream(dev, K, D):
    want = _want(D)
    tok, ppos, _, _ = _probe(D, dev)
    tok.requires_grad_(True)
    y = K.prompt_rows(tok, ppos, B, DROP, SEED)
    yc = y.detach().cpu()
    assert torch.equal((yc != 0).float(), want)
    keep = yc.max().item()
    assert abs(keep - 1.0 / (1.0 - DROP)) <= 1e-6 and torch.equal(yc, want * keep)         # 0 or 1 / (1 - p), nothing else
    dy = torch.randn(T, D, generator=torch.Generator().manual_seed(D)).to(dev)
    (y * dy).sum().backward()
    dtok = (want.double().view(B, P, D) * dy.cpu().double().view(B, P, D) / (1.0 - DROP)).sum(0)
    err = _rel(tok.grad, dtok)
    print(f"prompt_rows D={D}: dtok {err:.3e}")
    assert err <= 2e-6                                                                      # the bar of test_prompt_rows_fwd_bwd


@pytest.mark.parametrize("D", [60, 260, 768, 2048])
def test_prompt_layernorm_draws_the_host_stream(dev, K, D):
    tok, ppos, one, zero = _probe(D, dev)
    y = K.prompt_layernorm(tok, ppos, B, DROP, SEED, one, zero, EPS)
    assert torch.equal((y > 0).float().cpu(), _want(D))
    ctr = torch.tensor([CTR], dtype=torch.int64, device=dev)
    y = K.prompt_layernorm(tok, ppos, B, DROP, SEED, one, zero, EPS, seed_dev=ctr)
    assert torch.equal((y > 0).float().cpu(), _want(D, CTR))
    assert not torch.equal(_want(D), _want(D, CTR))


@pytest.mark.parametrize("D", [260, 768])
def test_prompt_kv_draws_the_host_stream(dev, K, D):
    """w = the first N rows of the identity, bias = 0: output column j is the normalised channel j"""
    N = 64
    if K.lib.act_prompt_kv_workspace(B, P, D, N) == 0:
        pytest.skip(f"act_prompt_kv_workspace reports (B, P, D, N) = {(B, P, D, N)} unsupported")
    assert K.lib.act_prompt_kv_sparse(-1) == 1
    tok, ppos, one, zero = _probe(D, dev)
    w = torch.eye(D, device=dev)[:N].contiguous()
    for ctr in (None, CTR):
        sd = None if ctr is None else torch.tensor([ctr], dtype=torch.int64, device=dev)
        kv = K.prompt_kv(tok, ppos, B, DROP, SEED, one, zero, EPS, w, torch.zeros(N, device=dev), seed_dev=sd)
        assert torch.equal((kv > 0).float().cpu(), _want(D, ctr)[:, :N])
        rows = K.prompt_layernorm(tok, ppos, B, DROP, SEED, one, zero, EPS, seed_dev=sd)
        err = _rel(kv, rows[:, :N])
        print(f"prompt_kv D={D} ctr={ctr}: vs prompt_layernorm {err:.3e}")
        assert err <= BAR
