"""Keys / values of the teacher's prompt rows with the dropped terms walked sparsely (csrc/prompt_kv.hip, K.prompt_kv) against the rows of
K.prompt_layernorm (same mask) multiplied in float64."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

BAR = 2e-5          # the project's bar for fp32 products (test_gpu_dense.py)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _rel(a, ref):
    a = a.detach().double().cpu(); ref = ref.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return ((a - ref).abs().max() / max(1.0, ref.abs().max())).item()


def _inputs(P, D, N, dev, offset=0.0, seed=0):
    g = torch.Generator().manual_seed(1000 + 7 * P + D + N + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    tok, ppos = r(P, D), r(P, D) * 0.5 + offset
    gamma, beta = 1.0 + 0.2 * r(D), 0.1 * r(D)
    w, bias = r(N, D) / D ** 0.5, 0.1 * r(N)
    return [t.to(dev) for t in (tok, ppos, gamma, beta, w, bias)]


def _three(tok, ppos, B, drop_p, seed, gamma, beta, w, bias, seed_dev=None):
    """(sparse path, dense path, float64 reference from the rows of the existing kernel)"""
    import act_amd.kernels as K
    assert K.lib.act_prompt_kv_sparse(-1) == 1
    got = K.prompt_kv(tok, ppos, B, drop_p, seed, gamma, beta, 1e-6, w, bias, seed_dev=seed_dev)
    rows = K.prompt_layernorm(tok, ppos, B, drop_p, seed, gamma, beta, 1e-6, seed_dev=seed_dev)
    dense = K.gemm(rows, w, True, True, bias=bias)
    ref = rows.double() @ w.double().T + bias.double()
    return got, dense, ref


@pytest.mark.parametrize("B,P,D,N", [(3, 5, 128, 256), (2, 64, 768, 1536), (7, 16, 64, 128), (3, 5, 128, 201)])
@pytest.mark.parametrize("drop_p", [0.0, 0.1, 0.5])
def test_prompt_kv_matches_float64_rows(dev, B, P, D, N, drop_p):
    tok, ppos, gamma, beta, w, bias = _inputs(P, D, N, dev)
    got, dense, ref = _three(tok, ppos, B, drop_p, 5, gamma, beta, w, bias)
    e_new, e_dense = _rel(got, ref), _rel(dense, ref)
    print(f"prompt_kv B={B} P={P} D={D} N={N} p={drop_p}: sparse {e_new:.3e}  dense {e_dense:.3e}")
    assert e_new <= BAR
    if drop_p == 0.0:                                  # no dropout: every cloud's rows are the same bits
        v = got.view(B, P, N)
        assert all(torch.equal(v[0], v[b]) for b in range(1, B))


def test_prompt_kv_device_seed(dev):
    B, P, D, N = 3, 5, 128, 256
    tok, ppos, gamma, beta, w, bias = _inputs(P, D, N, dev)
    ctr = torch.tensor([12345], dtype=torch.int64, device=dev)
    got, dense, ref = _three(tok, ppos, B, 0.1, 5, gamma, beta, w, bias, seed_dev=ctr)
    e_new, e_dense = _rel(got, ref), _rel(dense, ref)
    print(f"prompt_kv seed_dev: sparse {e_new:.3e}  dense {e_dense:.3e}")
    assert e_new <= BAR
    import act_amd.kernels as K
    plain = K.prompt_kv(tok, ppos, B, 0.1, 5, gamma, beta, 1e-6, w, bias)
    assert not torch.equal(plain, got)                 # the counter is part of the key


def test_prompt_kv_large_common_offset(dev):
    """ppos + 3.0: the row mean dwarfs the spread; the form centred on the undropped mean stays inside the same bar"""
    B, P, D, N = 2, 64, 768, 1536
    tok, ppos, gamma, beta, w, bias = _inputs(P, D, N, dev, offset=3.0)
    got, dense, ref = _three(tok, ppos, B, 0.1, 9, gamma, beta, w, bias)
    e_new, e_dense = _rel(got, ref), _rel(dense, ref)
    print(f"prompt_kv offset 3.0: sparse {e_new:.3e}  dense {e_dense:.3e}")
    assert e_new <= BAR


def test_prompt_kv_determinism_and_seeds(dev):
    import act_amd.kernels as K
    B, P, D, N = 7, 16, 64, 128
    tok, ppos, gamma, beta, w, bias = _inputs(P, D, N, dev)
    a = K.prompt_kv(tok, ppos, B, 0.1, 5, gamma, beta, 1e-6, w, bias)
    b = K.prompt_kv(tok, ppos, B, 0.1, 5, gamma, beta, 1e-6, w, bias)
    c = K.prompt_kv(tok, ppos, B, 0.1, 6, gamma, beta, 1e-6, w, bias)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    v = a.view(B, P, N)
    assert not torch.equal(v[0], v[1])


def test_prompt_kv_unsupported_shape_runs_dense(dev):
    """D = 1536: the 32-column weight tile does not fit LDS -> the entry reports it and the wrapper runs today's sequence"""
    import act_amd.kernels as K
    B, P, D, N = 2, 3, 1536, 64
    assert K.lib.act_prompt_kv_workspace(B, P, D, N) == 0
    tok, ppos, gamma, beta, w, bias = _inputs(P, D, N, dev)
    got = K.prompt_kv(tok, ppos, B, 0.1, 5, gamma, beta, 1e-6, w, bias)
    rows = K.prompt_layernorm(tok, ppos, B, 0.1, 5, gamma, beta, 1e-6)
    assert torch.equal(got, K.gemm(rows, w, True, True, bias=bias))
    z = torch.zeros(4, device=dev)
    rc = K.lib.act_prompt_kv_fwd_f32(tok.data_ptr(), ppos.data_ptr(), B, P, D, N, 0.1, 5, None, gamma.data_ptr(), beta.data_ptr(), 1e-6, w.data_ptr(),
                                     bias.data_ptr(), got.data_ptr(), z.data_ptr(), 16, None, 0, None)
    assert rc == -3


def test_prompt_kv_switch(dev, monkeypatch):
    """ACT_PROMPT_KV_SPARSE=0 (act_prompt_kv_sparse(0) at run time): the teacher's features are the bits of the dense form -- prompt_layernorm + GEMM per
    layer, what the per-kernel path ran before -- and the sparse form stays within 1e-5 of them for the same seed."""
    import act_amd.composite as CP
    import act_amd.kernels as K
    from act_amd.models import build_model_from_cfg
    from act_amd.utils.config import EasyDict
    from tests.golden.fill import fill_module, clouds, TINY_STAGE2
    cfg = copy.deepcopy(TINY_STAGE2["dvae_config"]); cfg["NAME"] = "ACTPromptedDiscreteVAEwithVIT"
    torch.manual_seed(3)
    vae = fill_module(build_model_from_cfg(EasyDict(cfg)), "cmp.vae.").to(dev).train()
    for p in vae.parameters():
        p.requires_grad = False
    pts = torch.from_numpy(clouds(31, 3, 128)).to(dev)

    def run():
        vae.__dict__.pop("_rng_state", None)
        torch.manual_seed(77)
        with torch.no_grad():
            nb, c = vae.group_divider(pts)
            f = vae.forward_tokenizer_features(nb, c)
        torch.cuda.synchronize()
        return f

    def dense_form(tok, ppos, B, drop_p, seed, gamma, beta, eps, w, bias=None, seed_dev=None):
        return K.gemm(K.prompt_layernorm(tok, ppos, B, drop_p, seed, gamma, beta, eps, seed_dev=seed_dev), w, True, True, bias=bias)

    assert K.lib.act_prompt_kv_sparse(-1) == 1
    on = run()
    prev = K.lib.act_prompt_kv_sparse(0)
    try:
        off = run()
        saved, CP.ENABLED = CP.ENABLED, False
        try:
            with monkeypatch.context() as mp:
                mp.setattr(K, "prompt_kv", dense_form)
                parent = run()
        finally:
            CP.ENABLED = saved
    finally:
        K.lib.act_prompt_kv_sparse(prev)
    assert torch.equal(off, parent)
    e = _rel(on, off)
    print(f"prompt_kv switch on vs off: {e:.3e}")
    assert e <= 1e-5
