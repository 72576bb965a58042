"""The OPT-IN split-bf16 path of the frozen teacher (csrc/gemm_bf16x3.hip, ACT_TEACHER_BF16X3=1): never the default, never in a headline number.
Kernel level: the plane split is exact (hi + lo reproduces the first 16 significand bits, round to nearest even), the three-product GEMM agrees with an
fp64 product of the ORIGINAL fp32 operands to 2e-5 and with an fp32 emulation of its own arithmetic much closer, with every epilogue the teacher uses.
Model level: the teacher's features with the switch on stay within the 1e-4 parity bar of the f32 path (measured ~7e-6) and of the CPU oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def test_split_planes_are_the_rne_bf16_decomposition(dev):
    import act_amd.kernels as K
    torch.manual_seed(0)
    x = torch.randn(256, 192, device=dev) * torch.logspace(-3, 3, 192, device=dev)
    pl = K.split_bf16x2(x)
    assert pl.dtype == torch.bfloat16 and tuple(pl.shape) == (2, 256, 192)
    hi = x.bfloat16()                                             # torch rounds to nearest even as well
    lo = (x - hi.float()).bfloat16()
    assert torch.equal(pl[0], hi) and torch.equal(pl[1], lo)
    # what the two planes keep: 16 significand bits
    err = (pl[0].float() + pl[1].float() - x).abs() / x.abs().clamp_min(1e-30)
    assert err.max().item() <= 2.0 ** -16
    # a row-strided view (column slice of a wider tensor) splits like its contiguous copy
    wide = torch.randn(128, 512, device=dev)
    v = wide[:, 128:384]
    assert torch.equal(K.split_bf16x2(v), K.split_bf16x2(v.contiguous()))


@pytest.mark.parametrize("M,N,Kd,bias,act,res", [(256, 128, 64, False, 0, False), (8192, 768, 768, True, 0, True), (1024, 3072, 768, True, 1, False),
                                                  (512, 768, 3072, True, 0, True), (384, 2304, 768, True, 0, False)])
def test_bf16x3_gemm_against_fp64_and_its_own_arithmetic(dev, M, N, Kd, bias, act, res):
    import act_amd.kernels as K
    g = torch.Generator().manual_seed(M + N + Kd)
    a = (torch.randn(M, Kd, generator=g) * 1.5).to(dev); w = (torch.randn(N, Kd, generator=g) * 0.05).to(dev)
    b = torch.randn(N, generator=g).to(dev) if bias else None
    r = torch.randn(M, N, generator=g).to(dev) if res else None
    ap, wp = K.split_bf16x2(a), K.split_bf16x2(w)
    out = K.gemm_nt_bf16x3(ap, wp, bias=b, act=(K.EPI_GELU if act else K.EPI_NONE), res=r)

    def epi(y):
        if b is not None:
            y = y + b.double()
        if act:
            y = torch.nn.functional.gelu(y)
        if r is not None:
            y = y + r.double()
        return y
    exact = epi(a.double() @ w.double().t())
    assert _rel(out, exact) <= 2e-5, _rel(out, exact)
    # the kernel's own arithmetic in fp64: (hi.hi + hi.lo + lo.hi) of the planes -- what is left is fp32 accumulation order only
    ah, al, wh, wl = (t.double() for t in (ap[0], ap[1], wp[0], wp[1]))
    own = epi(al @ wh.t() + ah @ wl.t() + ah @ wh.t())
    assert _rel(out, own) <= 2e-6, _rel(out, own)
    # and it is the SAME fp32 epilogue as the f32 kernel's (bias, exact-erf GELU, residual): compare against the product path on the same operands
    ref32 = K.gemm(a, w, True, True, bias=b, act=(K.EPI_GELU if act else K.EPI_NONE), res=r)
    assert _rel(out, ref32) <= 2e-5


def test_bf16x3_planes_output_is_the_split_of_the_fp32_output(dev):
    """the epilogue can hand its result on as (hi, lo) planes (teacher MLP: fc1 + GELU -> planes -> fc2, the hidden activation never exists in fp32):
    bit-identical to splitting the fp32 result afterwards"""
    import act_amd.kernels as K
    g = torch.Generator().manual_seed(7)
    a = torch.randn(384, 768, generator=g).to(dev); w = (torch.randn(3072, 768, generator=g) * 0.05).to(dev); b = torch.randn(3072, generator=g).to(dev)
    ap, wp = K.split_bf16x2(a), K.split_bf16x2(w)
    planes = torch.empty(2, 384, 3072, dtype=torch.bfloat16, device=dev)
    out = K.gemm_nt_bf16x3(ap, wp, bias=b, act=K.EPI_GELU, planes_out=planes)
    assert torch.equal(out, K.gemm_nt_bf16x3(ap, wp, bias=b, act=K.EPI_GELU))
    assert torch.equal(planes, K.split_bf16x2(out))


def test_producers_that_emit_planes_equal_a_split_of_their_fp32_result(dev):
    """LayerNorm writing planes == split(LayerNorm) bit for bit; the prefix attention forward writing planes == split(its fp32 output); the prompt
    LayerNorm writing planes == split(prompt LayerNorm) for the same seed, without and with dropout (ten rows of 264: the last four-row workgroup and the
    second 64-lane chunk of 66 float4 are both ragged)"""
    import ctypes
    import act_amd.kernels as K
    from act_amd import _C
    torch.manual_seed(3)
    x = torch.randn(512, 768, device=dev); pos = 0.1 * torch.randn(512, 768, device=dev)
    g = 1 + 0.1 * torch.randn(768, device=dev); b = 0.1 * torch.randn(768, device=dev)
    y, _, _, _ = K.layernorm_fwd(x, pos, g, b, 1e-6, want_stats=False)
    assert torch.equal(K.layernorm_planes(x, g, b, 1e-6, pos=pos), K.split_bf16x2(y))
    B, S0, Sq, H, hd = 4, 64, 64, 12, 64
    kv0 = torch.randn(B * S0, 2 * H * hd, device=dev); qkv = torch.randn(B * Sq, 3 * H * hd, device=dev)
    out = K.attention_fwd_prefix(kv0, S0, qkv, Sq, B, H, hd)
    planes = torch.empty(2, B * Sq, H * hd, dtype=torch.bfloat16, device=dev)
    _C.check(_C.lib.act_attention_fwd_prefix_planes_f32(_C.ptr(kv0), S0, _C.ptr(qkv), Sq, None, _C.ptr(planes[0]), _C.ptr(planes[1]), None, B, H, hd,
                                                        float(hd) ** -0.5, _C.stream()), "act_attention_fwd_prefix_planes_f32")
    assert torch.equal(planes, K.split_bf16x2(out))
    B, P, D = 2, 5, 264
    tok = torch.randn(P, D, device=dev); ppos = 0.1 * torch.randn(P, D, device=dev)
    g = 1 + 0.1 * torch.randn(D, device=dev); b = 0.1 * torch.randn(D, device=dev)
    for drop_p, seed in ((0.0, 0), (0.25, 1234)):
        planes = torch.empty(2, B * P, D, dtype=torch.bfloat16, device=dev)
        _C.check(_C.lib.act_prompt_layernorm_fwd_planes_f32(_C.ptr(tok), _C.ptr(ppos), B, P, D, drop_p, seed, None, _C.ptr(g), _C.ptr(b), 1e-6,
                                                            _C.ptr(planes[0]), _C.ptr(planes[1]), _C.stream()), "act_prompt_layernorm_fwd_planes_f32")
        assert torch.equal(planes, K.split_bf16x2(K.prompt_layernorm(tok, ppos, B, drop_p, seed, g, b, 1e-6))), drop_p


def test_bf16x3_rejects_what_it_does_not_support(dev):
    import act_amd.kernels as K
    from act_amd._C import ActHipError
    a = K.split_bf16x2(torch.randn(128, 64, device=dev)); w = K.split_bf16x2(torch.randn(128, 64, device=dev))
    K.gemm_nt_bf16x3(a, w)
    for bad_a, bad_w in ((K.split_bf16x2(torch.randn(96, 64, device=dev)), w), (K.split_bf16x2(torch.randn(128, 32, device=dev)), K.split_bf16x2(torch.randn(128, 32, device=dev)))):
        with pytest.raises(ActHipError):
            K.gemm_nt_bf16x3(bad_a, bad_w)
    with pytest.raises(ActHipError):
        K.gemm_nt_bf16x3(a.float(), w)


def test_teacher_features_with_split_bf16_stay_inside_the_parity_bar(dev):
    """ACT_TEACHER_BF16X3 semantics (composite.TEACHER_BF16X3 = True): the five Linear products of every ViT layer of the frozen teacher on the split-bf16
    kernel.  Full configs[1] geometry, B = 8: features within 1e-4 of the f32 HIP path AND of the CPU oracle (max |e| / max |ref|; the oracle emulation
    predicts 6e-6), the default path untouched (bit-identical before / after the switch was used)."""
    import act_amd.composite as CP
    if not hasattr(CP, "TEACHER_BF16X3"):
        pytest.skip("the teacher-side switch is not wired in this build")
    from oracle import models as OM, layers as OL
    from act_amd.models import build_model_from_cfg
    from act_amd.utils.config import cfg_from_yaml_file
    from act_amd.utils.draws import Draws
    from tests.golden.fill import clouds
    cfg = cfg_from_yaml_file("cfgs/pretrain/pretrain_act_distill.yaml").model
    cfg.dvae_config.ckpt = "none"
    torch.manual_seed(2)
    oracle = OM.ACT_PointDistillation(OM.edict(cfg)).train()
    model = build_model_from_cfg(cfg)
    model.load_state_dict(oracle.state_dict(), strict=True)
    model.to(dev).train()
    oracle.dvae_tokenizer.prompt_p = 0.0; model.dvae_tokenizer.prompt_dropout.p = 0.0      # (the fused stack draws its prompt dropout in-kernel: switch it off)
    pts = torch.from_numpy(clouds(6, 8, 1024))
    with torch.no_grad():
        nb_o, c_o = oracle.group_divider(pts)
        rec = OL.Draws(record=True)
        tf_o = oracle.dvae_tokenizer.forward_tokenizer_features(nb_o, c_o, rec)
        nb, c = model.group_divider(pts.to(dev))
        gum = Draws({"gumbel": rec.table["gumbel"]}, device=dev)
        saved = CP.TEACHER_BF16X3
        try:
            CP.TEACHER_BF16X3 = False
            f32_a = model.dvae_tokenizer.forward_tokenizer_features(nb, c, draws=Draws({"gumbel": rec.table["gumbel"]}, device=dev))
            CP.TEACHER_BF16X3 = True
            x3 = model.dvae_tokenizer.forward_tokenizer_features(nb, c, draws=Draws({"gumbel": rec.table["gumbel"]}, device=dev))
            CP.TEACHER_BF16X3 = False
            f32_b = model.dvae_tokenizer.forward_tokenizer_features(nb, c, draws=Draws({"gumbel": rec.table["gumbel"]}, device=dev))
        finally:
            CP.TEACHER_BF16X3 = saved
    assert torch.equal(f32_a, f32_b)
    assert not torch.equal(x3, f32_a)                             # the switch really took the other kernels
    e32, eo = _rel(x3, f32_a), _rel(x3, tf_o)
    print(f"split-bf16 teacher: max|e|/max|ref| vs f32 HIP path {e32:.2e}, vs CPU oracle {eo:.2e} (f32 path vs oracle {_rel(f32_a, tf_o):.2e})")
    assert e32 <= 1e-4 and eo <= 1e-4
    assert e32 <= 3e-5                                            # far inside the bar, as the oracle emulation predicts


@pytest.mark.parametrize("B", [1, 2])
def test_split_bf16_teacher_at_the_stress_geometry_and_with_mixed_kernels(dev, B):
    """configs[4] geometry (64 prompts + 512 tokens, d = 768): at B = 1 the prompt rows (64) are not a multiple of the kernel's 128-row tile, so the K / V product of
    the prompts stays on the f32 kernel while the other four go to the split-bf16 kernel (the per-product fallback inside one block); at B = 2 all five go.
    Features within 1e-4 of the f32 path either way."""
    import act_amd.composite as CP
    from act_amd.models import build_model_from_cfg
    from act_amd.utils.config import cfg_from_yaml_file
    from act_amd.utils.draws import Draws
    from tests.golden.fill import clouds
    cfg = cfg_from_yaml_file("cfgs/pretrain/pretrain_act_distill.yaml").model
    cfg.dvae_config.ckpt = "none"
    for k in ("encoder_dims", "tokens_dims", "decoder_dims"):
        cfg.dvae_config[k] = 768
    cfg.dvae_config.num_group = 512; cfg.dvae_config.group_size = 64
    cfg.transformer_config.embed_dim = 768; cfg.transformer_config.encoder_dims = 768; cfg.transformer_config.depth = 2
    cfg.transformer_config.num_heads = 12; cfg.transformer_config.decoder_num_heads = 12
    torch.manual_seed(4)
    model = build_model_from_cfg(cfg).to(dev).train()
    model.dvae_tokenizer.prompt_dropout.p = 0.0
    pts = torch.from_numpy(clouds(9, B, 8192)).to(dev)
    gum = -torch.empty(B, 512, 8192).exponential_().log()
    saved = CP.TEACHER_BF16X3
    try:
        with torch.no_grad():
            nb, c = model.group_divider(pts)
            CP.TEACHER_BF16X3 = False
            f32 = model.dvae_tokenizer.forward_tokenizer_features(nb, c, draws=Draws({"gumbel": gum}, device=dev))
            CP.TEACHER_BF16X3 = True
            x3 = model.dvae_tokenizer.forward_tokenizer_features(nb, c, draws=Draws({"gumbel": gum}, device=dev))
    finally:
        CP.TEACHER_BF16X3 = saved
    assert not torch.equal(x3, f32)
    e = _rel(x3, f32)
    print(f"stress geometry B={B}: split-bf16 teacher vs f32 path {e:.2e}")
    assert e <= 3e-5


@pytest.mark.parametrize("B,P,G", [(4, 32, 64), (2, 24, 64)])
def test_stage1_prefix_block_forward_in_split_bf16_keeps_the_f32_backward_exact_enough(dev, B, P, G):
    """The differentiable prefix block of Stage-I prompt tuning (composite.PrefixBlockFn) with the switch on: the frozen block's forward products run on the
    split-bf16 kernel (B=4, P=32: all five; B=2, P=24: the prompt K/V product -- 48 rows -- stays f32); the backward either the unchanged f32 one
    (ACT_TEACHER_BF16X3_BWD=0) reading what the forward still writes in fp32, or with its five input-gradient products on the split-bf16 kernel too (default
    when the switch is on).  Output and the gradients w.r.t. tokens, positions and prompts within 3e-5 of the all-f32 path (bar 1e-4)."""
    import act_amd.composite as CP
    D, H, Hd = 768, 12, 3072
    g = torch.Generator().manual_seed(31)
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dev)
    prm_ = [1 + rn(D, sc=0.1), rn(D, sc=0.1), rn(3 * D, D, sc=D ** -0.5), rn(3 * D, sc=0.02), rn(D, D, sc=D ** -0.5), rn(D, sc=0.02),
            1 + rn(D, sc=0.1), rn(D, sc=0.1), rn(Hd, D, sc=D ** -0.5), rn(Hd, sc=0.02), rn(D, Hd, sc=Hd ** -0.5), rn(D, sc=0.02)]
    x0, p0, m0, w = rn(B * G, D), rn(B * G, D, sc=0.2), rn(B * P, D, sc=0.3), rn(B * G, D)

    def run(on, bwd=False):
        saved = CP.TEACHER_BF16X3, CP.TEACHER_BF16X3_BWD
        CP.TEACHER_BF16X3, CP.TEACHER_BF16X3_BWD = on, bwd
        try:
            x, p, m = (t.clone().requires_grad_(True) for t in (x0, p0, m0))
            y = CP.PrefixBlockFn.apply(x, p, m, B, P, G, *prm_, H, 1e-6)
            (y * w).sum().backward()
            return y.detach(), x.grad, p.grad, m.grad
        finally:
            CP.TEACHER_BF16X3, CP.TEACHER_BF16X3_BWD = saved
    ref, got, both = run(False), run(True), run(True, True)
    assert not torch.equal(got[0], ref[0])                        # the split-bf16 kernel really ran
    assert torch.equal(both[0], got[0]) and not torch.equal(both[1], got[1])     # ... and so did the split-bf16 backward products
    for tag, res in (("forward", got), ("forward + backward", both)):
        for name, a, b in zip(("out", "dx", "dpos", "dprompt"), res, ref):
            e = _rel(a, b)
            print(f"stage-I prefix block B={B} P={P} {name}: split-bf16 {tag} vs f32 {e:.2e}")
            assert e <= 3e-5, (tag, name, e)
    # a block whose weights train is never routed there
    prm_[2].requires_grad_(True)
    try:
        again = run(True)
    finally:
        prm_[2].requires_grad_(False)
    assert torch.equal(again[0], ref[0])


def test_stage1_step_with_split_bf16_forward_matches_the_f32_step(dev):
    """One Stage-I step of the shipped configs[2] model at B=8 with the switch on vs off, every draw replayed: losses, fine reconstruction within 1e-4.  The
    gradients of this graph are discontinuous in its activations (Chamfer arg-min, max-pool and ReLU decisions reroute whole gradient rows: the same reason the
    oracle comparison of tests/test_gpu_model.py is noise-aware), so they are held to a CONTROL: the all-f32 step with proj_pre.bias moved by 1e-5 -- a
    perturbation of the Transformer's input of the size of the split-bf16 error.  The split-bf16 step's gradients may differ from the f32 step's by at most
    3x what that control differs (or 1e-4 relative L2, whichever is larger)."""
    import act_amd.composite as CP
    from act_amd.models import build_model_from_cfg
    from act_amd.utils.config import cfg_from_yaml_file
    from act_amd.utils.draws import Draws
    from tests.golden.fill import clouds
    cfg = cfg_from_yaml_file("cfgs/autoencoder/act_dvae_with_pretrained_transformer.yaml").model
    torch.manual_seed(5)
    vae = build_model_from_cfg(cfg).to(dev).train()
    vae.prompt_dropout.p = 0.0
    B = 8
    pts = torch.from_numpy(clouds(11, B, 1024)).to(dev)
    gum = -torch.empty(B, 64, 8192).exponential_().log()
    names = ["deep_prompt_tokens", "visual_prompt_token", "visual_prompt_pos", "proj_pre.weight", "proj_post.weight", "encoder.first_conv.0.weight", "codebook"]
    bias0 = vae.proj_pre.bias.detach().clone()
    nudge = 1e-5 * torch.randn(bias0.shape, generator=torch.Generator().manual_seed(3)).to(dev)

    def step(on, nudged):
        saved = CP.TEACHER_BF16X3
        CP.TEACHER_BF16X3 = on                                     # (TEACHER_BF16X3_BWD at its default: on -> forward AND backward products)
        try:
            with torch.no_grad():
                vae.proj_pre.bias.copy_(bias0 + nudge if nudged else bias0)
            vae.zero_grad(set_to_none=True)
            r = vae(pts, temperature=0.6, hard=False, draws=Draws({"gumbel": gum}, device=dev))
            lr, lk = vae.get_loss(r, pts)
            (lr + 0.05 * lk).backward()
            pd = dict(vae.named_parameters())
            return lr.item(), lk.item(), r[3].detach().clone(), {n: pd[n].grad.double().clone() for n in names}
        finally:
            CP.TEACHER_BF16X3 = saved
            with torch.no_grad():
                vae.proj_pre.bias.copy_(bias0)
    f32, x3, ctl = step(False, False), step(True, False), step(False, True)
    assert abs(x3[0] - f32[0]) <= 1e-4 and abs(x3[1] - f32[1]) <= 1e-4, (x3[:2], f32[:2])
    assert _rel(x3[2], f32[2]) <= 1e-4
    assert not torch.equal(x3[2], f32[2])                         # the reconstruction comes from after the Transformer: the split-bf16 kernel really ran
    l2 = lambda a, b: ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
    bad = []
    for n in names:
        e, c = l2(x3[3][n], f32[3][n]), l2(ctl[3][n], f32[3][n])
        print(f"stage-I step gradient {n}: split-bf16 forward vs f32 {e:.2e}; control (f32, Transformer input moved by 1e-5) {c:.2e}")
        if e > max(1e-4, 3 * c):
            bad.append((n, e, c))
    assert not bad, bad
