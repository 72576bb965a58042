"""The DEFAULT arithmetic of the frozen teacher's four Linear products per layer: split-f16 planes with a scaled low plane (csrc/gemm_bf16x3.hip F16 form,
csrc/split_planes.h, ACT_TEACHER_F16X3).  Kernel level: the split equals the numpy restatement (tests/f16x3_ref.py) bit for bit, the GEMM is EXACT on lattice
operands and fp32-grade on real ones (error against float64 within 1.5 x the f32 kernel's, same operands, same test).  Model level: the teacher's features
with the switch on sit as close to the CPU oracle as the f32 path does (within 2 x), the f32 path is untouched, the range guard falls back per Linear, and
the plane cache follows in-place weight changes."""
import copy

import numpy as np
import pytest
import torch

from tests import f16x3_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(128, 128, 64), (256, 384, 192), (1024, 128, 128)]          # (256, 384, 192): 6 workgroups, the XCD remap with a remainder


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _rel_l2(x, ref):
    return ((x.double() - ref).norm() / ref.norm()).item()


def _rel_max(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


# ---- split -------------------------------------------------------------------------------------------------------------------------------------------------
def _edge_values(n, rng):
    """24 threshold values first -- 0, +-2^-14 and its fp32 / f16 neighbours, values whose h1 (or h2) is flushed, 65504 * 2^-k, negatives --, then more
    of the 65504 * 2^-k family and log-uniform magnitudes up to n values"""
    t = np.float32(2.0 ** -14)
    v = [0.0, -0.0, t, -t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0)), -np.nextafter(t, np.float32(0)),
         2.0 ** -14 * (1 + 2.0 ** -10), 2.0 ** -14 * (1 - 2.0 ** -11), 2.0 ** -14 * (1 - 2.0 ** -12),       # the last one rounds UP to 2^-14 and stays
         2.0 ** -15, -2.0 ** -15, 3e-6, -1e-7, 2.0 ** -14 + 2.0 ** -26,                                      # h1 flushed / h2 flushed
         1.0, -1.0 - 2.0 ** -12, 1.0 + 2.0 ** -11, -0.3,
         65504.0, -65504.0 / 2, 65504.0 * 2.0 ** -7, -65504.0 * 2.0 ** -16, 65504.0 * 2.0 ** -29]
    assert len(v) == 24
    if n > 24:
        v += [65504.0 * 2.0 ** -k for k in range(1, 34, 3)] + [-65504.0 * 2.0 ** -k for k in range(2, 30, 4)] + [1.0 + 3 * 2.0 ** -12, 1000.123, -32768.0]
        v += list(rng.standard_normal(n - len(v)) * np.exp(rng.uniform(-12, 9, n - len(v))))
    return np.array(v[:n], dtype=np.float32)


@pytest.mark.parametrize("rows,cols", [(3, 8), (5, 64)])
def test_split_kernel_equals_the_restatement_bit_for_bit(dev, rows, cols):
    import act_amd.kernels as K
    rng = np.random.default_rng(rows)
    x = _edge_values(rows * cols, rng).reshape(rows, cols)
    xt = torch.from_numpy(x).to(dev)
    row_scale = np.ldexp(np.float32(1), rng.integers(-3, 4, rows)).astype(np.float32)
    for scale, rs in ((1.0, None), (0.25, None), (2.0, row_scale)):
        pl = K.split_f16x2(xt, scale, None if rs is None else torch.from_numpy(rs).to(dev))
        s = np.float32(scale) * (rs[:, None] if rs is not None else np.float32(1))
        keep = np.abs(x * s) <= 65504.0                        # (the caller's scale keeps |x s| <= 2^15; beyond f16's range nothing is specified)
        assert keep.all() or scale != 1.0
        h1, h2 = R.split(np.where(keep, x, 0), s)
        got1, got2 = _bits(pl[0]), _bits(pl[1])
        assert np.array_equal(got1[keep], h1.view(np.uint16)[keep]), (scale, np.argwhere(got1 != h1.view(np.uint16))[:4])
        assert np.array_equal(got2[keep], h2.view(np.uint16)[keep]), (scale, np.argwhere(got2 != h2.view(np.uint16))[:4])


# ---- GEMM --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,Kd", SHAPES)
def test_lattice_gemm_is_exact(dev, M, N, Kd):
    """operands i + j 2^-12 with i, j in [-2, 2], restricted to the part of that lattice on which fp32 accumulation is EXACT: i != 0 and j of i's sign or
    zero (plus elements that are exactly zero).  Then h1 = i s and h2 = j s / 2, every plane product and both accumulators are integers times one power of
    two that fit 24 bits, and C must EQUAL sum i_a i_b + 2^-12 sum (i_a j_b + j_a i_b) -- the integer result without the h2.h2 term.  (Left out on purpose:
    i = 0 with j != 0, and j against i's sign, e.g. -1 + 2^-11 -- f16 is finer below a power of two, so h1 would carry j at a 2^-12 finer quantum next to
    the i terms and the exact sum of products would need up to 34 bits, more than an fp32 accumulator holds: no kernel could be torch.equal there.)"""
    import act_amd.kernels as K
    rng = np.random.default_rng(M + N + Kd)

    def lattice(r):
        i = rng.choice([-2, -1, 1, 2], (r, Kd)); j = np.sign(i) * rng.integers(0, 3, (r, Kd))
        z = rng.random((r, Kd)) < 0.05
        return np.where(z, 0, i), np.where(z, 0, j)
    ia, ja = lattice(M); ib, jb = lattice(N)
    a = (ia + ja * 2.0 ** -12).astype(np.float32); w = (ib + jb * 2.0 ** -12).astype(np.float32)
    s_a = R.act_scale(float(np.abs(a).max()))
    h1, h2 = R.split(a, s_a)                                   # the split is what the docstring says
    assert np.array_equal(h1.astype(np.float64), ia * s_a) and np.array_equal(h2.astype(np.float64), ja * s_a / 2)
    want = (ia @ ib.T) * 4096 + (ia @ jb.T + ja @ ib.T)        # int64, in units of 2^-12
    assert np.abs(want).max() < 2 ** 24
    at, wt = torch.from_numpy(a).to(dev), torch.from_numpy(w).to(dev)
    sb, sb_inv = K.f16x3_row_scales(wt)
    assert np.array_equal(sb.cpu().numpy(), R.row_scales(w))
    out = K.gemm_nt_f16x3(K.split_f16x2(at, s_a), s_a, K.split_f16x2(wt, 1.0, sb), sb_inv)
    assert torch.equal(out.cpu(), torch.from_numpy((want / 4096.0).astype(np.float32)))


def _ln_like(g, m, k):
    x = torch.randn(m, k, generator=g, dtype=torch.float64)
    x = (x - x.mean(1, keepdim=True)) / x.std(1, keepdim=True)
    return (x * (1 + 0.1 * torch.randn(k, generator=g, dtype=torch.float64)) + 0.1 * torch.randn(k, generator=g, dtype=torch.float64)).float()


def _families(g, M, N, Kd):
    w = (0.02 * torch.randn(N, Kd, generator=g)).float()
    ln = _ln_like(g, M, Kd)
    return [("layernorm", ln, w), ("acts*1e-2", ln * 1e-2, w), ("gelu", torch.nn.functional.gelu(torch.randn(M, Kd, generator=g)), w),
            ("acts<=3e4", ln * (3e4 / ln.abs().max()), w)]


def _x3(K, a, w, a_bound_factor=1.0, **kw):
    s_a = R.act_scale(a_bound_factor * a.abs().max().item())
    sb, sb_inv = K.f16x3_row_scales(w)
    return K.gemm_nt_f16x3(K.split_f16x2(a, s_a), s_a, K.split_f16x2(w, 1.0, sb), sb_inv, **kw)


@pytest.mark.parametrize("M,N,Kd", SHAPES + [(128, 256, 3072)])
def test_real_valued_gemm_is_as_close_to_float64_as_the_f32_kernel(dev, M, N, Kd):
    """measured on MI355X (relative L2 against the float64 product; split-f16 / f32 kernel): see notebook/teacher_f16x3.md"""
    import act_amd.kernels as K
    g = torch.Generator().manual_seed(M + N + Kd)
    for name, a, w in _families(g, M, N, Kd):
        a, w = a.to(dev), w.to(dev)
        ref = a.double() @ w.double().t()
        e32 = _rel_l2(K.gemm(a, w, True, True), ref)
        e16 = _rel_l2(_x3(K, a, w), ref)
        print(f"{M}x{N}x{Kd} {name:10s}: f32 kernel {e32:.3e}  split-f16 {e16:.3e}  ratio {e16 / e32:.2f}")
        assert e16 <= 1.5 * e32, (name, e16, e32)


@pytest.mark.parametrize("bias,act,res", [(True, 0, False), (True, 1, False), (True, 0, True), (False, 1, True)])
def test_epilogues_match_the_f32_kernels(dev, bias, act, res):
    import act_amd.kernels as K
    M, N, Kd = 256, 384, 192
    g = torch.Generator().manual_seed(11 + bias + 2 * act + 4 * res)
    a, w = _ln_like(g, M, Kd).to(dev), (0.05 * torch.randn(N, Kd, generator=g)).to(dev)
    b = torch.randn(N, generator=g).to(dev) if bias else None
    r = torch.randn(M, N, generator=g).to(dev) if res else None
    y = a.double() @ w.double().t()
    if b is not None:
        y = y + b.double()
    if act:
        y = torch.nn.functional.gelu(y)
    if r is not None:
        y = y + r.double()
    kw = dict(bias=b, act=(K.EPI_GELU if act else K.EPI_NONE), res=r)
    e32, e16 = _rel_l2(K.gemm(a, w, True, True, **kw), y), _rel_l2(_x3(K, a, w, **kw), y)
    print(f"epilogue bias={bias} gelu={act} res={res}: f32 kernel {e32:.3e}  split-f16 {e16:.3e}")
    assert e16 <= 1.5 * e32


def test_planes_out_feed_a_second_product(dev):
    """fc1 + GELU -> planes at the next product's scale -> fc2: the planes equal a split of the fp32 result bit for bit, and the chained product is as close
    to float64 as the f32 kernels' chain"""
    import act_amd.kernels as K
    M, D, Hd = 256, 128, 384
    g = torch.Generator().manual_seed(5)
    a, w1, b1 = _ln_like(g, M, D).to(dev), (0.05 * torch.randn(Hd, D, generator=g)).to(dev), torch.randn(Hd, generator=g).to(dev)
    w2, b2 = (0.05 * torch.randn(D, Hd, generator=g)).to(dev), torch.randn(D, generator=g).to(dev)
    s1 = R.act_scale(a.abs().max().item())
    bound2 = R.l1_bound(w1.cpu().numpy(), b1.cpu().numpy(), np.full(D, a.abs().max().item())).max()      # |gelu(x)| <= |x| <= the l1 bound
    s2 = R.act_scale(bound2)
    sb1, inv1 = K.f16x3_row_scales(w1); sb2, inv2 = K.f16x3_row_scales(w2)
    hid_planes = torch.empty(2, M, Hd, dtype=torch.float16, device=dev)
    hid = K.gemm_nt_f16x3(K.split_f16x2(a, s1), s1, K.split_f16x2(w1, 1.0, sb1), inv1, bias=b1, act=K.EPI_GELU, planes_out=hid_planes, out_scale=s2)
    assert torch.equal(hid_planes, K.split_f16x2(hid, s2))
    assert torch.equal(hid, K.gemm_nt_f16x3(K.split_f16x2(a, s1), s1, K.split_f16x2(w1, 1.0, sb1), inv1, bias=b1, act=K.EPI_GELU))
    out = K.gemm_nt_f16x3(hid_planes, s2, K.split_f16x2(w2, 1.0, sb2), inv2, bias=b2, res=a)
    ref = torch.nn.functional.gelu(a.double() @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double() + a.double()
    chain32 = K.gemm(K.gemm(a, w1, True, True, bias=b1, act=K.EPI_GELU), w2, True, True, bias=b2, res=a)
    e32, e16 = _rel_l2(chain32, ref), _rel_l2(out, ref)
    print(f"fc1-GELU-fc2 chain: f32 kernels {e32:.3e}  split-f16 {e16:.3e}")
    assert e16 <= 1.5 * e32


def test_producers_that_emit_f16_planes_equal_a_split_of_their_fp32_result(dev):
    import act_amd.kernels as K
    from act_amd import _C
    torch.manual_seed(3)
    x = torch.randn(260, 768, device=dev); pos = 0.1 * torch.randn(260, 768, device=dev)
    g = 1 + 0.1 * torch.randn(768, device=dev); b = 0.1 * torch.randn(768, device=dev)
    y, _, _, _ = K.layernorm_fwd(x, pos, g, b, 1e-6, want_stats=False)
    assert torch.equal(K.layernorm_f16_planes(x, g, b, 1e-6, 512.0, pos=pos), K.split_f16x2(y, 512.0))
    B, S0, Sq, H, hd = 2, 32, 64, 12, 64
    kv0 = torch.randn(B * S0, 2 * H * hd, device=dev); qkv = torch.randn(B * Sq, 3 * H * hd, device=dev)
    out = K.attention_fwd_prefix(kv0, S0, qkv, Sq, B, H, hd)
    planes = torch.empty(2, B * Sq, H * hd, dtype=torch.float16, device=dev)
    _C.check(_C.lib.act_attention_fwd_prefix_f16_planes_f32(_C.ptr(kv0), S0, _C.ptr(qkv), Sq, None, _C.ptr(planes[0]), _C.ptr(planes[1]), 4096.0, None, B, H,
                                                            hd, float(hd) ** -0.5, _C.stream()), "act_attention_fwd_prefix_f16_planes_f32")
    assert torch.equal(planes, K.split_f16x2(out, 4096.0))


# ---- whole teacher -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def teacher(dev):
    """full configs[1] geometry at B = 2 (TG = 128): the HIP model, the CPU oracle with the same weights, one batch and the oracle's recorded gumbel draws"""
    from oracle import models as OM, layers as OL
    from act_amd.models import build_model_from_cfg
    from act_amd.utils.config import cfg_from_yaml_file
    from tests.golden.fill import clouds
    cfg = cfg_from_yaml_file("cfgs/pretrain/pretrain_act_distill.yaml").model
    cfg.dvae_config.ckpt = "none"
    torch.manual_seed(2)
    oracle = OM.ACT_PointDistillation(OM.edict(cfg)).train()
    model = build_model_from_cfg(cfg)
    model.load_state_dict(oracle.state_dict(), strict=True)
    model.to(dev).train()
    oracle.dvae_tokenizer.prompt_p = 0.0; model.dvae_tokenizer.prompt_dropout.p = 0.0
    pts = torch.from_numpy(clouds(6, 2, 1024))
    with torch.no_grad():
        nb_o, c_o = oracle.group_divider(pts)
        rec = OL.Draws(record=True)
        tf_o = oracle.dvae_tokenizer.forward_tokenizer_features(nb_o, c_o, rec)
        nb, c = model.group_divider(pts.to(dev))
    return dict(model=model, oracle=oracle, nb=nb, c=c, gumbel=rec.table["gumbel"], tf_o=tf_o, OL=OL)


class _switch:
    """composite.TEACHER_F16X3 for the duration of a block (the split-bf16 opt-in off)"""
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        import act_amd.composite as CP
        self.saved = CP.TEACHER_F16X3, CP.TEACHER_BF16X3
        CP.TEACHER_F16X3, CP.TEACHER_BF16X3 = self.on, False

    def __exit__(self, *a):
        import act_amd.composite as CP
        CP.TEACHER_F16X3, CP.TEACHER_BF16X3 = self.saved


def _features(t, dev, on):
    from act_amd.utils.draws import Draws
    with torch.no_grad(), _switch(on):
        return t["model"].dvae_tokenizer.forward_tokenizer_features(t["nb"], t["c"], draws=Draws({"gumbel": t["gumbel"]}, device=dev))


def _embed(tokzr, x, c, on):
    with torch.no_grad(), _switch(on):
        return tokzr.visual_embedding(x, c)


def test_teacher_features_are_as_close_to_the_oracle_as_the_f32_path(dev, teacher):
    """measured on MI355X: see the figures in notebook/teacher_f16x3.md (max |e| / max |ref| against the CPU oracle)"""
    f32_a = _features(teacher, dev, False)
    x3_a = _features(teacher, dev, True)
    f32_b = _features(teacher, dev, False)
    x3_b = _features(teacher, dev, True)
    e32, e16 = _rel_max(f32_a, teacher["tf_o"]), _rel_max(x3_a, teacher["tf_o"])
    print(f"teacher features vs CPU oracle: f32 path {e32:.3e}  split-f16 default {e16:.3e}  (split-f16 vs f32 path {_rel_max(x3_a, f32_a):.3e})")
    assert torch.equal(f32_a, f32_b)                              # the f32 path is untouched by the switch having been used
    assert torch.equal(x3_a, x3_b)                                # deterministic
    assert not torch.equal(x3_a, f32_a)                           # the switch really took the other kernel
    assert e16 <= 2 * e32, (e16, e32)


def _vit_inputs(t, dev, mag):
    tk = t["model"].dvae_tokenizer
    g = torch.Generator().manual_seed(9)
    x = mag * torch.randn(2, t["c"].shape[1], tk.proj_pre.weight.shape[1], generator=g)
    return tk, x


def test_tokens_of_magnitude_1e6_give_finite_features_at_the_same_bar(dev, teacher):
    tk, x = _vit_inputs(teacher, dev, 1e6)
    with torch.no_grad():
        ref = teacher["oracle"].dvae_tokenizer.visual_embedding(x, teacher["c"].cpu(), teacher["OL"].Draws(record=True))
    f32, x3 = _embed(tk, x.to(dev), teacher["c"], False), _embed(tk, x.to(dev), teacher["c"], True)
    assert torch.isfinite(x3).all()
    e32, e16 = _rel_max(f32, ref), _rel_max(x3, ref)
    print(f"tokens ~1e6: vs CPU oracle f32 path {e32:.3e}  split-f16 default {e16:.3e}")
    assert e16 <= 2 * e32, (e16, e32)


def test_range_guard_keeps_an_out_of_range_linear_on_the_f32_kernel(dev, teacher, monkeypatch):
    """fc1 of block 0 scaled by 2^17: the bound on ITS OUTPUT -- fc2's operand -- passes 2^15, so fc2 of that block gets no scale and runs on the f32 kernel
    while every other Linear keeps the split-f16 kernel; the scales are the restatement's.  With every scale withheld the native split-f16 entry runs all
    products on the f32 kernels and equals the f32 path bit for bit (the per-product fallback is the f32 product itself)."""
    import act_amd.composite as CP
    tk, x = _vit_inputs(teacher, dev, 1.0)
    x, c = x.to(dev), teacher["c"]
    blk = tk.visual_embed[0][0]
    w = blk.mlp.fc1.weight
    with torch.no_grad():
        w.mul_(2.0 ** 17)
    try:
        out = _embed(tk, x, c, True)
        scales = CP._VIT_F16[tk][3]
        n = lambda t: None if t is None else t.detach().cpu().numpy()
        want = [R.act_scale(b) for b in R.block_bounds(n(blk.norm1.weight), n(blk.norm1.bias), n(blk.attn.qkv.weight), n(blk.attn.qkv.bias),
                                                       n(blk.norm2.weight), n(blk.norm2.bias), n(w), n(blk.mlp.fc1.bias))]
        assert list(scales[:4]) == want and want[3] == 0.0 and all(s > 0 for s in want[:3]) and all(s > 0 for s in scales[4:])
        f32 = _embed(tk, x, c, False)
        assert torch.isfinite(out).all() and not torch.equal(out, f32)
        assert _rel_max(out, f32) <= 1e-4
        monkeypatch.setattr(CP, "f16x3_act_scale", lambda b: 0.0)
        CP._VIT_F16.pop(tk, None)
        assert torch.equal(_embed(tk, x, c, True), f32)
    finally:
        with torch.no_grad():
            w.mul_(2.0 ** -17)
        CP._VIT_F16.pop(tk, None)


def test_plane_cache_follows_an_in_place_weight_change(dev, teacher):
    tk, x = _vit_inputs(teacher, dev, 1.0)
    x, c = x.to(dev), teacher["c"]
    before = _embed(tk, x, c, True)                               # fills the cache
    w = tk.visual_embed[0][3].attn.proj.weight
    with torch.no_grad():
        w.mul_(2.0)
    try:
        after = _embed(tk, x, c, True)
        fresh = copy.deepcopy(tk)                                 # a new module: nothing cached for it
        assert torch.equal(after, _embed(fresh, x, c, True))
        assert not torch.equal(after, before)
    finally:
        with torch.no_grad():
            w.mul_(0.5)
