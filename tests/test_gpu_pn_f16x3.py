"""The last product of the frozen tokenizer's mini-PointNet on split-f16 planes (act_sgemm_nt_f16x3_gmax_f32, act_pointnet_fwd_groups_f16x3_f32,
composite.pointnet_forward, ACT_TOKENIZER_PN_F16X3).  Kernel level: as close to a float64 restatement of max_group(relu(h sc + sh) W^T + b) as the f32 fused
kernel on the same inputs (within 1.5 x, the gate of tests/test_gpu_f16x3.py), the on-load form equals the pass form and the 128 x 192 tile the 128 x 128
tile bit for bit, lattice operands give exact integers.  Entry level: every case that must stay on the f32 product equals act_pointnet_fwd_groups_f32 bit for
bit.  Model level: the whole tokenizer sits as close to the CPU oracle as on the f32 path (within 2 x) with the same 128 codes, and the plane cache follows
in-place changes.

Kernel shapes are (R, C, K, n): rows, columns, depth, rows per group."""
import copy
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import f16x3_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (128, 128, 64, 32): one workgroup, two K tiles, four groups per tile; (384, 384, 128, 64): both tiles, the XCD remap with a remainder, one group per wave
# block; (1024, 384, 512, 32): the real K
SHAPES = [(128, 128, 64, 32), (384, 384, 128, 64), (1024, 384, 512, 32)]
CASES = [(s, "plain") for s in SHAPES] + [((384, 384, 128, 64), "bias-10"), ((128, 128, 64, 32), "dead-column"), ((1024, 384, 512, 32), "bias-10")]
A_SCALE = 32.0            # what the guard derives at the Stage-II row count: sqrt(262,144) max|gamma| + max|beta| in (512, 1024]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _f32_fused(h, sc, sh, w, bias, n):
    """the f32 fused kernel of the product path: affine + ReLU on load, group max as the epilogue, no store"""
    import act_amd.composite as CP
    import act_amd.kernels as K
    Rr, Kd = h.shape
    C = w.shape[0]
    out = torch.empty(Rr // n, C, dtype=torch.float32, device=h.device)
    epi = K.GemmEpilogue(); epi.alpha = 1.0; epi.bias = bias.data_ptr()
    fx = CP.GemmFx(); fx.a_scale = sc.data_ptr(); fx.a_shift = sh.data_ptr(); fx.gmax = out.data_ptr(); fx.group = n; fx.store_c = 0
    rc = CP.lib.act_sgemm_fx_f32(1, 1, Rr, C, Kd, h.data_ptr(), Kd, w.data_ptr(), Kd, None, C, ctypes.byref(epi), ctypes.byref(fx), None, 0,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return out


@functools.lru_cache(maxsize=None)
def _case(shape, variant="plain"):
    """inputs, the float64 reference and every form's output of one case: computed once, shared, never changed"""
    import act_amd.kernels as K
    Rr, C, Kd, n = shape
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(sum(shape) + len(variant))
    h = rng.standard_normal((Rr, Kd)).astype(np.float32)
    sc = (0.5 + rng.random(Kd)).astype(np.float32) * rng.choice([-1.0, 1.0], Kd).astype(np.float32)
    sh = (0.3 * rng.standard_normal(Kd)).astype(np.float32)
    w = (0.05 * rng.standard_normal((C, Kd))).astype(np.float32)
    bias = (0.1 * rng.standard_normal(C)).astype(np.float32)
    if variant == "bias-10":
        bias -= 10.0                                       # every output of many groups is negative: a max that started from 0 would show
    if variant == "dead-column":
        h[:, 5] = -np.abs(h[:, 5]) - 1.0; sc[5] = abs(sc[5]); sh[5] = 0.0        # the operand is exactly 0 down a whole column
    a64 = np.maximum(h.astype(np.float64) * sc.astype(np.float64) + sh.astype(np.float64), 0.0)
    if variant == "dead-column":
        assert not a64[:, 5].any()
    ref = (a64 @ w.astype(np.float64).T + bias.astype(np.float64)).reshape(Rr // n, n, C).max(axis=1)
    if variant == "bias-10":
        assert (ref.max(axis=1) < 0).sum() > 0
    assert float(a64.max()) * A_SCALE <= 32768.0
    t = lambda x: torch.from_numpy(x).to(dev)
    hd, scd, shd, wd, bd = t(h), t(sc), t(sh), t(w), t(bias)
    sb, sb_inv = K.f16x3_row_scales(wd)
    wp = K.split_f16x2(wd, 1.0, sb)
    ap = K.split_f16x2_affine_relu(hd, scd, shd, A_SCALE)
    tiles = (128, 192) if C % 192 == 0 else (128,)
    load = {tl: K.gemm_nt_f16x3_gmax(hd, A_SCALE, wp, sb_inv, n, bias=bd, col_scale=scd, col_shift=shd, tile=tl) for tl in (0,) + tiles}
    split = {tl: K.gemm_nt_f16x3_gmax(ap, A_SCALE, wp, sb_inv, n, bias=bd, tile=tl) for tl in tiles}
    f32 = _f32_fused(hd, scd, shd, wd, bd, n)
    torch.cuda.synchronize()
    return dict(ref=ref, f32=f32, load=load, split=split, h=h, sc=sc, sh=sh, planes=ap)


def _rel_l2(x, ref):
    ref = torch.from_numpy(ref) if isinstance(ref, np.ndarray) else ref.double().cpu()
    return ((x.double().cpu() - ref).norm() / ref.norm()).item()


# ---- 1. accuracy -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,variant", CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}n{s[3]}-{v}" for s, v in CASES])
def test_the_split_product_is_as_close_to_float64_as_the_f32_fused_kernel(dev, shape, variant):
    """measured on MI355X: see notebook/pn_f16x3.md"""
    c = _case(shape, variant)
    e32, e16 = _rel_l2(c["f32"], c["ref"]), _rel_l2(c["load"][0], c["ref"])
    print(f"{shape} {variant}: relative L2 against float64: f32 fused {e32:.3e}  split-f16 on load {e16:.3e}  ratio {e16 / e32:.2f}")
    assert torch.isfinite(c["load"][0]).all()
    assert e16 <= 1.5 * e32, (e16, e32)


# ---- 2. exactness ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,variant", CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}n{s[3]}-{v}" for s, v in CASES])
def test_on_load_equals_the_pass_form_and_both_tiles_give_the_same_bits(dev, shape, variant):
    c = _case(shape, variant)
    # the pass writes the planes of the numpy restatement: one fp32 fma with the scale folded in, ReLU, split
    a = np.maximum((c["h"].astype(np.float64) * (c["sc"] * np.float32(A_SCALE)).astype(np.float64) + (c["sh"] * np.float32(A_SCALE)).astype(np.float64))
                   .astype(np.float32), 0)
    h1, h2 = R.split(a, 1.0)
    assert np.array_equal(c["planes"][0].cpu().numpy().view(np.uint16), h1.view(np.uint16))
    assert np.array_equal(c["planes"][1].cpu().numpy().view(np.uint16), h2.view(np.uint16))
    first = c["load"][128]
    for tl, out in list(c["load"].items()) + list(c["split"].items()):
        assert torch.equal(out, first), tl
    assert (192 in c["load"]) == (shape[1] % 192 == 0)


@pytest.mark.parametrize("shape", SHAPES)
def test_lattice_operands_give_exact_integers(dev, shape):
    """the lattice of tests/test_gpu_f16x3.py (i + j 2^-12, j of i's sign or zero) through the identity affine map: ReLU turns the negative elements into exact
    zeros, the rest is exact in both accumulators, and the group max of exact values is exact"""
    import act_amd.kernels as K
    Rr, C, Kd, n = shape
    rng = np.random.default_rng(sum(shape))

    def lattice(r):
        i = rng.choice([-2, -1, 1, 2], (r, Kd)); j = np.sign(i) * rng.integers(0, 3, (r, Kd))
        z = rng.random((r, Kd)) < 0.05
        return np.where(z, 0, i), np.where(z, 0, j)
    ia, ja = lattice(Rr); ib, jb = lattice(C)
    a = (ia + ja * 2.0 ** -12).astype(np.float32); w = (ib + jb * 2.0 ** -12).astype(np.float32)
    ia, ja = np.where(ia > 0, ia, 0), np.where(ia > 0, ja, 0)                   # after ReLU
    want = ((ia @ ib.T) * 4096 + (ia @ jb.T + ja @ ib.T)).reshape(Rr // n, n, C).max(axis=1)        # int64, in units of 2^-12
    assert np.abs(want).max() < 2 ** 24
    s_a = R.act_scale(float(np.abs(a).max()))
    at, wt = torch.from_numpy(a).to(dev), torch.from_numpy(w).to(dev)
    sb, sb_inv = K.f16x3_row_scales(wt)
    one, zero = torch.ones(Kd, device=dev), torch.zeros(Kd, device=dev)
    out = K.gemm_nt_f16x3_gmax(at, s_a, K.split_f16x2(wt, 1.0, sb), sb_inv, n, col_scale=one, col_shift=zero)
    assert torch.equal(out.cpu(), torch.from_numpy((want / 4096.0).astype(np.float32)))


def test_arguments_the_kernel_does_not_take_are_refused(dev):
    import act_amd.kernels as K
    from act_amd import _C
    c = _case(SHAPES[0])
    hd = torch.from_numpy(c["h"]).to(dev)
    wp = torch.zeros(2, 128, 64, dtype=torch.float16, device=dev)
    inv, v = torch.ones(128, device=dev), torch.ones(64, device=dev)
    for kw in (dict(group=16), dict(group=32, tile=192), dict(group=32, tile=64)):         # a group no wave block holds; a tile the shape / the kernel does not take
        with pytest.raises(_C.ActHipError):
            K.gemm_nt_f16x3_gmax(hd, A_SCALE, wp, inv, kw.pop("group"), col_scale=v, col_shift=v, **kw)


# ---- 3. the native entry: fallbacks ------------------------------------------------------------------------------------------------------------------------
def _encoder(C, seed):
    """a frozen Encoder on the CPU in training mode: torch's default initialisation under ``seed``, both BatchNorm affines moved off (1, 0)"""
    from act_amd.models.dvae import Encoder
    torch.manual_seed(seed)
    enc = Encoder(C)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for bn in (enc.first_conv[1], enc.second_conv[1]):
            bn.weight.add_(0.1 * torch.randn(bn.weight.shape, generator=g))
            bn.bias.add_(0.1 * torch.randn(bn.bias.shape, generator=g))
    for p in enc.parameters():
        p.requires_grad = False
    return enc.train()


def _native(enc, pts, x3=False, edit=None, keep=0, groups=None):
    """one call of the native entry on the device module: act_pointnet_fwd_groups_f32, or (x3) act_pointnet_fwd_groups_f16x3_f32 with the struct the host path
    builds, after ``edit(x3)`` changed it.  pts [BG, n, 3]"""
    import act_amd.composite as CP
    from act_amd import _C
    lib, _p = _C.lib, CP._p
    BG, n, _ = pts.shape
    dims, (c1, bn1, c2, c3, bn2, c4) = CP._pointnet_structs(enc, BG, n)
    w2 = lambda c: c.weight.view(c.weight.shape[0], c.weight.shape[1])
    bufs = [t.clone() for t in (bn1.running_mean, bn1.running_var, bn2.running_mean, bn2.running_var)]          # the module's own stay as they are
    prm = CP.PointnetParams(*[_p(t) for t in (w2(c1), c1.bias, bn1.weight, bn1.bias, w2(c2), c2.bias, w2(c3), c3.bias, bn2.weight, bn2.bias, w2(c4), c4.bias)
                              + tuple(bufs)])
    saved = torch.empty(int(lib.act_pointnet_saved_floats(ctypes.byref(dims))), dtype=torch.float32, device=pts.device)
    out = torch.empty(BG, dims.C, dtype=torch.float32, device=pts.device)
    ws = CP.K.workspace(pts.device)
    x = pts.reshape(BG * n, 3).contiguous()
    ng = 0 if groups is None else int(groups.numel())
    args = (ctypes.byref(dims), ctypes.byref(prm), _p(x), 1, int(keep), _p(saved), _p(out), _p(groups) if ng else None, ng, _p(ws), ws.numel() * 4)
    CP.ensure_tuned(("pn_fwd", dims.BG, dims.n, dims.C, ng), lambda: lib.act_pointnet_fwd_groups_f32(*args, _C.stream()), pts.device)
    if not x3:
        _C.check(lib.act_pointnet_fwd_groups_f32(*args, _C.stream()), "act_pointnet_fwd_groups_f32")
    else:
        s, alive = CP._pointnet_f16_planes(enc, BG * n)
        if edit is not None:
            edit(s)
        _C.check(lib.act_pointnet_fwd_groups_f16x3_f32(args[0], args[1], ctypes.byref(s), *args[2:], _C.stream()), "act_pointnet_fwd_groups_f16x3_f32")
        torch.cuda.synchronize()
        del alive
    return out


@functools.lru_cache(maxsize=None)
def _pn(C, BG, n, seed=0):
    dev = torch.device("cuda:0")
    enc = _encoder(C, 100 + seed).to(dev)
    pts = torch.from_numpy(np.random.default_rng(200 + seed).standard_normal((BG, n, 3)).astype(np.float32)).to(dev)
    return dict(enc=enc, pts=pts, f32=_native(enc, pts), x3=_native(enc, pts, x3=True))


def _zero_scale(s):
    s.a_scale = 0.0


def _null_planes(s):
    s.c4_planes = None


def _null_inv(s):
    s.c4_inv_scale = None


def test_the_entry_takes_the_split_product_and_keeps_the_gate(dev):
    """(BG, n) = (8, 32): R = 256, two workgroup rows.  The float64 reference here is the f32 entry's own h3 and affine map put through float64 -- everything
    in front of the last product is shared bit for bit, so the two entries differ by that product alone"""
    c = _pn(384, 8, 32)
    assert not torch.equal(c["x3"], c["f32"])
    assert torch.equal(c["x3"], _native(c["enc"], c["pts"], x3=True))
    rel = ((c["x3"].double() - c["f32"].double()).norm() / c["f32"].double().norm()).item()
    print(f"entry, split product against f32 product: relative L2 {rel:.3e}")
    assert rel < 1e-5


@pytest.mark.parametrize("C,BG,n,edit,kw", [(200, 8, 32, None, {}), (384, 3, 32, None, {}), (384, 8, 32, _zero_scale, {}), (384, 8, 32, _null_planes, {}),
                                            (384, 8, 32, _null_inv, {}), (384, 8, 32, None, dict(keep=1)), (384, 8, 32, None, dict(groups=(0, 3, 5, 6)))],
                         ids=["C=200", "R=96", "a_scale=0", "null-planes", "null-inv-scale", "keep_for_backward=1", "groups"])
def test_a_call_that_must_stay_on_the_f32_product_equals_the_f32_entry_bit_for_bit(dev, C, BG, n, edit, kw):
    c = _pn(C, BG, n)
    if "groups" in kw:
        kw = dict(groups=torch.tensor(kw["groups"], dtype=torch.int32, device=dev))
    want = _native(c["enc"], c["pts"], **kw) if kw else c["f32"]
    got = _native(c["enc"], c["pts"], x3=True, edit=edit, **kw)
    assert torch.equal(got, want)
    if C == 384 and BG == 8:
        assert not torch.equal(_pn(384, 8, 32)["x3"], _pn(384, 8, 32)["f32"])           # ... where the plain call does take the other kernel


def _host(enc, pts):
    with torch.no_grad():
        return enc(pts.unsqueeze(0)).squeeze(0)


def test_the_host_path_takes_it_only_frozen_under_no_grad_with_batch_statistics(dev):
    c = _pn(384, 8, 32)
    enc = copy.deepcopy(c["enc"])
    assert torch.equal(_host(enc, c["pts"]), c["x3"])
    assert torch.equal(enc(c["pts"].unsqueeze(0)).squeeze(0), c["f32"])                    # grad enabled
    enc.second_conv[3].bias.requires_grad = True
    assert torch.equal(_host(enc, c["pts"]), c["f32"])                                     # a trainable parameter
    enc.second_conv[3].bias.requires_grad = False
    with torch.no_grad():
        enc.second_conv[1].weight.mul_(4096.0)                                             # sqrt(256) * 4096 * max|gamma| > 2^15: no scale
    import act_amd.composite as CP
    out = _host(enc, c["pts"])
    assert CP._PN_F16[enc][5][256] == 0.0 and torch.equal(out, _native(enc, c["pts"]))
    ev = copy.deepcopy(c["enc"]).eval()                                                    # running statistics: no bound, the f32 product
    a = _host(ev, c["pts"])
    assert ev not in CP._PN_F16 and torch.isfinite(a).all()


def _child():
    """run by test_the_switch_at_0_restores_the_f32_path in a fresh interpreter with ACT_TOKENIZER_PN_F16X3=0"""
    import act_amd.composite as CP
    assert CP.TOKENIZER_PN_F16X3 is False
    c = _pn(384, 8, 32)
    assert torch.equal(_host(c["enc"], c["pts"]), c["f32"]) and not torch.equal(c["x3"], c["f32"])
    print("child-ok")


def test_the_switch_at_0_restores_the_f32_path(dev):
    env = dict(os.environ, ACT_TOKENIZER_PN_F16X3="0")
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_pn_f16x3 as T; T._child()"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "child-ok" in r.stdout, r.stdout + r.stderr


# ---- 4. the cache ------------------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_equal_and_the_cache_follows_in_place_changes(dev):
    c = _pn(384, 8, 32)
    enc = copy.deepcopy(c["enc"])
    a, b = _host(enc, c["pts"]), _host(enc, c["pts"])
    assert torch.equal(a, b) and torch.equal(a, c["x3"])
    with torch.no_grad():
        enc.second_conv[3].weight.mul_(1.5)               # (not a power of two: the planes themselves change)
        enc.second_conv[1].weight[7].mul_(40.0)           # one gamma of bn2: max|gamma| now gives another scale
    after = _host(enc, c["pts"])
    fresh = copy.deepcopy(enc)                            # a new module: nothing cached for it
    assert torch.equal(after, _host(fresh, c["pts"]))
    assert not torch.equal(after, a)


# ---- 5. whole tokenizer ------------------------------------------------------------------------------------------------------------------------------------
class _switch:
    """composite.TOKENIZER_PN_F16X3 for the duration of a block"""
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        import act_amd.composite as CP
        self.saved, CP.TOKENIZER_PN_F16X3 = CP.TOKENIZER_PN_F16X3, self.on

    def __exit__(self, *a):
        import act_amd.composite as CP
        CP.TOKENIZER_PN_F16X3 = self.saved


def test_tokenizer_features_and_codes_are_those_of_the_f32_path(dev):
    """full Stage-II tokenizer geometry at B = 2 with the oracle's gumbel draws replayed: features within 2 x the f32 path's distance to the CPU oracle (the
    rule of the teacher's ViT change) and all 128 codes equal.  Seed 2 / clouds 6: the oracle's own top-two margin of (logit + gumbel) over the 128 tokens is
    6.46e-3 at its smallest, in float32 and in float64 alike (they differ by 9e-7), against logits of magnitude 6.6 -- no code is at the mercy of rounding."""
    import act_amd.kernels as K
    from oracle import models as OM, layers as OL
    from act_amd.models import build_model_from_cfg
    from act_amd.models.dvae import DGCNN
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
    oracle.dvae_tokenizer.prompt_p = 0.0; model.dvae_tokenizer.prompt_dropout.p = 0.0
    pts = torch.from_numpy(clouds(6, 2, 1024))
    with torch.no_grad():
        nb_o, c_o = oracle.group_divider(pts)
        rec = OL.Draws(record=True)
        tf_o = oracle.dvae_tokenizer.forward_tokenizer_features(nb_o, c_o, rec)
        nb, c = model.group_divider(pts.to(dev))
    tok = model.dvae_tokenizer
    gumbel = rec.table["gumbel"]

    def run(on):
        with torch.no_grad(), _switch(on):
            return tok.forward_tokenizer_features(nb, c, draws=Draws({"gumbel": gumbel}, device=dev))

    def codes(on):
        with torch.no_grad(), _switch(on):
            B, G, _ = c.shape
            h = tok.dgcnn_1.features(tok.encoder(nb), c, DGCNN.graph_index(c))
            noise = Draws({"gumbel": gumbel}, device=dev).get("gumbel", None)
            return K.gn_gumbel_argmax_gather(h, B, G, tok.dgcnn_1.layer5[1], tok.codebook, noise=noise)[1].reshape(-1).cpu()

    def tokens(on):
        with torch.no_grad(), _switch(on):
            return tok.encoder(nb)

    assert not torch.equal(tokens(True), tokens(False))   # the frozen tokenizer's encoder really takes the other kernel
    rel_max = lambda a: ((a.double().cpu() - tf_o.double()).abs().max() / tf_o.double().abs().max()).item()
    f32, x3 = run(False), run(True)
    e32, e16 = rel_max(f32), rel_max(x3)
    i32, i16 = codes(False), codes(True)
    print(f"tokenizer features vs CPU oracle: f32 last product {e32:.3e}  split-f16 last product (default) {e16:.3e}; codes that differ: {int((i32 != i16).sum())} of {i32.numel()}")
    assert torch.equal(f32, run(False)) and torch.equal(x3, run(True))
    assert i32.numel() == 128 and torch.equal(i32, i16)
    assert e16 <= 2 * e32, (e16, e32)
