"""The stacked edge-conv products of the frozen tokenizer's DGCNNs (layers 2-4) on the split-f16 kernel (act_dgcnn_features_f16x3_f32 with `layers`,
ACT_TOKENIZER_DGCNN_F16X3):

 1. the strided entries under them -- A planes read as a column slice of a wider buffer, the split pass writing such a slice -- give the bits of the dense ones,
    and refuse a bad stride or a misaligned slice without launching;
 2. the whole DGCNN is as close to a float64 restatement (torch ops, below) as the f32 entry, within the project's 1.5 x, with the head on planes and on f32;
 3. every unusable struct equals act_dgcnn_features_f32 bit for bit; the switch at 0 gives the parent's path;
 4. two runs are equal and the plane cache follows in-place changes of a layer weight and a GroupNorm gamma;
 5. the whole tokenizer at B = 2 sits within 2 x of the switch-off path's distance to the CPU oracle (the rule of notebook/teacher_f16x3.md).

(tests/test_gpu_dgcnn_f16x3.py keeps checking the head alone; its helpers are reused here.)
The host path takes the layers from composite.DGCNN_F16X3_MIN_T rows on; the tests lower it to reach the path at T = 128 and 384, the smallest the kernel takes."""
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
from tests import test_gpu_dgcnn_f16x3 as DG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BADARG = -1
SHAPES = [(2, 64, 4, 384, 8192), (6, 64, 4, 384, 8192), (2, 64, 4, 384, 384), (6, 64, 4, 384, 384)]      # T = 128 | 384 (a tile-count remainder); head on planes | f32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _set:
    """attributes of act_amd.composite for the duration of a block"""
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        import act_amd.composite as CP
        self.saved = {k: getattr(CP, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(CP, k, v)

    def __exit__(self, *a):
        import act_amd.composite as CP
        for k, v in self.saved.items():
            setattr(CP, k, v)


# ---- 1. strided entries ------------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from act_amd import _C
    import act_amd.composite as CP
    return _C.lib, CP._p, _C.stream


def _ptr(t, elem_off=0):
    return ctypes.c_void_p(t.data_ptr() + elem_off * t.element_size())


def _product_lda(M, N, Kd, wide, lda, off, a_scale, bp, binv, tile, out):
    lib, _p, stream = _lib()
    return lib.act_sgemm_nt_f16x3_planes_lda_f32(M, N, Kd, _ptr(wide[0], off), _ptr(wide[1], off), lda, float(a_scale), _p(bp[0]), _p(bp[1]), _p(binv), _p(out), N,
                                                 None, None, 0.0, None, stream(), tile)


@pytest.mark.parametrize("M,N,Kd,lda,off,tiles", [(128, 128, 64, 192, 64, (128,)), (384, 384, 128, 320, 128, (128, 192))],
                         ids=["one-workgroup-two-K-tiles", "xcd-remainder-both-tiles"])
def test_the_strided_entries_give_the_bits_of_the_dense_ones(dev, M, N, Kd, lda, off, tiles):
    import act_amd.kernels as K
    lib, _p, stream = _lib()
    rng = np.random.default_rng(M + Kd)
    a = rng.standard_normal((M, Kd)).astype(np.float32)
    a[0, 0], a[1, 1] = 0.0, 1e-7                                         # a zero and a value whose planes flush
    w = (rng.standard_normal((N, Kd)) / 8).astype(np.float32)
    a_scale = 64.0
    ad, wd = torch.from_numpy(a).to(dev), torch.from_numpy(w).to(dev)
    # the split pass into a column slice of [2, M, lda]; the source is itself a slice of a wider fp32 buffer
    src = torch.full((M, lda), 7.0, device=dev)
    src[:, off:off + Kd] = ad
    wide = torch.full((2, M, lda), -3.0, dtype=torch.float16, device=dev)
    rc = lib.act_split_f16x2_ld_f32(_ptr(src, off), M, Kd, lda, a_scale, _ptr(wide[0], off), _ptr(wide[1], off), lda, stream())
    assert rc == 0
    dense = K.split_f16x2(ad, a_scale)
    assert torch.equal(wide[:, :, off:off + Kd], dense)
    keep = torch.ones(lda, dtype=torch.bool, device=dev)
    keep[off:off + Kd] = False
    assert bool((wide[:, :, keep] == -3.0).all())                         # nothing outside the slice is written
    h1, h2 = R.split(a, a_scale)
    assert np.array_equal(dense[0].cpu().numpy().view(np.uint16), h1.view(np.uint16)) and np.array_equal(dense[1].cpu().numpy().view(np.uint16), h2.view(np.uint16))
    # the product reading that slice
    scale, inv = K.f16x3_row_scales(wd)
    bp = K.split_f16x2(wd, 1.0, scale)
    for tile in tiles:
        ref = K.gemm_nt_f16x3(dense, a_scale, bp, inv, tile=tile)
        out = torch.empty(M, N, device=dev)
        assert _product_lda(M, N, Kd, wide, lda, off, a_scale, bp, inv, tile, out) == 0
        assert torch.equal(out, ref)
        out2 = torch.empty(M, N, device=dev)                              # lda == K on the compacted copy: the dense entry
        assert _product_lda(M, N, Kd, dense, Kd, 0, a_scale, bp, inv, tile, out2) == 0 and torch.equal(out2, ref)
    want = (a.astype(np.float64) @ w.astype(np.float64).T)
    assert np.abs(ref.cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()


def test_bad_strides_and_a_misaligned_slice_are_refused_and_launch_nothing(dev):
    import act_amd.kernels as K
    lib, _p, stream = _lib()
    M, N, Kd, lda = 128, 128, 64, 192
    wide = torch.zeros(2, M, lda, dtype=torch.float16, device=dev)
    wd = torch.randn(N, Kd, device=dev)
    scale, inv = K.f16x3_row_scales(wd)
    bp = K.split_f16x2(wd, 1.0, scale)
    out = torch.full((M, N), 5.0, device=dev)
    for ld, off in ((Kd - 8, 0), (lda + 4, 64), (lda, 4), (0, 0)):        # lda < K; lda % 8 != 0; a slice 8 bytes off the 16-byte grid; no stride
        assert _product_lda(M, N, Kd, wide, ld, off, 64.0, bp, inv, 0, out) == E_BADARG
    src = torch.ones(M, Kd, device=dev)
    planes = torch.full((2, M, lda), -3.0, dtype=torch.float16, device=dev)
    for ldp, off in ((Kd - 8, 0), (lda + 4, 64), (lda, 4)):
        assert lib.act_split_f16x2_ld_f32(_p(src), M, Kd, Kd, 64.0, _ptr(planes[0], off), _ptr(planes[1], off), ldp, stream()) == E_BADARG
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((planes == -3.0).all())


# ---- 2. the whole DGCNN against float64 --------------------------------------------------------------------------------------------------------------------
def _ref64(dg, f, idx):
    """float64 restatement of DGCNN.features from torch ops on the CPU: stacked products, gather, GroupNorm (biased variance over (C / groups, G, k) per
    cloud), LeakyReLU(0.2), max over k, concatenation, head.  -> h [B*G, Cout]"""
    B, G, Cin = f.shape
    d = lambda t: t.detach().cpu().double()
    x = d(f).reshape(B * G, Cin) @ d(dg.input_trans.weight)[:, :, 0].T + d(dg.input_trans.bias)
    ar = torch.arange(B)[:, None, None]
    outs = []
    for layer in DG._layers(dg):
        conv, gn = layer[0], layer[1]
        w = d(conv.weight)[:, :, 0, 0]
        cout, cin = w.shape[0], w.shape[1] // 2
        wa, wb = w[:, :cin], w[:, cin:]
        y, z = (x @ wa.T).reshape(B, G, cout), (x @ (wb - wa).T).reshape(B, G, cout)
        pre = y[ar, idx.cpu()] + z[:, None]                                # [B, k, G, cout]: Y of the neighbour + Z of the point
        pg = pre.reshape(B, -1, gn.num_groups, cout // gn.num_groups)      # [B, k G, groups, C / groups]
        mean = pg.mean(dim=(1, 3), keepdim=True)
        var = ((pg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
        yh = ((pg - mean) / torch.sqrt(var + gn.eps)).reshape(pre.shape) * d(gn.weight) + d(gn.bias)
        x = torch.where(yh >= 0, yh, 0.2 * yh).amax(dim=1).reshape(B * G, cout)
        outs.append(x)
    return torch.cat(outs, dim=1) @ d(dg.layer5[0].weight)[:, :, 0].T


def _native(dg, f, idx, mode, edit=None):
    """one call of the native entry on the device module: mode 'f32' = act_dgcnn_features_f32; 'layers' = the split entry with the layer planes (and the head's
    from 1024 columns on, as the host path builds it); 'head' = the head planes alone (the parent's struct).  ``edit(x3, T)`` changes the struct first."""
    import act_amd.composite as CP
    from act_amd import _C
    lib, _p = _C.lib, CP._p
    B, G, Cin = f.shape
    w5 = dg.layer5[0].weight
    with torch.no_grad():
        stacked = [dg._stacked_weight(layer[0]) for layer in DG._layers(dg)]
    m = CP.Dgcnn()
    gn0 = dg.layer1[1]
    m.B, m.G, m.k, m.Cin, m.Cout, m.groups = B, G, idx.shape[1], Cin, w5.shape[0], gn0.num_groups
    m.eps, m.slope = float(gn0.eps), 0.2
    m.w_in, m.b_in, m.w5 = _p(dg.input_trans.weight), _p(dg.input_trans.bias), _p(w5)
    for l, layer in enumerate(DG._layers(dg)):
        m.stacked[l], m.gn_w[l], m.gn_b[l] = _p(stacked[l]), _p(layer[1].weight), _p(layer[1].bias)
    scratch = torch.empty(int(lib.act_dgcnn_scratch_floats(ctypes.byref(m))), dtype=torch.float32, device=f.device)
    h = torch.empty(B * G, m.Cout, dtype=torch.float32, device=f.device)
    ws = CP.K.workspace(f.device)
    args = (ctypes.byref(m), _p(f), _p(idx), _p(h), _p(scratch), _p(ws), ws.numel() * 4)
    CP.ensure_tuned(("dgcnn", B, G, Cin, m.Cout), lambda: lib.act_dgcnn_features_f32(*args, _C.stream()), f.device)
    if mode == "f32":
        _C.check(lib.act_dgcnn_features_f32(*args, _C.stream()), "act_dgcnn_features_f32")
        return h
    s, keep = CP._dgcnn_f16_planes(dg, B * G, G, m.k, f.device, head=m.Cout >= 1024, layers=(mode == "layers"))
    if edit is not None:
        edit(s, B * G)
    _C.check(lib.act_dgcnn_features_f16x3_f32(args[0], ctypes.byref(s), *args[1:], _C.stream()), "act_dgcnn_features_f16x3_f32")
    torch.cuda.synchronize()
    del keep
    return h


@functools.lru_cache(maxsize=None)
def _case(shape, seed=0):
    """module (CPU + device copy), inputs, the float64 reference and the entries' outputs of one shape: computed once, shared, never changed"""
    B, G, k, Cin, Cout = shape
    dev = torch.device("cuda:0")
    cpu = DG._module(Cin, Cout, 500 + seed)
    f, idx = DG._inputs(B, G, Cin, 600 + seed)
    dg = copy.deepcopy(cpu).to(dev)
    fd, idxd = f.to(dev), idx.to(dev)
    return dict(cpu=cpu, dg=dg, f=fd, idx=idxd, h64=_ref64(cpu, f, idx), h32=_native(dg, fd, idxd, "f32"), head=_native(dg, fd, idxd, "head") if Cout >= 1024 else None,
                x3=_native(dg, fd, idxd, "layers"))


@pytest.mark.parametrize("shape", SHAPES)
def test_the_split_layers_are_as_close_to_float64_as_the_f32_entry(dev, shape):
    """measured on MI355X: see notebook/dgcnn_f16x3.md"""
    c = _case(shape)
    e32, e16 = DG._rel_l2(c["h32"], c["h64"]), DG._rel_l2(c["x3"], c["h64"])
    print(f"{shape}: relative L2 of h against float64: f32 entry {e32:.3e}  split-f16 layers{' + head' if shape[4] >= 1024 else ''} {e16:.3e}  ratio {e16 / e32:.2f}")
    assert not torch.equal(c["x3"], c["h32"])                             # the entry really took the other kernel ...
    if c["head"] is not None:
        assert not torch.equal(c["x3"], c["head"])                        # ... for the layers, not only for the head
    assert e16 <= 1.5 * e32, (e16, e32)


# ---- 3. fall-backs -----------------------------------------------------------------------------------------------------------------------------------------
def _zero_scale(s, T):
    s.a_scale = 0.0


def _null_layer_plane(s, T):
    s.st_planes[1] = None


def _null_layer_inv(s, T):
    s.st_inv_scale[2] = None


def _null_scratch(s, T):
    s.a_planes = None


def _one_short(s, T):
    s.a_planes_elems = 2 * T * 2304 - 1


@pytest.mark.parametrize("shape,edit", [((1, 64, 4, 384, 384), None), ((2, 64, 4, 384, 384), _zero_scale), ((2, 64, 4, 384, 8192), _zero_scale),
                                        ((2, 64, 4, 384, 384), _null_layer_plane), ((2, 64, 4, 384, 8192), _null_layer_inv),
                                        ((2, 64, 4, 384, 384), _null_scratch), ((2, 64, 4, 384, 8192), _one_short)],
                         ids=["T=64", "a_scale=0", "a_scale=0-head", "null-layer-plane", "null-layer-inv-scale-head", "null-a-planes", "one-element-short-head"])
def test_an_unusable_struct_equals_the_f32_entry_bit_for_bit(dev, shape, edit):
    c = _case(shape)
    if edit is None:
        assert torch.equal(c["x3"], c["h32"])                             # a row count the kernel does not take
    else:
        assert not torch.equal(c["x3"], c["h32"])
        assert torch.equal(_native(c["dg"], c["f"], c["idx"], "layers", edit=edit), c["h32"])


def test_without_head_planes_only_the_head_stays_on_the_f32_kernel(dev):
    """Cout = 8192 with the head's planes taken out of the struct: not the f32 entry (the layers run split), not the full split path (the head does not)"""
    c = _case((2, 64, 4, 384, 8192))

    def no_head(s, T):
        s.w5_planes = None
    out = _native(c["dg"], c["f"], c["idx"], "layers", edit=no_head)
    assert not torch.equal(out, c["h32"]) and not torch.equal(out, c["x3"])
    assert DG._rel_l2(out, c["h64"]) <= 1.5 * DG._rel_l2(c["h32"], c["h64"])


def _child():
    """run by test_the_switch_at_0_restores_the_parent_path in a fresh interpreter with ACT_TOKENIZER_DGCNN_F16X3=0"""
    import act_amd.composite as CP
    assert CP.TOKENIZER_DGCNN_F16X3 is False
    with _set(DGCNN_F16X3_MIN_T=128):
        c = _case((2, 64, 4, 384, 384))
        assert torch.equal(DG._host(c["dg"], c["f"], c["idx"]), c["h32"]) and not torch.equal(c["x3"], c["h32"])      # dgcnn_2's width: the f32 entry
        c = _case((2, 64, 4, 384, 8192))
        assert torch.equal(DG._host(c["dg"], c["f"], c["idx"]), c["head"]) and not torch.equal(c["x3"], c["head"])    # dgcnn_1's: the head alone, as before
    print("child-ok")


def test_the_switch_at_0_restores_the_parent_path(dev):
    env = dict(os.environ, ACT_TOKENIZER_DGCNN_F16X3="0")
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_dgcnn_edge_f16x3 as T; T._child()"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "child-ok" in r.stdout, r.stdout + r.stderr


# ---- 4. the host path: threshold, determinism, the cache ---------------------------------------------------------------------------------------------------
def test_the_host_path_takes_the_layers_from_the_row_threshold_on(dev):
    import act_amd.composite as CP
    assert CP.DGCNN_F16X3_MIN_T == 4096                                   # one round of 128 x 128 workgroups on 256 CUs at the 1024-column product
    for shape in ((2, 64, 4, 384, 384), (2, 64, 4, 384, 8192)):
        c = _case(shape)
        assert torch.equal(DG._host(c["dg"], c["f"], c["idx"]), c["h32"] if c["head"] is None else c["head"])         # T = 128: below it
        with _set(DGCNN_F16X3_MIN_T=128):
            assert torch.equal(DG._host(c["dg"], c["f"], c["idx"]), c["x3"])


def test_two_runs_are_equal_and_the_cache_follows_in_place_changes(dev):
    for shape in ((2, 64, 4, 384, 384), (2, 64, 4, 384, 8192)):
        c = _case(shape)
        dg = copy.deepcopy(c["dg"])
        with _set(DGCNN_F16X3_MIN_T=128):
            a, b = DG._host(dg, c["f"], c["idx"]), DG._host(dg, c["f"], c["idx"])
            assert torch.equal(a, b) and torch.equal(a, c["x3"])
            with torch.no_grad():
                dg.layer3[0].weight.mul_(1.5)                             # (not a power of two: the planes of the stacked matrix change)
            mid = DG._host(dg, c["f"], c["idx"])
            assert torch.equal(mid, DG._host(copy.deepcopy(dg), c["f"], c["idx"])) and not torch.equal(mid, a)       # a new module: nothing cached for it
            with torch.no_grad():
                dg.layer2[1].weight.mul_(3.0)                             # max|gamma| of layer 2 now gives the bound: another scale
            after = DG._host(dg, c["f"], c["idx"])
            assert torch.equal(after, DG._host(copy.deepcopy(dg), c["f"], c["idx"])) and not torch.equal(after, mid)


# ---- 5. whole tokenizer ------------------------------------------------------------------------------------------------------------------------------------
def test_tokenizer_features_are_as_close_to_the_oracle_as_with_the_switch_off(dev):
    """full Stage-II tokenizer geometry at B = 2 (T = 128) with the oracle's gumbel draws replayed; the row threshold lowered so that both DGCNNs take the path"""
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
    sw = lambda on: _set(TOKENIZER_DGCNN_F16X3=on, DGCNN_F16X3_MIN_T=128)

    def run(on):
        with torch.no_grad(), sw(on):
            return tok.forward_tokenizer_features(nb, c, draws=Draws({"gumbel": gumbel}, device=dev))

    def logits(on):
        with torch.no_grad(), sw(on):
            return tok.dgcnn_1.features(tok.encoder(nb), c, DGCNN.graph_index(c))

    def codes(h):
        B, G, _ = c.shape
        noise = Draws({"gumbel": gumbel}, device=dev).get("gumbel", None)
        return K.gn_gumbel_argmax_gather(h, B, G, tok.dgcnn_1.layer5[1], tok.codebook, noise=noise)[1].reshape(-1).cpu()

    rel_max = lambda a: ((a.double().cpu() - tf_o.double()).abs().max() / tf_o.double().abs().max()).item()
    off, on = run(False), run(True)
    e_off, e_on = rel_max(off), rel_max(on)
    h_off, h_on = logits(False), logits(True)
    i_off, i_on = codes(h_off), codes(h_on)
    # smallest top-two margin of (GroupNorm(logits) + gumbel) over the 128 tokens, from the switch-off logits in float64
    B, G, _ = c.shape
    gn = tok.dgcnn_1.layer5[1]
    z = torch.nn.functional.group_norm(h_off.double().cpu().reshape(B, G, -1).permute(0, 2, 1), gn.num_groups, gn.weight.double().cpu(), gn.bias.double().cpu(), gn.eps)
    noise = Draws({"gumbel": gumbel}, device=dev).get("gumbel", None).double().cpu().reshape(B, G, -1)
    top2 = (z.permute(0, 2, 1) + noise).topk(2, dim=2).values
    margin = (top2[..., 0] - top2[..., 1]).min().item()
    print(f"tokenizer features vs CPU oracle: switch off {e_off:.3e}  on (default) {e_on:.3e}; codes that differ: {int((i_off != i_on).sum())} of {i_off.numel()}; "
          f"smallest top-two margin {margin:.3e}")
    assert not torch.equal(h_on, h_off)
    assert torch.equal(off, run(False)) and torch.equal(on, run(True))
    assert e_on <= 2 * e_off, (e_on, e_off)
