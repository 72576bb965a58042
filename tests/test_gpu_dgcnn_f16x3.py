"""The head product of the frozen tokenizer's DGCNN on split-f16 planes (act_dgcnn_features_f16x3_f32, composite.dgcnn_features, ACT_TOKENIZER_F16X3):
as close to a float64 restatement of the whole DGCNN as the f32 entry (within 1.5 x, the gate of tests/test_gpu_f16x3.py), every unusable-x3 case equals the
f32 entry bit for bit, the range guard withholds the scale when the bound passes 2^15, the codes drawn from the logits agree wherever float64 separates the
top two, the plane cache follows in-place changes, and the whole tokenizer sits as close to the CPU oracle as with the f32 head (within 2 x).

Shapes are (B, G, k, Cin, Cout) with GroupNorm groups = 4; the graph is a fixed random one (tests/dgcnn_ref.graph), so every reference is CPU-reproducible."""
import copy
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dgcnn_ref as DR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_NN = 4
ACCURACY = [(2, 64, 4, 384, 128), (3, 128, 4, 256, 384), (2, 64, 4, 384, 8192)]       # T = 128: one workgroup; T = 384: 9, a remainder in the XCD remap; the real width
HEAD = (2, 64, 4, 384, 8192)
CODE_SEED = 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _layers(dg):
    return (dg.layer1, dg.layer2, dg.layer3, dg.layer4)


def _module(Cin, Cout, seed):
    """a frozen DGCNN on the CPU: torch's default initialisation under ``seed``, every GroupNorm affine moved off (1, 0)"""
    from act_amd.models.dvae import DGCNN
    torch.manual_seed(seed)
    dg = DGCNN(Cin, Cout)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for layer in _layers(dg) + (dg.layer5,):
            layer[1].weight.add_(0.1 * torch.randn(layer[1].weight.shape, generator=g))
            layer[1].bias.add_(0.1 * torch.randn(layer[1].bias.shape, generator=g))
    for p in dg.parameters():
        p.requires_grad = False
    return dg.eval()


def _inputs(B, G, Cin, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.standard_normal((B, G, Cin)).astype(np.float32)), torch.from_numpy(DR.graph(rng, B, G, K_NN))


def _ref64(dg, f, idx):
    """float64 restatement of DGCNN.features: -> (cat [T, 2304], h [T, Cout])"""
    n = lambda t: t.detach().cpu().double().numpy()
    B, G, Cin = f.shape
    idx = idx.cpu().numpy()
    x = n(f).reshape(B * G, Cin) @ n(dg.input_trans.weight)[:, :, 0].T + n(dg.input_trans.bias)
    outs = []
    for layer in _layers(dg):
        w = n(layer[0].weight)[:, :, 0, 0]
        cout, cin = w.shape[0], w.shape[1] // 2
        wa, wb = w[:, :cin], w[:, cin:]
        yz = np.concatenate((x @ wa.T, x @ (wb - wa).T), axis=1)
        x, _, _ = DR.edge_tail(yz, cout, idx, B, G, K_NN, cout, layer[1].num_groups, n(layer[1].weight), n(layer[1].bias), layer[1].eps, 0.2)
        outs.append(x)
    cat = np.concatenate(outs, axis=1)
    return cat, cat @ n(dg.layer5[0].weight)[:, :, 0].T


def _native(dg, f, idx, x3=None, edit=None, want_cat=False):
    """one call of the native entry on the device module ``dg``: act_dgcnn_features_f32, or (x3 = True) act_dgcnn_features_f16x3_f32 with the struct the host
    path builds, after ``edit(x3, T)`` changed it"""
    import act_amd.composite as CP
    from act_amd import _C
    lib, _p = _C.lib, CP._p
    B, G, Cin = f.shape
    w5 = dg.layer5[0].weight
    with torch.no_grad():
        stacked = [dg._stacked_weight(layer[0]) for layer in _layers(dg)]
    m = CP.Dgcnn()
    gn0 = dg.layer1[1]
    m.B, m.G, m.k, m.Cin, m.Cout, m.groups = B, G, idx.shape[1], Cin, w5.shape[0], gn0.num_groups
    m.eps, m.slope = float(gn0.eps), 0.2
    m.w_in, m.b_in, m.w5 = _p(dg.input_trans.weight), _p(dg.input_trans.bias), _p(w5)
    for l, layer in enumerate(_layers(dg)):
        m.stacked[l], m.gn_w[l], m.gn_b[l] = _p(stacked[l]), _p(layer[1].weight), _p(layer[1].bias)
    scratch = torch.empty(int(lib.act_dgcnn_scratch_floats(ctypes.byref(m))), dtype=torch.float32, device=f.device)
    h = torch.empty(B * G, m.Cout, dtype=torch.float32, device=f.device)
    ws = CP.K.workspace(f.device)
    args = (ctypes.byref(m), _p(f), _p(idx), _p(h), _p(scratch), _p(ws), ws.numel() * 4)
    CP.ensure_tuned(("dgcnn", B, G, Cin, m.Cout), lambda: lib.act_dgcnn_features_f32(*args, _C.stream()), f.device)     # the host path's key: one configuration for both
    if x3 is None:
        _C.check(lib.act_dgcnn_features_f32(*args, _C.stream()), "act_dgcnn_features_f32")
    else:
        s, keep = CP._dgcnn_f16_planes(dg, B * G, G, m.k, f.device)
        if edit is not None:
            edit(s, B * G)
        _C.check(lib.act_dgcnn_features_f16x3_f32(args[0], ctypes.byref(s), *args[1:], _C.stream()), "act_dgcnn_features_f16x3_f32")
        torch.cuda.synchronize()
        del keep
    if want_cat:                                          # scratch = x0 [T, 128] | yz [T, 2048] | cat [T, 2304] | statistics
        T = B * G
        return h, scratch[T * 2176:T * 2176 + T * 2304].view(T, 2304).clone()
    return h


@functools.lru_cache(maxsize=None)
def _case(shape, seed=0):
    """module (CPU + device copy), inputs, the float64 reference and both entries' outputs of one shape: computed once, shared, never changed"""
    B, G, k, Cin, Cout = shape
    assert k == K_NN
    dev = torch.device("cuda:0")
    cpu = _module(Cin, Cout, 100 + seed)
    f, idx = _inputs(B, G, Cin, 200 + seed)
    cat64, h64 = _ref64(cpu, f, idx)
    dg = copy.deepcopy(cpu).to(dev)
    fd, idxd = f.to(dev), idx.to(dev)
    h32, cat = _native(dg, fd, idxd, want_cat=True)
    h16 = _native(dg, fd, idxd, x3=True)
    return dict(cpu=cpu, dg=dg, f=fd, idx=idxd, cat64=cat64, h64=h64, h32=h32, h16=h16, cat=cat)


def _rel_l2(x, ref):
    ref = torch.from_numpy(ref) if isinstance(ref, np.ndarray) else ref.double().cpu()
    return ((x.double().cpu() - ref).norm() / ref.norm()).item()


def _host(dg, f, idx):
    with torch.no_grad():
        return dg.features(f, None, idx)


class _switch:
    """composite.TOKENIZER_F16X3 for the duration of a block"""
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        import act_amd.composite as CP
        self.saved, CP.TOKENIZER_F16X3 = CP.TOKENIZER_F16X3, self.on

    def __exit__(self, *a):
        import act_amd.composite as CP
        CP.TOKENIZER_F16X3 = self.saved


# ---- 1. accuracy -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ACCURACY)
def test_the_split_head_is_as_close_to_float64_as_the_f32_head(dev, shape):
    """measured on MI355X: see notebook/tokenizer_f16x3.md"""
    c = _case(shape)
    e32, e16 = _rel_l2(c["h32"], c["h64"]), _rel_l2(c["h16"], c["h64"])
    print(f"{shape}: relative L2 against float64: f32 head {e32:.3e}  split-f16 head {e16:.3e}  ratio {e16 / e32:.2f}  (cat {_rel_l2(c['cat'], c['cat64']):.3e})")
    assert not torch.equal(c["h16"], c["h32"])            # the entry really took the other kernel
    assert e16 <= 1.5 * e32, (e16, e32)


def test_the_host_path_takes_the_split_head_from_1024_columns_on(dev):
    c = _case(HEAD)
    assert torch.equal(_host(c["dg"], c["f"], c["idx"]), c["h16"])
    small = _case((2, 64, 4, 384, 128))
    assert torch.equal(_host(small["dg"], small["f"], small["idx"]), small["h32"])        # below 1024 columns: the f32 entry


# ---- 2. fallbacks ------------------------------------------------------------------------------------------------------------------------------------------
def _zero_scale(s, T):
    s.a_scale = 0.0


def _null_planes(s, T):
    s.w5_planes = None


def _null_scratch(s, T):
    s.a_planes = None


def _one_short(s, T):
    s.a_planes_elems = 2 * T * 2304 - 1


@pytest.mark.parametrize("shape,edit", [((2, 64, 4, 384, 200), None), ((2, 48, 4, 384, 128), None), ((2, 64, 4, 384, 128), _zero_scale),
                                        ((2, 64, 4, 384, 128), _null_planes), ((2, 64, 4, 384, 128), _null_scratch), ((2, 64, 4, 384, 128), _one_short)],
                         ids=["Cout=200", "T=96", "a_scale=0", "null-w5-planes", "null-a-planes", "one-element-short"])
def test_an_unusable_x3_equals_the_f32_entry_bit_for_bit(dev, shape, edit):
    c = _case(shape)
    if edit is None:
        assert torch.equal(c["h16"], c["h32"])            # a shape the kernel does not take
    else:
        assert not torch.equal(c["h16"], c["h32"])
        assert torch.equal(_native(c["dg"], c["f"], c["idx"], x3=True, edit=edit), c["h32"])


def _child():
    """run by test_the_switch_at_0_restores_the_f32_path in a fresh interpreter with ACT_TOKENIZER_F16X3=0"""
    import act_amd.composite as CP
    assert CP.TOKENIZER_F16X3 is False
    c = _case(HEAD)
    assert torch.equal(_host(c["dg"], c["f"], c["idx"]), c["h32"]) and not torch.equal(c["h16"], c["h32"])
    print("child-ok")


def test_the_switch_at_0_restores_the_f32_path(dev):
    env = dict(os.environ, ACT_TOKENIZER_F16X3="0")
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_dgcnn_f16x3 as T; T._child()"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "child-ok" in r.stdout, r.stdout + r.stderr


# ---- 3. range ----------------------------------------------------------------------------------------------------------------------------------------------
def test_planes_near_the_top_of_the_f16_range_keep_the_gate(dev):
    """The guard's bound grows with gamma as fast as the values do (max|cat| / bound is about 5 / sqrt(n), n = 65,536 here, whatever gamma is), so gamma alone
    cannot bring cat near the bound.  Two runs instead: (a) layer 4's gamma times 64 puts the bound in (2^14, 2^15], the scale at 1 and cat at its largest
    magnitudes under the guard, through the host path; (b) the native entry at the scale of a bound of twice the real max|cat| -- the planes then reach past
    2^14, half the limit the scale rule aims at.  Both: finite, and the gate of test 1."""
    import act_amd.composite as CP
    B, G, k, Cin, Cout = HEAD
    cpu = copy.deepcopy(_case(HEAD)["cpu"])
    with torch.no_grad():
        cpu.layer4[1].weight.mul_(64.0)
    f, idx = _inputs(B, G, Cin, 300)
    cat64, h64 = _ref64(cpu, f, idx)
    dg = copy.deepcopy(cpu).to(dev)
    f, idx = f.to(dev), idx.to(dev)
    h32, cat = _native(dg, f, idx, want_cat=True)
    e32 = _rel_l2(h32, h64)
    # (a)
    ha = _host(dg, f, idx)
    sc = CP._DGCNN_F16[dg][7][(G, k)]
    bound = CP.f16x3_dgcnn_bound(*CP._DGCNN_F16[dg][3:7], G, k)
    assert sc == 1.0 and 16384.0 < bound <= 32768.0, (sc, bound)
    ea = _rel_l2(ha, h64)
    # (b)
    top = cat.abs().max().item()
    sb = CP.f16x3_act_scale(2 * top)

    def at(s, T):
        s.a_scale = sb
    hb = _native(dg, f, idx, x3=True, edit=at)
    eb = _rel_l2(hb, h64)
    print(f"bound {bound:.0f} max|cat| {top:.1f}: f32 head {e32:.3e}  guard's scale {sc:g}: {ea:.3e}  scale {sb:g} (planes to {top * sb:.0f}): {eb:.3e}")
    assert top <= bound and 8192.0 < top * sb <= 16384.0
    assert torch.isfinite(ha).all() and torch.isfinite(hb).all() and not torch.equal(ha, h32) and not torch.equal(hb, h32)
    assert ea <= 1.5 * e32 and eb <= 1.5 * e32, (ea, eb, e32)


def test_a_bound_past_2_pow_15_keeps_the_head_on_the_f32_kernel(dev):
    import act_amd.composite as CP
    B, G, k, Cin, Cout = HEAD
    dg = copy.deepcopy(_case(HEAD)["cpu"]).to(dev)
    with torch.no_grad():
        dg.layer4[1].weight.mul_(256.0)                   # sqrt(65,536) * 256 * max|gamma| > 2^15
    f, idx = (t.to(dev) for t in _inputs(B, G, Cin, 301))
    out = _host(dg, f, idx)
    assert CP._DGCNN_F16[dg][7][(G, k)] == 0.0
    assert torch.equal(out, _native(dg, f, idx))


# ---- 4. codes ----------------------------------------------------------------------------------------------------------------------------------------------
def _code_inputs():
    """gumbel noise [B, G, 8192] and a codebook for HEAD, from CODE_SEED.  The float64 top-two margin of (logit + g) over the 128 tokens at this seed:
    smallest 8.83e-3 (computed on the CPU from _ref64: nothing below 1e-4, no token is excluded; seeds 1 and 2 give 3.1e-3 and 2.3e-2)"""
    B, G, _, _, C = HEAD
    rng = np.random.default_rng(CODE_SEED)
    noise = -np.log(rng.exponential(size=(B, G, C)))
    return noise.astype(np.float32), rng.standard_normal((C, 16)).astype(np.float32)


def test_the_codes_agree_wherever_float64_separates_the_top_two(dev):
    import act_amd.kernels as K
    B, G, _, _, C = HEAD
    c = _case(HEAD)
    noise, codebook = _code_inputs()
    gn = c["cpu"].layer5[1]
    n = lambda t: t.detach().double().numpy()
    _, index64, _, gap, _, _ = DR.gumbel_argmax_gather(c["h64"], B, G, C, gn.num_groups, n(gn.weight), n(gn.bias), noise.astype(np.float64), 1.0, codebook, gn.eps)
    print(f"float64 top-two margins: smallest {gap.min():.3e}, {int((gap < 1e-4).sum())} of {gap.size} below 1e-4")
    assert gap.min() >= 1e-4                              # the seed's condition: every token counts
    noise_d, cb_d = torch.from_numpy(noise).to(dev), torch.from_numpy(codebook).to(dev)
    gnd = c["dg"].layer5[1]
    i32 = K.gn_gumbel_argmax_gather(c["h32"], B, G, gnd, cb_d, noise=noise_d)[1].cpu().numpy().reshape(-1)
    i16 = K.gn_gumbel_argmax_gather(c["h16"], B, G, gnd, cb_d, noise=noise_d)[1].cpu().numpy().reshape(-1)
    keep = gap >= 1e-4
    assert np.array_equal(i32[keep], index64[keep]) and np.array_equal(i16[keep], index64[keep]), (np.flatnonzero(i16 != index64), np.flatnonzero(i32 != index64))


# ---- 5. determinism and the cache --------------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_equal_and_the_cache_follows_in_place_changes(dev):
    c = _case(HEAD)
    dg = copy.deepcopy(c["dg"])
    a, b = _host(dg, c["f"], c["idx"]), _host(dg, c["f"], c["idx"])
    assert torch.equal(a, b) and torch.equal(a, c["h16"])
    with torch.no_grad():
        dg.layer5[0].weight.mul_(1.5)                     # (not a power of two: the planes themselves change)
        dg.layer2[1].weight.mul_(3.0)                     # max|gamma| of layer 2 now gives the bound: another scale
    after = _host(dg, c["f"], c["idx"])
    fresh = copy.deepcopy(dg)                             # a new module: nothing cached for it
    assert torch.equal(after, _host(fresh, c["f"], c["idx"]))
    assert not torch.equal(after, a)


# ---- 6. whole tokenizer ------------------------------------------------------------------------------------------------------------------------------------
def test_tokenizer_features_are_as_close_to_the_oracle_as_with_the_f32_head(dev):
    """full Stage-II tokenizer geometry at B = 2 with the oracle's gumbel draws replayed (the rule of the teacher's ViT change: within 2 x)"""
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
    oracle.dvae_tokenizer.prompt_p = 0.0; model.dvae_tokenizer.prompt_dropout.p = 0.0
    pts = torch.from_numpy(clouds(6, 2, 1024))
    with torch.no_grad():
        nb_o, c_o = oracle.group_divider(pts)
        rec = OL.Draws(record=True)
        tf_o = oracle.dvae_tokenizer.forward_tokenizer_features(nb_o, c_o, rec)
        nb, c = model.group_divider(pts.to(dev))

    def run(on):
        with torch.no_grad(), _switch(on):
            return model.dvae_tokenizer.forward_tokenizer_features(nb, c, draws=Draws({"gumbel": rec.table["gumbel"]}, device=dev))

    rel_max = lambda a: ((a.double().cpu() - tf_o.double()).abs().max() / tf_o.double().abs().max()).item()
    f32, x3 = run(False), run(True)
    e32, e16 = rel_max(f32), rel_max(x3)
    print(f"tokenizer features vs CPU oracle: f32 head {e32:.3e}  split-f16 head (default) {e16:.3e}")
    assert torch.equal(f32, run(False)) and torch.equal(x3, run(True))
    assert e16 <= 2 * e32, (e16, e32)
