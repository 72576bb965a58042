"""Keys / values of the default teacher's prompt rows as ONE dense split-f16 product (act_prompt_kv_fwd_f16x3_f32: prompt LayerNorm to f16 planes + the planes
product of csrc/gemm_bf16x3.hip).  Kernel level: the planes equal a split of K.prompt_layernorm's rows bit for bit; the entry equals the hand-composed
sequence bit for bit and sits as close to the float64 product of those rows as the dense f32 kernel (bar 2e-5 of tests/test_gpu_prompt_kv.py, and within
1.5 x the f32 product's error).  Every refusal leaves the output untouched.  Model level: the whole teacher with the switch on against off."""
import os
import subprocess
import sys

import pytest
import torch

from tests import f16x3_ref as R

pytestmark = pytest.mark.gpu

BAR = 2e-5          # the project's bar for fp32 products (tests/test_gpu_prompt_kv.py)
EPS = 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(a, ref):
    a = a.detach().double().cpu(); ref = ref.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return ((a - ref).abs().max() / max(1.0, ref.abs().max())).item()


def _rel_l2(a, ref):
    return ((a.double() - ref).norm() / ref.norm()).item()


def _inputs(P, D, N, dev, offset=0.0, seed=0):
    """the generator of tests/test_gpu_prompt_kv.py"""
    g = torch.Generator().manual_seed(1000 + 7 * P + D + N + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    tok, ppos = r(P, D), r(P, D) * 0.5 + offset
    gamma, beta = 1.0 + 0.2 * r(D), 0.1 * r(D)
    w, bias = r(N, D) / D ** 0.5, 0.1 * r(N)
    return [t.to(dev) for t in (tok, ppos, gamma, beta, w, bias)]


def _scale(gamma, beta):
    """the static scale the teacher gives its qkv Linear: from the weight-only bound on a LayerNorm row"""
    return R.act_scale(R.ln_bound(gamma.cpu().numpy(), beta.cpu().numpy()).max())


def _w_planes(K, w):
    sb, sb_inv = K.f16x3_row_scales(w)
    return K.split_f16x2(w, 1.0, sb), sb_inv.contiguous()


# ---- LayerNorm to planes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P,D", [(2, 64, 128), (3, 5, 128), (2, 64, 768)])
@pytest.mark.parametrize("drop_p", [0.0, 0.1, 0.5])
def test_layernorm_planes_equal_a_split_of_the_fp32_rows(dev, B, P, D, drop_p):
    import act_amd.kernels as K
    tok, ppos, gamma, beta, _, _ = _inputs(P, D, 128, dev)
    s = _scale(gamma, beta)
    rows = K.prompt_layernorm(tok, ppos, B, drop_p, 5, gamma, beta, EPS)
    planes = K.prompt_layernorm_f16_planes(tok, ppos, B, drop_p, 5, gamma, beta, EPS, s)
    assert torch.equal(planes, K.split_f16x2(rows, s))
    assert torch.equal(rows, K.prompt_layernorm(tok, ppos, B, drop_p, 5, gamma, beta, EPS))


def test_layernorm_planes_device_seed_and_bad_arguments(dev):
    import act_amd.kernels as K
    B, P, D = 3, 5, 128
    tok, ppos, gamma, beta, _, _ = _inputs(P, D, 128, dev)
    s = _scale(gamma, beta)
    ctr = torch.tensor([12345], dtype=torch.int64, device=dev)
    rows = K.prompt_layernorm(tok, ppos, B, 0.1, 5, gamma, beta, EPS, seed_dev=ctr)
    planes = K.prompt_layernorm_f16_planes(tok, ppos, B, 0.1, 5, gamma, beta, EPS, s, seed_dev=ctr)
    assert torch.equal(planes, K.split_f16x2(rows, s))
    assert not torch.equal(planes, K.prompt_layernorm_f16_planes(tok, ppos, B, 0.1, 5, gamma, beta, EPS, s))      # the counter is part of the key
    sentinel = torch.full((2, B * P, D), 7.0, dtype=torch.float16, device=dev)
    buf = sentinel.clone()
    call = lambda h1, h2, sc: K.lib.act_prompt_layernorm_fwd_f16_planes_f32(tok.data_ptr(), ppos.data_ptr(), B, P, D, 0.1, 5, None, gamma.data_ptr(),
                                                                            beta.data_ptr(), EPS, h1, h2, sc, None)
    assert call(buf[0].data_ptr(), buf[1].data_ptr(), 0.0) == -1                      # ACT_E_BADARG: no scale
    assert call(buf[0].data_ptr(), buf[1].data_ptr(), -2.0) == -1
    assert call(buf[0].data_ptr() + 2, buf[1].data_ptr(), s) == -1                    # a plane that is not 8-byte aligned
    torch.cuda.synchronize()
    assert torch.equal(buf, sentinel)


# ---- the entry -------------------------------------------------------------------------------------------------------------------------------------------
def _entry_case(K, dev, B, P, D, N, drop_p, offset=0.0, seed=5, tile=0):
    tok, ppos, gamma, beta, w, bias = _inputs(P, D, N, dev, offset)
    s = _scale(gamma, beta)
    wp, winv = _w_planes(K, w)
    got = K.prompt_kv_f16x3(tok, ppos, B, drop_p, seed, gamma, beta, EPS, wp, winv, s, bias=bias, tile=tile)
    assert got is not None
    return got, (tok, ppos, gamma, beta, w, bias, s, wp, winv)


@pytest.mark.parametrize("B,P,D,N", [(2, 64, 128, 256), (6, 64, 128, 384), (2, 64, 768, 1536)])
@pytest.mark.parametrize("drop_p,offset", [(0.0, 0.0), (0.1, 0.0), (0.5, 0.0), (0.1, 3.0)])
def test_entry_matches_float64_rows_and_the_hand_composed_sequence(dev, B, P, D, N, drop_p, offset):
    import act_amd.kernels as K
    got, (tok, ppos, gamma, beta, w, bias, s, wp, winv) = _entry_case(K, dev, B, P, D, N, drop_p, offset)
    rows = K.prompt_layernorm(tok, ppos, B, drop_p, 5, gamma, beta, EPS)
    ref = rows.double() @ w.double().T + bias.double()
    dense = K.gemm(rows, w, True, True, bias=bias)
    e_new, e_dense = _rel(got, ref), _rel(dense, ref)
    l_new, l_dense = _rel_l2(got, ref), _rel_l2(dense, ref)
    print(f"prompt_kv_f16x3 B={B} P={P} D={D} N={N} p={drop_p} offset={offset}: max split-f16 {e_new:.3e} f32 {e_dense:.3e}  "
          f"L2 split-f16 {l_new:.3e} f32 {l_dense:.3e} ratio {l_new / l_dense:.2f}")
    assert e_new <= BAR
    assert l_new <= 1.5 * l_dense, (l_new, l_dense)
    by_hand = K.gemm_nt_f16x3(K.split_f16x2(rows, s), s, wp, winv, bias=bias)
    assert torch.equal(got, by_hand)
    if N % 192 == 0:                                     # both tile forms, forced: the bits do not depend on the tile
        t128, _ = _entry_case(K, dev, B, P, D, N, drop_p, offset, tile=128)
        t192, _ = _entry_case(K, dev, B, P, D, N, drop_p, offset, tile=192)
        assert torch.equal(t128, t192) and torch.equal(t128, got)


def test_entry_is_deterministic_and_follows_the_seed(dev):
    import act_amd.kernels as K
    a, _ = _entry_case(K, dev, 6, 64, 128, 384, 0.1, seed=5)
    b, _ = _entry_case(K, dev, 6, 64, 128, 384, 0.1, seed=5)
    c, _ = _entry_case(K, dev, 6, 64, 128, 384, 0.1, seed=6)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    v = a.view(6, 64, 384)
    assert not torch.equal(v[0], v[1])                   # every cloud draws its own mask


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def _refused(K, dev, B, P, D, N, *, scale=None, null_plane=None, short=False):
    """the raw entry on a sentinel-filled output -> (return code, output untouched)"""
    tok, ppos, gamma, beta, w, bias = _inputs(P, D, N, dev)
    s = _scale(gamma, beta) if scale is None else scale
    sb, sb_inv = K.f16x3_row_scales(w)
    wp = K.split_f16x2(w, 1.0, sb)
    planes = torch.empty(2 * B * P * D - (8 if short else 0), dtype=torch.float16, device=dev)
    ptrs = dict(w_h1=wp[0].data_ptr(), w_h2=wp[1].data_ptr(), w_inv=sb_inv.data_ptr(), planes=planes.data_ptr())
    if null_plane:
        ptrs[null_plane] = None
    out = torch.full((B * P, N), -77.0, device=dev)
    rc = K.lib.act_prompt_kv_fwd_f16x3_f32(tok.data_ptr(), ppos.data_ptr(), B, P, D, N, 0.1, 5, None, gamma.data_ptr(), beta.data_ptr(), EPS, ptrs["w_h1"],
                                           ptrs["w_h2"], ptrs["w_inv"], s, bias.data_ptr(), out.data_ptr(), ptrs["planes"], planes.numel(), 0, None)
    torch.cuda.synchronize()
    return rc, bool((out == -77.0).all())


@pytest.mark.parametrize("case", ["rows", "N=201", "a_scale=0", "null w_h1", "null w_h2", "null w_inv", "null planes", "short scratch", "setter"])
def test_refusals_launch_nothing(dev, case):
    import act_amd.kernels as K
    B, P, D, N = 2, 64, 128, 256
    assert K.lib.act_prompt_kv_f16x3(-1) == 1
    if case == "rows":
        rc, clean = _refused(K, dev, 3, 5, D, N)
    elif case == "N=201":
        rc, clean = _refused(K, dev, B, P, D, 201)
    elif case == "a_scale=0":
        rc, clean = _refused(K, dev, B, P, D, N, scale=0.0)
    elif case.startswith("null"):
        rc, clean = _refused(K, dev, B, P, D, N, null_plane=case.split()[1])
    elif case == "short scratch":
        rc, clean = _refused(K, dev, B, P, D, N, short=True)
    else:
        prev = K.lib.act_prompt_kv_f16x3(0)
        try:
            assert prev == 1 and K.lib.act_prompt_kv_f16x3(-1) == 0
            rc, clean = _refused(K, dev, B, P, D, N)
        finally:
            K.lib.act_prompt_kv_f16x3(prev)
        assert _refused(K, dev, B, P, D, N) == (0, False)             # back on: the same call is taken and writes
    assert rc == -3 and clean, (case, rc, clean)


# ---- whole teacher ---------------------------------------------------------------------------------------------------------------------------------------
def _teacher(dev):
    """the tokenizer of configs[1] (ViT-B geometry, 64 prompts, depth 12), randomly initialised, with drawn prompt tables; B = 2 -> 128 patch tokens"""
    from act_amd.models import build_model_from_cfg
    from act_amd.utils.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file("cfgs/pretrain/pretrain_act_distill.yaml").model
    cfg.dvae_config.ckpt = "none"
    torch.manual_seed(2)
    tk = build_model_from_cfg(cfg).dvae_tokenizer
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for name in ("visual_prompt_token", "visual_prompt_pos", "deep_prompt_tokens", "deep_prompt_pos"):
            p = getattr(tk, name)
            p.copy_(0.5 * torch.randn(p.shape, generator=g))
    tk.to(dev).train()
    x = torch.randn(2, 64, tk.proj_pre.weight.shape[1], generator=g).to(dev)
    c = torch.randn(2, 64, 3, generator=g).to(dev)
    return tk, x, c


def _run_teacher(tk, x, c, on):
    """act_prefix_vit_fwd_f16x3_f32, prompt dropout 0.1, with the switch set -> (features, launches by profiled kernel id)"""
    import act_amd._C as C
    import act_amd.composite as CP
    saved = CP.TEACHER_F16X3, CP.TEACHER_BF16X3
    CP.TEACHER_F16X3, CP.TEACHER_BF16X3 = True, False
    prev = C.lib.act_prompt_kv_f16x3(1 if on else 0)
    was = C.prof_enable(True)
    try:
        with torch.no_grad():
            CP.prefix_vit_forward(tk, x, c, 0.1, 4242, None)            # (tunes the f32 shapes on the first call; not counted)
            torch.cuda.synchronize()
            C.prof_reset()
            out = CP.prefix_vit_forward(tk, x, c, 0.1, 4242, None)
        torch.cuda.synchronize()
        return out, {k: v["launches"] for k, v in C.prof_table().items()}
    finally:
        C.prof_enable(bool(was))
        C.lib.act_prompt_kv_f16x3(prev)
        CP.TEACHER_F16X3, CP.TEACHER_BF16X3 = saved


def test_whole_teacher_with_the_switch_on_against_off(dev):
    """measured on MI355X: see notebook/prompt_kv_f16x3.md"""
    tk, x, c = _teacher(dev)
    depth = tk.visual_embed_depth
    on_a, k_on = _run_teacher(tk, x, c, True)
    off_a, k_off = _run_teacher(tk, x, c, False)
    on_b, _ = _run_teacher(tk, x, c, True)
    off_b, _ = _run_teacher(tk, x, c, False)
    e = ((on_a.double() - off_a.double()).abs().max() / off_a.double().abs().max()).item()
    print(f"teacher features, prompt keys/values split-f16 vs sparse f32: max |d| / max |ref| = {e:.3e}; launches on {k_on} off {k_off}")
    assert torch.equal(off_a, off_b)                                  # the sparse path is untouched by the switch having been used
    assert torch.equal(on_a, on_b)                                    # deterministic
    assert not torch.equal(on_a, off_a)                               # the switch really took the other kernels
    assert torch.isfinite(on_a).all() and e <= 1e-4, e                # the project's parity bar
    assert k_on.get("prompt_kv_sparse", 0) == 0 and k_off.get("prompt_kv_sparse", 0) == depth
    assert k_on["sgemm_nt_bf16x3"] == k_off["sgemm_nt_bf16x3"] + depth


_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
import torch
from tests.test_gpu_prompt_kv_f16x3 import _teacher
import act_amd._C as C
import act_amd.composite as CP
assert C.lib.act_prompt_kv_f16x3(-1) == 0
tk, x, c = _teacher(torch.device("cuda:0"))
CP.TEACHER_F16X3, CP.TEACHER_BF16X3 = True, False
C.prof_enable(True)
with torch.no_grad():
    CP.prefix_vit_forward(tk, x, c, 0.1, 4242, None)
    torch.cuda.synchronize()
    C.prof_reset()
    CP.prefix_vit_forward(tk, x, c, 0.1, 4242, None)
torch.cuda.synchronize()
t = C.prof_table()
print("KIDS", t.get("prompt_kv_sparse", {{}}).get("launches", 0), t["sgemm_nt_bf16x3"]["launches"], tk.visual_embed_depth)
"""


def test_environment_switch_restores_the_sparse_kernels(dev):
    """ACT_PROMPT_KV_F16X3=0 is read once, natively: a fresh process runs the sparse walk in every layer and only the four products per layer on split-f16"""
    env = dict(os.environ, ACT_PROMPT_KV_F16X3="0")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("KIDS")][-1].split()
    sparse, x3, depth = int(line[1]), int(line[2]), int(line[3])
    assert sparse == depth and x3 == 4 * depth, line
