"""K-tile-major ("KT") planes of the split-f16 GEMM (csrc/gemm_bf16x3.hip, notebook/x3_ktile.md): element (r, k) of a plane [R][K] at
((k / 32) R + r) 32 + k % 32, so that a workgroup stages an operand tile in whole 128-byte lines.  The kernel walks either layout through a row stride and a
K-tile stride; the values and the order of summation are those of the row-major launch, so every comparison here is torch.equal against that launch on the same
operands (which tests/test_gpu_f16x3.py holds to float64)."""
import ctypes

import pytest
import torch

from tests import f16x3_ref as R

pytestmark = pytest.mark.gpu

BADARG = -1                                                       # ACT_E_BADARG (include/act_hip.h)
ROW, KT = 0, 1                                                    # ACT_X3_ROWMAJOR, ACT_X3_KTILE


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rand(dev, rows, cols, seed, weight=False):
    g = torch.Generator().manual_seed(seed)
    if weight:                                                    # rows of different magnitude: different row scales
        return (0.05 * torch.randn(rows, cols, generator=g) * torch.exp(torch.randn(rows, 1, generator=g))).to(dev)
    return torch.randn(rows, cols, generator=g).to(dev)


def _operands(dev, M, N, Kd, seed):
    """row-major planes of random operands: activations at one static scale, weights at one power of two per row -> (a planes, s_a, b planes, 1 / s_b)"""
    import act_amd.kernels as K
    a, w = _rand(dev, M, Kd, seed), _rand(dev, N, Kd, seed + 1, weight=True)
    s_a = R.act_scale(a.abs().max().item())
    sb, sb_inv = K.f16x3_row_scales(w)
    return K.split_f16x2(a, s_a), s_a, K.split_f16x2(w, 1.0, sb), sb_inv


def _flat(planes, offset=0):
    """the (h1, h2) pair of a planes tensor [2, rows, cols] from element ``offset`` of each plane on"""
    return planes[0].reshape(-1)[offset:], planes[1].reshape(-1)[offset:]


def _same(x, y):
    return not torch.isnan(x.float()).any().item() and torch.equal(x, y)


def _nan(dev, *shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


# ---- the repack and the split that writes the layout ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(128, 64), (384, 128), (256, 3072)])
def test_repack_is_the_permutation_of_the_layout(dev, rows, cols):
    import act_amd.kernels as K
    src = torch.randint(-32768, 32767, (2, rows, cols), dtype=torch.int16, device=dev)
    kt = K.repack_ktile(src)
    for p in range(2):
        assert torch.equal(kt[p].view(cols // 32, rows, 32).permute(1, 0, 2).reshape(rows, cols), src[p])
        assert torch.equal(K.ktile_rows(kt[p], rows, cols), src[p])
    a = _rand(dev, rows, cols, rows + cols)
    s_a = R.act_scale(a.abs().max().item())
    assert torch.equal(K.split_f16x2_kt(a, s_a), K.repack_ktile(K.split_f16x2(a, s_a)))           # the split-to-KT pass = the repack of the dense split


def test_split_to_kt_writes_a_column_slice_of_a_wider_buffer(dev):
    """the tokenizer's cat planes: each tail writes its slice; the slice at column c of [T][W] planes starts (c / 32) T 32 elements in"""
    import act_amd.kernels as K
    T, W, off, w = 256, 256, 64, 128
    a = _rand(dev, T, W, 5)
    s_a = R.act_scale(a.abs().max().item())
    buf = torch.zeros(2, T, W, dtype=torch.float16, device=dev)
    o = (off // 32) * T * 32
    from act_amd import _C
    sl = a[:, off:off + w]
    _C.check(_C.lib.act_split_f16x2_kt_f32(_C.ptr_rows(sl), T, w, sl.stride(0), float(s_a), _C.ptr(_flat(buf, o)[0]), _C.ptr(_flat(buf, o)[1]), T, _C.stream()),
             "act_split_f16x2_kt_f32")
    whole = K.repack_ktile(K.split_f16x2(a, s_a))
    for p in range(2):
        got, want = buf[p].reshape(-1), whole[p].reshape(-1)
        assert torch.equal(got[o:o + T * w], want[o:o + T * w])
        assert not got[:o].any() and not got[o + T * w:].any()        # nothing outside the slice


# ---- the product --------------------------------------------------------------------------------------------------------------------------------------------
# (256, 384, 128): both tiles forced -- 6 workgroups of 128 x 128 (the XCD remap with a remainder), 4 of 128 x 192 (the partial staging pass of the 8-wave form)
@pytest.mark.parametrize("M,N,Kd,tiles", [(128, 128, 64, (0,)), (256, 384, 128, (128, 192)), (128, 128, 3072, (0,))],
                         ids=["two-k-tiles", "both-tiles", "deep-k"])
def test_kt_operands_give_the_bits_of_the_row_major_launch(dev, M, N, Kd, tiles):
    import act_amd.kernels as K
    ap, s_a, bp, sb_inv = _operands(dev, M, N, Kd, M + N + Kd)
    akt, bkt = K.repack_ktile(ap), K.repack_ktile(bp)
    for tile in tiles:
        want = K.gemm_nt_f16x3(ap, s_a, bp, sb_inv, tile=tile)
        for a, la, b, lb in [(ap, ROW, bkt, KT), (akt, KT, bp, ROW), (akt, KT, bkt, KT), (ap, ROW, bp, ROW)]:
            got = K.gemm_nt_f16x3_layout(M, N, Kd, _flat(a), s_a, _flat(b), sb_inv, a_layout=la, a_rows_total=M, b_layout=lb, b_rows_total=N,
                                         out=_nan(dev, M, N), tile=tile)
            assert _same(got, want), (tile, la, lb)


def test_rows_of_a_taller_kt_weight_the_prompt_kv_case(dev):
    """B = rows 128 .. 384 of a [384][128] weight: pointer 128 * 32 elements in, rows_total = 384"""
    import act_amd.kernels as K
    M, N, Kd, r0 = 384, 256, 128, 128
    ap, s_a, bp, sb_inv = _operands(dev, M, r0 + N, Kd, 11)
    want = K.gemm_nt_f16x3(ap, s_a, bp[:, r0:].contiguous(), sb_inv[r0:].contiguous())
    got = K.gemm_nt_f16x3_layout(M, N, Kd, _flat(ap), s_a, _flat(K.repack_ktile(bp), r0 * 32), sb_inv[r0:].contiguous(), b_layout=KT, b_rows_total=r0 + N,
                                 out=_nan(dev, M, N))
    assert _same(got, want)


def test_a_column_slice_of_a_wider_kt_buffer(dev):
    """A = columns 64 .. 192 of [256][256] planes: pointer (64 / 32) * 256 * 32 elements in, rows_total = 256"""
    import act_amd.kernels as K
    M, N, Kd, W, off = 256, 256, 128, 256, 64
    wide, s_a, bp, sb_inv = _operands(dev, M, N, W, 13)
    bp = bp[:, :, :Kd].contiguous()
    want = K.gemm_nt_f16x3(wide[:, :, off:off + Kd].contiguous(), s_a, bp, sb_inv)
    assert _same(K.gemm_nt_f16x3_layout(M, N, Kd, _flat(wide, off), s_a, _flat(bp), sb_inv, lda=W, out=_nan(dev, M, N)), want)      # row-major slice: lda
    for b, lb in [(bp, ROW), (K.repack_ktile(bp), KT)]:
        got = K.gemm_nt_f16x3_layout(M, N, Kd, _flat(K.repack_ktile(wide), (off // 32) * M * 32), s_a, _flat(b), sb_inv, a_layout=KT, a_rows_total=M,
                                     b_layout=lb, b_rows_total=N, out=_nan(dev, M, N))
        assert _same(got, want), lb


@pytest.mark.parametrize("case", ["bias", "bias+gelu-kt-planes-only", "bias+res"])
@pytest.mark.parametrize("tile", [128, 192])
def test_epilogues_and_kt_planes_out(dev, case, tile):
    import act_amd.kernels as K
    M, N, Kd, N2 = 256, 384, 128, 128
    ap, s_a, bp, sb_inv = _operands(dev, M, N, Kd, 17)
    bkt = K.repack_ktile(bp)
    g = torch.Generator().manual_seed(len(case))
    bias = torch.randn(N, generator=g).to(dev)
    if case != "bias+gelu-kt-planes-only":
        kw = dict(bias=bias, res=torch.randn(M, N, generator=g).to(dev) if case == "bias+res" else None, tile=tile)
        want = K.gemm_nt_f16x3(ap, s_a, bp, sb_inv, **kw)
        got = K.gemm_nt_f16x3_layout(M, N, Kd, _flat(ap), s_a, _flat(bkt), sb_inv, b_layout=KT, b_rows_total=N, out=_nan(dev, M, N), **kw)
        assert _same(got, want) and not torch.equal(want, K.gemm_nt_f16x3(ap, s_a, bp, sb_inv, tile=tile))
        return
    # fc1 -> fc2: the hidden activation leaves fc1's epilogue as planes alone, K-tile-major, and is fc2's A operand as it stands
    s_o = 64.0
    row_planes = _nan(dev, 2, M, N, dtype=torch.float16)
    K.gemm_nt_f16x3(ap, s_a, bp, sb_inv, bias=bias, act=K.EPI_GELU, planes_out=row_planes, out_scale=s_o, tile=tile)
    kt_planes = _nan(dev, 2, M, N, dtype=torch.float16)
    K.gemm_nt_f16x3_layout(M, N, Kd, _flat(ap), s_a, _flat(bkt), sb_inv, b_layout=KT, b_rows_total=N, bias=bias, act=K.EPI_GELU, want_c=False,
                           planes_out=kt_planes, out_scale=s_o, out_layout=KT, tile=tile)
    assert _same(kt_planes, K.repack_ktile(row_planes))
    w2 = _rand(dev, N2, N, 19, weight=True)
    s2, s2_inv = K.f16x3_row_scales(w2)
    b2 = K.split_f16x2(w2, 1.0, s2)
    want = K.gemm_nt_f16x3(row_planes, s_o, b2, s2_inv)
    got = K.gemm_nt_f16x3_layout(M, N2, N, _flat(kt_planes), s_o, _flat(K.repack_ktile(b2)), s2_inv, a_layout=KT, a_rows_total=M, b_layout=KT, b_rows_total=N2,
                                 out=_nan(dev, M, N2))
    assert _same(got, want)


@pytest.mark.parametrize("group", [32, 64])
@pytest.mark.parametrize("on_load", [True, False], ids=["a-on-load", "a-planes"])
def test_group_max_form_with_kt_weight(dev, group, on_load):
    import act_amd.kernels as K
    M, N, Kd = 256, 128, 128
    g = torch.Generator().manual_seed(group)
    a, w = _rand(dev, M, Kd, 23), _rand(dev, N, Kd, 29, weight=True)
    sc, sh = (0.5 + torch.rand(Kd, generator=g)).to(dev), (0.1 * torch.randn(Kd, generator=g)).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    s_a = R.act_scale(float((a * sc + sh).clamp_min(0).abs().max().item()))
    sb, sb_inv = K.f16x3_row_scales(w)
    bp = K.split_f16x2(w, 1.0, sb)
    if on_load:
        kw = dict(col_scale=sc, col_shift=sh, bias=bias)
        x = a
    else:
        kw = dict(bias=bias)
        x = K.split_f16x2_affine_relu(a, sc, sh, s_a)
    want = K.gemm_nt_f16x3_gmax(x, s_a, bp, sb_inv, group, **kw)
    got = K.gemm_nt_f16x3_gmax(x, s_a, K.repack_ktile(bp), sb_inv, group, b_layout=KT, **kw)
    assert want.shape == (M // group, N) and _same(got, want)


# ---- the composites, ACT_X3_KT on against off ---------------------------------------------------------------------------------------------------------------
class _kt:
    """the run-time switch for the duration of a block"""
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        import act_amd.kernels as K
        self.saved = K.x3_kt(self.on)

    def __exit__(self, *a):
        import act_amd.kernels as K
        K.x3_kt(self.saved)


def test_the_switch_is_on_by_default_and_answers_its_previous_setting(dev):
    import act_amd.kernels as K
    assert K.x3_kt() is True
    assert K.x3_kt(False) is True and K.x3_kt() is False and K.x3_kt(True) is False and K.x3_kt() is True


def test_whole_teacher_is_the_same_bits_either_way(dev, monkeypatch):
    """the Stage-II teacher's geometry at B = 2 (TG = 128), as tests/test_gpu_f16x3.py: four KT weights per block, the hidden activation handed on KT"""
    import act_amd.composite as CP
    from act_amd.models import build_model_from_cfg
    from act_amd.utils.config import cfg_from_yaml_file
    from tests.golden.fill import clouds
    cfg = cfg_from_yaml_file("cfgs/pretrain/pretrain_act_distill.yaml").model
    cfg.dvae_config.ckpt = "none"
    torch.manual_seed(2)
    model = build_model_from_cfg(cfg).to(dev).train()
    tk = model.dvae_tokenizer
    tk.prompt_dropout.p = 0.0
    with torch.no_grad():
        _, c = model.group_divider(torch.from_numpy(clouds(6, 2, 1024)).to(dev))
    x = torch.randn(2, c.shape[1], tk.proj_pre.weight.shape[1], generator=torch.Generator().manual_seed(9)).to(dev)
    assert CP.TEACHER_F16X3 and not CP.TEACHER_BF16X3
    import act_amd.kernels as K

    def run(on):
        with torch.no_grad(), _kt(on):
            out = tk.visual_embedding(x, c)
            assert CP._VIT_F16[tk][0][-1] == (CP.X3_KT_VIT if on else 0)          # the cached planes are in the layout of the switch
            return out, [p.clone() for p in CP._VIT_F16[tk][1][:4]]
    off, planes_off = run(False)
    for mask in (CP.X3_KT_VIT, 0b1111, 0b0011):                   # as shipped; every Linear (qkv: its K,V rows too); the two that ship row-major
        monkeypatch.setattr(CP, "X3_KT_VIT", mask)
        on, planes_on = run(True)
        assert torch.isfinite(on).all() and torch.equal(on, off), mask
        for j, (a, b) in enumerate(zip(planes_on, planes_off)):   # qkv, proj, fc1, fc2 of block 0
            assert torch.equal(a, K.repack_ktile(b) if (mask >> j) & 1 else b) and torch.equal(a, b) != bool((mask >> j) & 1)
        assert torch.equal(run(False)[0], off)                    # and back


def test_mini_pointnet_is_the_same_bits_either_way(dev, monkeypatch):
    import act_amd.composite as CP
    from tests import test_gpu_pn_f16x3 as PN
    c = PN._pn(384, 8, 32)
    monkeypatch.setattr(CP, "X3_KT_PN", True)                     # (ships row-major: its gain stayed below the launch's spread, notebook/x3_ktile.md)
    with _kt(False):
        off = PN._native(c["enc"], c["pts"], x3=True)
    with _kt(True):
        on = PN._native(c["enc"], c["pts"], x3=True, edit=lambda s: _is(s.w_layout, KT))
    assert torch.equal(on, off) and not torch.equal(on, c["f32"])


def _is(a, b):
    assert a == b, (a, b)


@pytest.mark.parametrize("shape", [(2, 64, 4, 384, 8192), (2, 64, 4, 384, 384)], ids=["layers+head", "layers"])
def test_dgcnn_is_the_same_bits_either_way(dev, shape):
    from tests import test_gpu_dgcnn_edge_f16x3 as DE
    c = DE._case(shape)
    with _kt(False):
        off = DE._native(c["dg"], c["f"], c["idx"], "layers", edit=lambda s, T: _is(s.w_layout, ROW))
    with _kt(True):
        on = DE._native(c["dg"], c["f"], c["idx"], "layers", edit=lambda s, T: _is(s.w_layout, KT))
    assert torch.equal(on, off) and not torch.equal(on, c["h32"])
    if shape[4] >= 1024:
        with _kt(False):                                          # the head alone (cat split row-major in one pass): w5 row-major against w5 KT
            assert torch.equal(DE._native(c["dg"], c["f"], c["idx"], "head", edit=lambda s, T: _is(s.w_layout, ROW)), c["head"])


# ---- bad arguments: ACT_E_BADARG and nothing launched -------------------------------------------------------------------------------------------------------
def _raw(M, N, Kd, a, s_a, b, sb_inv, out, a_layout=ROW, lda=0, a_rows=0, b_layout=ROW, b_rows=0, planes_out=None, out_layout=ROW):
    from act_amd import _C
    from act_amd._abi import GemmEpilogue
    e = GemmEpilogue(alpha=1.0)
    o1, o2 = (_C.ptr(planes_out[0]), _C.ptr(planes_out[1])) if planes_out is not None else (None, None)
    return _C.lib.act_sgemm_nt_f16x3_planes_layout_f32(M, N, Kd, _C.ptr(a[0]), _C.ptr(a[1]), a_layout, lda, a_rows, float(s_a), _C.ptr(b[0]), _C.ptr(b[1]), b_layout,
                                                       b_rows, _C.ptr(sb_inv), _C.ptr(out), N, o1, o2, 64.0, out_layout, ctypes.byref(e), _C.stream(), 0)


def test_bad_layout_arguments_are_refused_before_any_launch(dev):
    import act_amd.kernels as K
    from act_amd import _C
    M, N, Kd = 128, 128, 64
    ap, s_a, bp, sb_inv = _operands(dev, M, N, Kd, 31)
    akt, bkt = K.repack_ktile(ap), K.repack_ktile(bp)
    out = _nan(dev, M, N)
    pl = _nan(dev, 2, M + 1, N, dtype=torch.float16)
    cases = {
        "b rows_total < N": dict(a=_flat(ap), b=_flat(bkt), b_layout=KT, b_rows=N - 1),
        "a rows_total < M": dict(a=_flat(akt), b=_flat(bp), a_layout=KT, a_rows=M - 1),
        "kt b base off its line": dict(a=_flat(ap), b=_flat(torch.cat([bkt, bkt], 1), 8), b_layout=KT, b_rows=2 * N),
        "kt a base off its line": dict(a=_flat(torch.cat([akt, akt], 1), 32), b=_flat(bp), a_layout=KT, a_rows=2 * M),
        "unknown b layout": dict(a=_flat(ap), b=_flat(bp), b_layout=2, b_rows=N),
        "unknown a layout": dict(a=_flat(ap), b=_flat(bp), a_layout=-1, a_rows=M),
        "unknown out layout": dict(a=_flat(ap), b=_flat(bp), planes_out=pl, out_layout=2),
        "kt planes-out off their line": dict(a=_flat(ap), b=_flat(bp), planes_out=(pl[0].reshape(-1)[8:], pl[1].reshape(-1)[8:]), out_layout=KT),
        "negative lda": dict(a=_flat(ap), b=_flat(bp), lda=-8),
    }
    for name, kw in cases.items():
        a, b = kw.pop("a"), kw.pop("b")
        assert _raw(M, N, Kd, a, s_a, b, sb_inv, out, **kw) == BADARG, name
    assert _raw(M, N, Kd, _flat(akt), s_a, _flat(bkt), sb_inv, out, a_layout=KT, a_rows=M, b_layout=KT, b_rows=N) == 0       # the well-formed call goes through
    torch.cuda.synchronize()
    assert torch.isnan(pl.float()).all() and _same(out, K.gemm_nt_f16x3(ap, s_a, bp, sb_inv))
    # the group-max form
    gm = _nan(dev, M // 32, N)
    a32, sc = _rand(dev, M, Kd, 37), torch.ones(Kd, device=dev)
    gmax = lambda lay, rows, b: _C.lib.act_sgemm_nt_f16x3_gmax_layout_f32(M, N, Kd, _C.ptr(a32), Kd, _C.ptr(sc), _C.ptr(sc), None, None, 64.0, _C.ptr(b[0]), _C.ptr(b[1]),
                                                                         lay, rows, _C.ptr(sb_inv), None, 32, _C.ptr(gm), N, 0, _C.stream())
    assert gmax(KT, N - 1, _flat(bkt)) == BADARG and gmax(3, N, _flat(bkt)) == BADARG and gmax(KT, 2 * N, _flat(torch.cat([bkt, bkt], 1), 8)) == BADARG
    # the repack and the split
    src, dst = torch.zeros(64, 48, dtype=torch.int16, device=dev), _nan(dev, 64, 48, dtype=torch.float16)
    assert _C.lib.act_repack_ktile_u16(_C.ptr(src), _C.ptr(dst), 64, 48, _C.stream()) == BADARG                               # K % 32
    assert _C.lib.act_repack_ktile_u16(_C.ptr(src), _C.ptr(src), 64, 32, _C.stream()) == BADARG                               # in place
    x = _rand(dev, 64, 48, 41)
    assert _C.lib.act_split_f16x2_kt_f32(_C.ptr(x), 64, 48, 48, 1.0, _C.ptr(dst), _C.ptr(dst), 64, _C.stream()) == BADARG     # K % 32
    x = _rand(dev, 64, 64, 43)
    d2 = _nan(dev, 2, 64, 64, dtype=torch.float16)
    assert _C.lib.act_split_f16x2_kt_f32(_C.ptr(x), 64, 64, 64, 1.0, _C.ptr(d2[0]), _C.ptr(d2[1]), 63, _C.stream()) == BADARG  # rows_total < R
    torch.cuda.synchronize()
    assert torch.isnan(gm).all() and torch.isnan(dst.float()).all() and torch.isnan(d2.float()).all()
