"""The split-f16 GEMM's tile forms (csrc/gemm_bf16x3.hip): 128 x 128 on 2 x 2 waves and 128 x 192 on 2 x 4 waves.  The accumulation order of an output element
does not depend on the tile -- K tiles in sequence, the three plane products in the same order, the same epilogue -- so a forced 128 x 192 launch must give the
bits of a forced 128 x 128 launch, on every epilogue; the rule that picks the tile is a pure function of the shape and the CU count."""
import ctypes

import pytest
import torch

from tests import f16x3_ref as R

pytestmark = pytest.mark.gpu

BADARG = -1                                                       # ACT_E_BADARG (include/act_hip.h)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _operands(dev, M, N, Kd, seed):
    """random planes: activations at one static scale, weights at one power of two per row"""
    import act_amd.kernels as K
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, Kd, generator=g).to(dev)
    w = (0.05 * torch.randn(N, Kd, generator=g) * torch.exp(torch.randn(N, 1, generator=g))).to(dev)      # rows of different magnitude: different row scales
    s_a = R.act_scale(a.abs().max().item())
    sb, sb_inv = K.f16x3_row_scales(w)
    assert sb.unique().numel() > 1
    return K.split_f16x2(a, s_a), s_a, K.split_f16x2(w, 1.0, sb), sb_inv


def _product(ops, tile, bias=None, act=0, res=None, planes=False, want_c=True, out_scale=64.0):
    """one launch through the C entry that takes the tile -> (return code, C or None, planes or None); outputs start as NaN, so an element that a tile form
    does not write fails the comparison"""
    from act_amd import _C
    from act_amd._abi import GemmEpilogue
    ap, s_a, bp, sb_inv = ops
    (_, M, Kd), N = ap.shape, bp.shape[1]
    nan = float("nan")
    out = torch.full((M, N), nan, dtype=torch.float32, device=ap.device) if want_c else None
    pl = torch.full((2, M, N), nan, dtype=torch.float16, device=ap.device) if planes else None
    e = GemmEpilogue(alpha=1.0, act=act, accumulate=0, rows_per_scale=0, ldr=(res.stride(0) if res is not None else 0), ldaux=0, res_row_div=0,
                     bias=_C.ptr(bias), rowscale=None, res=_C.ptr(res), aux=None)
    rc = _C.lib.act_sgemm_nt_f16x3_planes_tile_f32(M, N, Kd, _C.ptr(ap[0]), _C.ptr(ap[1]), float(s_a), _C.ptr(bp[0]), _C.ptr(bp[1]), _C.ptr(sb_inv),
                                                   _C.ptr(out), N, _C.ptr(pl[0]) if planes else None, _C.ptr(pl[1]) if planes else None, float(out_scale),
                                                   ctypes.byref(e), _C.stream(), tile)
    return rc, out, pl


def _same(x, y):
    return not torch.isnan(x.float()).any().item() and torch.equal(x, y)


# (384, 768, 128): 12 / 18 workgroups, the XCD remap with a remainder; (1152, 384, 64): 9 row tiles, the grouped rasterisation's tail group of one row tile
@pytest.mark.parametrize("M,N,Kd", [(128, 384, 64), (256, 384, 192), (384, 768, 128), (1152, 384, 64), (128, 384, 3072)])
def test_the_128x192_tile_gives_the_bits_of_the_128x128_tile(dev, M, N, Kd):
    ops = _operands(dev, M, N, Kd, M + N + Kd)
    rc0, c128, _ = _product(ops, 128)
    rc1, c192, _ = _product(ops, 192)
    assert rc0 == 0 and rc1 == 0
    assert _same(c128, c192)
    rc2, crule, _ = _product(ops, 0)                              # whatever the rule takes
    assert rc2 == 0 and _same(crule, c128)


@pytest.mark.parametrize("case", ["bias", "bias+gelu", "bias+res", "gelu-planes-only", "res-offset-4-bytes"])
def test_epilogues_are_the_same_bits_on_both_tiles(dev, case):
    import act_amd.kernels as K
    M, N, Kd = 256, 384, 192
    ops = _operands(dev, M, N, Kd, 7)
    g = torch.Generator().manual_seed(len(case))
    bias = torch.randn(N, generator=g).to(dev)
    kw = dict(bias=bias)
    if "gelu" in case:
        kw["act"] = K.EPI_GELU
    if case == "bias+res":
        kw["res"] = torch.randn(M, N, generator=g).to(dev)
    if case == "res-offset-4-bytes":                              # a residual that is not 16-byte aligned: the scalar branch of the epilogue
        buf = torch.randn(M * N + 1, generator=g).to(dev)
        kw["res"] = buf[1:].view(M, N)
        assert kw["res"].data_ptr() % 16 == 4 and kw["res"].is_contiguous()
    if case == "gelu-planes-only":                                # C = NULL: the result leaves as planes alone
        kw.update(planes=True, want_c=False)
    rc0, c128, p128 = _product(ops, 128, **kw)
    rc1, c192, p192 = _product(ops, 192, **kw)
    assert rc0 == 0 and rc1 == 0
    if case == "gelu-planes-only":
        assert c128 is None and _same(p128, p192)
        _, c, p = _product(ops, 128, planes=True, bias=bias, act=K.EPI_GELU)          # ... and they are the planes of the fp32 result
        assert _same(p, p128) and torch.equal(p, K.split_f16x2(c, 64.0))
    else:
        assert _same(c128, c192)
        assert not torch.equal(c128, _product(ops, 128)[1])       # the epilogue was applied


def test_a_forced_tile_that_the_shape_does_not_take_is_refused(dev):
    ops = _operands(dev, 128, 256, 64, 3)
    assert _product(ops, 192)[0] == BADARG                        # 256 is no multiple of 192
    assert _product(ops, 64)[0] == BADARG and _product(ops, -1)[0] == BADARG
    rc, c128, _ = _product(ops, 128)
    rc0, crule, _ = _product(ops, 0)
    assert rc == 0 and rc0 == 0 and _same(crule, c128)


def test_the_rule_keeps_128x128_where_192_does_not_divide(dev):
    """N = 8192 (the tokenizer head's width, 8192 % 192 != 0) at a small M"""
    ops = _operands(dev, 128, 8192, 64, 4)
    assert _product(ops, 192)[0] == BADARG
    rc, c128, _ = _product(ops, 128)
    rc0, crule, _ = _product(ops, 0)
    assert rc == 0 and rc0 == 0 and _same(crule, c128)


RULE = [((8192, 768, 768), 192), ((8192, 768, 3072), 192),                                          # the teacher's proj and fc2 at B = 128: 384 workgroups
        ((2048, 2304, 768), 192), ((6144, 768, 3072), 192),                                         # 288 workgroups of 128 x 128: more than one per CU
        ((8192, 3072, 768), 128), ((8192, 8192, 2304), 128), ((128, 384, 64), 128),                 # fc1 (a tie), the head (192 does not divide), a grid of 3
        ((8192, 2304, 768), 128),                                                                   # qkv: 5 units against 4.5, not an eighth cheaper
        ((4096, 768, 768), 128), ((16384, 768, 3072), 128), ((16384, 2304, 768), 128)]              # one workgroup per CU; the stress geometry's fc2 and qkv (ties)


def test_the_rule_on_the_bench_shapes(dev):
    """The measured rule: isolated per-launch times of both tiles on these shapes in profiles/x3_tiles_micro.txt, in-step times of the B = 128 teacher shapes in
    profiles/x3_tiles_trace_by_grid_{parent,change,qkv192}.txt.  Two shapes were expected to take 128 x 192 and do not.  (16384, 768, 3072), 768 against 512
    workgroups, two rounds of 2 against two of 1.5: measured 257.3 us on 128 x 128 and 265.7 us on 128 x 192 -- the last 256 of the 768 workgroups have a CU
    each and finish sooner, so the rule counts such a last round as 1 and the shape is a tie.  (8192, 2304, 768), 5 units against 4.5: 138.2 against 131.7 us
    alone, but 132.7 against 135.4 us per launch inside the serialised step, so the rule asks for an eighth."""
    from act_amd import _C
    pick = _C.lib.act_sgemm_nt_f16x3_pick_tile
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    for shape, want in RULE:
        assert pick(*shape, 256) == want, shape
        assert pick(*shape, cus) == want, (shape, cus)           # the device's own count instead of the literal
    assert pick(8192, 768, 768, 0) == 0 and pick(100, 384, 64, 256) == 0 and pick(128, 384, 32, 256) == 0             # no CUs, unsupported shapes
    assert pick(128, 256, 64, 256) == 128
