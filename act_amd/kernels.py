"""Host-side plumbing over the C ABI: raw launch wrappers + the autograd Functions the model mirror uses.

Nothing here computes on the host: every function allocates outputs with torch (device memory, caching
allocator) and launches kernels of libact_hip.so on the current HIP stream.
"""
import ctypes
import os

import numpy as np

import torch

from . import _C
from ._abi import GemmEpilogue, GemmTnProblem          # (declared with the rest of the C ABI; built here and by tests / benchmarks as K.*)

EPI_NONE, EPI_GELU, EPI_RELU, EPI_MUL_GELU_GRAD, EPI_MUL_RELU_MASK = 0, 1, 2, 3, 4

lib, ptr, stream, check = _C.lib, _C.ptr, _C.stream, _C.check

# ---- persistent scratch (split-K partials, LN / colsum partial rows): one buffer per device and stream ----------
_WS = {}
_WS_BYTES = 160 << 20       # split-K / grouped-GEMM partials: 7 K ranges of the two d=768 MLP weight gradients need 132 MB (round 3; 64 MB before)


def workspace(device, nbytes=_WS_BYTES, stream_handle=None):
    """scratch buffer of one stream on ``device`` -- the CURRENT one unless a raw handle is given (kernels of different streams may run concurrently)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, _C.stream_handle(idx) if stream_handle is None else stream_handle)
    w = _WS.get(key)
    if w is None or w.numel() * 4 < nbytes:
        w = torch.empty(max(nbytes, _WS_BYTES) // 4, dtype=torch.float32, device=device)
        _WS[key] = w
    return w


_SIDE = {}


def side_stream(device, which=0):
    """auxiliary HIP streams per device for work that is independent of the main chain: 0 = frozen teacher forward (may run a
    whole step ahead), 1 = weight-gradient GEMMs of the student's backward (forked and joined inside one block's backward)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), which)
    st = _SIDE.get(key)
    if st is None:
        prio = int(os.environ.get("ACT_SIDE_PRIO%d" % which, "0"))      # experiment knob: hipStream priority of the auxiliary streams
        st = _SIDE[key] = torch.cuda.Stream(device=device, priority=prio)
    return st


OVERLAP_DW = os.environ.get("ACT_OVERLAP_DW", "1") != "0"
LINEAR_OVERLAP_DW = os.environ.get("ACT_LINEAR_OVERLAP_DW", "0") == "1"     # LinearFn.backward: dW / db on the auxiliary stream (measured per workload; see DESIGN)
GROUPED_DW = os.environ.get("ACT_GROUPED_DW", "1") != "0"      # weight + bias gradients of two Linears per launch (0: one GEMM + column sum each)


class fork_side:
    """``with fork_side(dev):`` enqueues the body on the auxiliary stream, ordered after everything already enqueued on the
    current stream.  Used for weight-gradient GEMMs / bias column sums, which nothing in the rest of the backward chain reads:
    they then share the chip with the (small, latency-bound) dX GEMMs of the student instead of running back to back."""

    def __init__(self, device):
        self.main, self.side = torch.cuda.current_stream(device), side_stream(device, 1)

    def __enter__(self):
        self.side.wait_stream(self.main)
        self.ctx = torch.cuda.stream(self.side)
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)


def join_side(device, *tensors):
    """the current stream waits for the auxiliary stream; ``tensors`` (allocated there) are handed over to the current stream."""
    main = torch.cuda.current_stream(device)
    main.wait_stream(side_stream(device, 1))
    for t in tensors:
        if t is not None:
            t.record_stream(main)


def _f32c(t, name="tensor"):
    if t.dtype != torch.float32:
        raise _C.ActHipError(f"{name}: expected float32")
    return t if t.is_contiguous() else t.contiguous()


def _f32rows(t, name="tensor"):
    """2-D operand with unit inner stride (row-strided views such as column slices of a weight are passed as is: the GEMM
    takes a leading dimension)."""
    if t.dtype != torch.float32:
        raise _C.ActHipError(f"{name}: expected float32")
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1] and (
            t.is_contiguous() or (t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0)):
        return t                              # strided views must keep the float4 path of the tuned kernels available
    return t.contiguous()


# ---- raw wrappers ---------------------------------------------------------------------------------------
def gemm(a, b, a_kmajor=True, b_kmajor=True, bias=None, act=EPI_NONE, aux=None, res=None, rowscale=None,
         rows_per_scale=0, out=None, accumulate=False, alpha=1.0, res_row_div=0, cfg=None):
    """C[M,N] = epilogue(op(a) @ op(b)); a: [M,K] if a_kmajor else [K,M]; b: [N,K] if b_kmajor else [K,N]."""
    a = _f32rows(a, "a"); b = _f32rows(b, "b")
    if a_kmajor:
        M, K = a.shape
    else:
        K, M = a.shape
    if b_kmajor:
        N, Kb = b.shape
    else:
        Kb, N = b.shape
    if K != Kb:
        raise _C.ActHipError(f"gemm: inner dimensions differ ({K} vs {Kb})")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    e = GemmEpilogue(alpha=alpha, act=act, accumulate=int(accumulate), rows_per_scale=int(rows_per_scale),
                     ldr=(res.stride(0) if res is not None else 0), ldaux=(aux.stride(0) if aux is not None else 0),
                     res_row_div=int(res_row_div), bias=ptr(bias), rowscale=ptr(rowscale), res=ptr(res), aux=ptr(aux))
    ws = workspace(a.device)
    if cfg is None:
        cfg = gemm_config(a_kmajor, b_kmajor, M, N, K, a.device, a, b, ws)
    tile, splits = cfg if cfg is not None else (0, 0)         # undecided during stream capture: the cost model now, the decision on a later eager call
    check(lib.act_sgemm_ex_f32(int(a_kmajor), int(b_kmajor), M, N, K, _C.ptr_rows(a), a.stride(0), _C.ptr_rows(b), b.stride(0), ptr(out),
                               out.stride(0), ctypes.byref(e), ptr(ws), ws.numel() * 4, tile, splits, stream()), "act_sgemm_f32")
    return out


def gemm_tn_grouped(pairs, want_bias=True, splits=0):
    """[(dy [T,M], x [T,N]), ...] -> ([dW_p = dy_p^T . x_p  [M,N]], [db_p = column sums of dy_p  [M]]) in ONE launch (+ one reduction launch
    for the K ranges): the weight / bias gradients of several Linears that share the token dimension (csrc/gemm_grouped.hip).
    splits <= 0: the library's count, capped by the shared workspace (_WS_BYTES) exactly as the composite block backward caps it, so the
    per-kernel and the composite host paths fold the same K ranges in the same order (bit-identical) for any model width."""
    if not pairs or len(pairs) > 8:
        raise _C.ActHipError(f"gemm_tn_grouped: 1..8 problems per launch, got {len(pairs)}")
    pairs = [(_f32rows(dy, "dy"), _f32rows(x, "x")) for dy, x in pairs]      # fp32, unit inner stride, float4-able rows (else a contiguous copy)
    T = pairs[0][0].shape[0]
    dev = pairs[0][0].device
    probs = (GemmTnProblem * len(pairs))()
    dws, dbs = [], []
    for i, (dy, x) in enumerate(pairs):
        if dy.dim() != 2 or x.dim() != 2 or dy.shape[0] != T or x.shape[0] != T:
            raise _C.ActHipError("gemm_tn_grouped: every operand needs the same number of rows")
        M, N = dy.shape[1], x.shape[1]
        dw = torch.empty(M, N, dtype=torch.float32, device=dev)
        db = torch.empty(M, dtype=torch.float32, device=dev) if want_bias else None
        dws.append(dw); dbs.append(db)
        probs[i] = GemmTnProblem(_C.ptr_rows(dy).value, dy.stride(0), _C.ptr_rows(x).value, x.stride(0), dw.data_ptr(), N, M, N,
                                 db.data_ptr() if db is not None else None)
    ws = workspace(dev)
    if splits <= 0:
        splits = lib.act_sgemm_tn_grouped_splits(probs, len(pairs), T)
        while splits > 1 and lib.act_sgemm_tn_grouped_workspace(probs, len(pairs), T, splits) > ws.numel() * 4:
            splits -= 1
    else:
        ws = workspace(dev, lib.act_sgemm_tn_grouped_workspace(probs, len(pairs), T, splits))      # an explicit count gets the space it needs
    check(lib.act_sgemm_tn_grouped_f32(probs, len(pairs), T, splits, ptr(ws), ws.numel() * 4, stream()), "act_sgemm_tn_grouped_f32")
    return dws, dbs


# ---- OPT-IN split-bf16 products (csrc/gemm_bf16x3.hip): frozen teacher only, never the default -------------------------------------------------
def split_bf16x2(x, out=None):
    """fp32 [R, K] -> bf16 planes [2, R, K]: hi = bf16(x), lo = bf16(x - hi) (round to nearest even) -- the operand form of gemm_nt_bf16x3."""
    x = _f32rows(x, "x")
    R, Kd = x.shape
    if out is None:
        out = torch.empty(2, R, Kd, dtype=torch.bfloat16, device=x.device)
    check(lib.act_split_bf16x2_f32(_C.ptr_rows(x), R, Kd, x.stride(0), ptr(out[0]), ptr(out[1]), stream()), "act_split_bf16x2_f32")
    return out


def layernorm_planes(x, gamma, beta, eps, pos=None):
    """LN(x + pos) * gamma + beta written as (hi, lo) bf16 planes [2, T, D] (bit-identical to split_bf16x2(layernorm_fwd(...)))"""
    x = _f32c(x)
    T, D = x.shape
    planes = torch.empty(2, T, D, dtype=torch.bfloat16, device=x.device)
    check(lib.act_layernorm_fwd_planes_f32(ptr(x), ptr(_f32c(pos)) if pos is not None else None, ptr(gamma), ptr(beta), None, None, ptr(planes[0]), ptr(planes[1]),
                                           None, None, T, D, float(eps), stream()), "act_layernorm_fwd_planes_f32")
    return planes


def _x3_problem(name, dtype, a_planes, b_planes, bias, act, res, out, planes_out):
    """what gemm_nt_bf16x3 and gemm_nt_f16x3 share: the plane, shape and ``planes_out`` checks, the result tensor and the epilogue struct
    -> (M, N, K, the operand pointers a1, a2, b1, b2, out, the planes_out pointers o1, o2 (None, None without), epilogue)"""
    fmt = "bf16" if dtype == torch.bfloat16 else "f16"
    _, M, Kd = a_planes.shape
    _, N, Kb = b_planes.shape
    if Kd != Kb or a_planes.dtype != dtype or b_planes.dtype != dtype or not (a_planes.is_contiguous() and b_planes.is_contiguous()):
        raise _C.ActHipError(f"{name}: contiguous {fmt} planes [2, rows, K] with equal K expected")
    if not lib.act_sgemm_nt_bf16x3_supported(M, N, Kd):      # (act_sgemm_nt_f16x3_supported is the same predicate)
        raise _C.ActHipError(f"{name}: unsupported shape {M} x {N} x {Kd} (M, N % 128, K % 64)")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a_planes.device)
    e = GemmEpilogue(alpha=1.0, act=act, accumulate=0, rows_per_scale=0, ldr=(res.stride(0) if res is not None else 0), ldaux=0, res_row_div=0,
                     bias=ptr(bias), rowscale=None, res=ptr(res), aux=None)
    o1, o2 = (None, None)
    if planes_out is not None:                               # the result also as planes [2, M, N] -- the A operand of a following product
        if planes_out.dtype != dtype or tuple(planes_out.shape) != (2, M, N) or not planes_out.is_contiguous():
            raise _C.ActHipError(f"{name}: planes_out must be a contiguous {fmt} tensor [2, M, N]")
        o1, o2 = ptr(planes_out[0]), ptr(planes_out[1])
    return M, N, Kd, ptr(a_planes[0]), ptr(a_planes[1]), ptr(b_planes[0]), ptr(b_planes[1]), out, o1, o2, e


def gemm_nt_bf16x3(a_planes, b_planes, bias=None, act=EPI_NONE, res=None, out=None, planes_out=None):
    """C[M,N] = epilogue(a . b^T) with both operands given as (hi, lo) bf16 planes [2, rows, K] (split_bf16x2) and the three products hi.hi + hi.lo + lo.hi
    on the bf16 matrix cores (fp32 accumulation): 4e-6 relative per product.  M, N % 128 == 0, K % 64 == 0.  Opt-in path of the frozen teacher."""
    M, N, Kd, a1, a2, b1, b2, out, o1, o2, e = _x3_problem("gemm_nt_bf16x3", torch.bfloat16, a_planes, b_planes, bias, act, res, out, planes_out)
    if planes_out is not None:
        check(lib.act_sgemm_nt_bf16x3_planes_f32(M, N, Kd, a1, a2, b1, b2, ptr(out), out.stride(0), o1, o2, ctypes.byref(e), stream()),
              "act_sgemm_nt_bf16x3_planes_f32")
    else:
        check(lib.act_sgemm_nt_bf16x3_f32(M, N, Kd, a1, a2, b1, b2, ptr(out), out.stride(0), ctypes.byref(e), stream()), "act_sgemm_nt_bf16x3_f32")
    return out


# ---- split-f16 products (same file, F16 form): the DEFAULT arithmetic of the frozen teacher's four Linear products per layer ------------------------
def f16x3_row_scales(w):
    """one power of two per row of w [N, K] that lifts the row's largest magnitude into [2^14, 2^15) (1 for an all-zero row) -> (scale [N], 1 / scale [N])"""
    mx = w.detach().abs().amax(dim=1).float()
    e = torch.frexp(mx).exponent                                              # max = m * 2^e, m in [0.5, 1)
    e = torch.where(mx > 0, e, torch.full_like(e, 15))
    one = torch.ones(e.shape, dtype=torch.float32, device=w.device)
    return torch.ldexp(one, 15 - e), torch.ldexp(one, e - 15)


def split_f16x2(x, scale=1.0, row_scale=None, out=None):
    """fp32 [R, K] -> f16 planes [2, R, K] of xs = x * scale * row_scale[row] (powers of two): h1 = f16(xs), h2 = f16((xs - h1) * 2^11), round to nearest
    even, a plane element below 2^-14 written as +0 before the residual is taken (csrc/split_planes.h; tests/f16x3_ref.py restates it)."""
    x = _f32rows(x, "x")
    R, Kd = x.shape
    if out is None:
        out = torch.empty(2, R, Kd, dtype=torch.float16, device=x.device)
    check(lib.act_split_f16x2_f32(_C.ptr_rows(x), R, Kd, x.stride(0), float(scale), ptr(_f32c(row_scale)) if row_scale is not None else None,
                                  ptr(out[0]), ptr(out[1]), stream()), "act_split_f16x2_f32")
    return out


def layernorm_f16_planes(x, gamma, beta, eps, scale, pos=None):
    """LN(x + pos) * gamma + beta written as f16 planes [2, T, D] at ``scale`` (bit-identical to split_f16x2(layernorm_fwd(...), scale))"""
    x = _f32c(x)
    T, D = x.shape
    planes = torch.empty(2, T, D, dtype=torch.float16, device=x.device)
    check(lib.act_layernorm_fwd_f16_planes_f32(ptr(x), ptr(_f32c(pos)) if pos is not None else None, ptr(gamma), ptr(beta), None, None, ptr(planes[0]),
                                               ptr(planes[1]), float(scale), None, None, T, D, float(eps), stream()), "act_layernorm_fwd_f16_planes_f32")
    return planes


def gemm_nt_f16x3(a_planes, a_scale, b_planes, b_inv_scale, bias=None, act=EPI_NONE, res=None, out=None, planes_out=None, out_scale=1.0, tile=0):
    """C[M,N] = epilogue((a . b^T) / a_scale / b_scale[n]) with both operands as f16 planes [2, rows, K] (split_f16x2: a at the scalar ``a_scale``, b at
    f16x3_row_scales) and the products h1.h1 + 2^-11 (h1.h2 + h2.h1) on the f16 matrix cores, two fp32 accumulators: fp32-grade.  M, N % 128 == 0,
    K % 64 == 0.  ``planes_out`` [2, M, N] f16: the result also as planes at ``out_scale`` -- the A operand of a following product.  ``tile``: 0 = the
    library's rule (act_sgemm_nt_f16x3_pick_tile), 128 or 192 = that column width of the tile (tests and A/B runs; the bits do not depend on it)."""
    M, N, Kd, a1, a2, b1, b2, out, o1, o2, e = _x3_problem("gemm_nt_f16x3", torch.float16, a_planes, b_planes, bias, act, res, out, planes_out)
    b_inv_scale = _f32c(b_inv_scale)
    if b_inv_scale.numel() != N:
        raise _C.ActHipError("gemm_nt_f16x3: b_inv_scale must hold one value per row of b")
    check(lib.act_sgemm_nt_f16x3_planes_tile_f32(M, N, Kd, a1, a2, float(a_scale), b1, b2, ptr(b_inv_scale), ptr(out), out.stride(0), o1, o2, float(out_scale),
                                                 ctypes.byref(e), stream(), int(tile)), "act_sgemm_nt_f16x3_planes_tile_f32")
    return out


def split_f16x2_affine_relu(x, col_scale, col_shift, scale):
    """fp32 [R, K] -> f16 planes [2, R, K] of relu(x * col_scale[k] + col_shift[k]) * scale, the power of two folded into the affine map first: the pass form of
    what gemm_nt_f16x3_gmax does on load (test helper and speed baseline; the product path splits on load)"""
    x = _f32rows(x, "x")
    R, Kd = x.shape
    out = torch.empty(2, R, Kd, dtype=torch.float16, device=x.device)
    check(lib.act_split_f16x2_affine_relu_f32(_C.ptr_rows(x), R, Kd, x.stride(0), ptr(_f32c(col_scale)), ptr(_f32c(col_shift)), float(scale), ptr(out[0]),
                                              ptr(out[1]), stream()), "act_split_f16x2_affine_relu_f32")
    return out


def gemm_nt_f16x3_gmax(a, a_scale, b_planes, b_inv_scale, group, bias=None, col_scale=None, col_shift=None, tile=0, b_layout=0):
    """out[M / group, N] = max over every ``group`` (32 | 64) consecutive rows of ((a' . b^T) / a_scale / b_scale[n] + bias): the last product of the frozen
    tokenizer's mini-PointNet on the split-f16 kernel, nothing but the group max stored.  ``a`` fp32 [M, K] with col_scale / col_shift: a' = the planes of
    relu(a * col_scale + col_shift) * a_scale, formed while the kernel stages a; ``a`` f16 planes [2, M, K]: a' = those planes.  K <= 512.
    ``b_layout`` X3_KTILE: the two planes of b are K-tile-major (repack_ktile)."""
    planes = a.dtype == torch.float16
    b_planes, b_inv_scale = b_planes.contiguous(), _f32c(b_inv_scale)
    N, Kd = b_planes.shape[1], b_planes.shape[2]
    if planes:
        a = a.contiguous()
        M = a.shape[1]
        args = (None, 0, None, None, ptr(a[0]), ptr(a[1]))
    else:
        a = _f32rows(a, "a")
        M = a.shape[0]
        args = (_C.ptr_rows(a), a.stride(0), ptr(_f32c(col_scale)), ptr(_f32c(col_shift)), None, None)
    if a.shape[-1] != Kd or b_inv_scale.numel() != N or M % int(group):
        raise _C.ActHipError("gemm_nt_f16x3_gmax: shapes do not match")
    out = torch.empty(M // int(group), N, dtype=torch.float32, device=a.device)
    check(lib.act_sgemm_nt_f16x3_gmax_layout_f32(M, N, Kd, *args, float(a_scale), ptr(b_planes[0]), ptr(b_planes[1]), int(b_layout), N, ptr(b_inv_scale),
                                                 ptr(_f32c(bias)) if bias is not None else None, int(group), ptr(out), N, int(tile), stream()),
          "act_sgemm_nt_f16x3_gmax_layout_f32")
    return out


# ---- K-tile-major planes (csrc/gemm_bf16x3.hip, notebook/x3_ktile.md): the layout frozen weight planes are kept in ---------------------------------------
X3_ROWMAJOR, X3_KTILE = 0, 1
X3_BK = 32                     # elements per K tile


def ktile_index(r, k, rows_total):
    """where element (r, k) of a plane [rows_total][K] lies in the K-tile-major layout: the 64-byte pieces of all rows of one K tile side by side"""
    return ((k // X3_BK) * rows_total + r) * X3_BK + k % X3_BK


def ktile_rows(kt, R, Kd):
    """the row-major [R, K] reading of one K-tile-major plane (a view-and-copy on the host side of tests and tools)"""
    return kt.reshape(Kd // X3_BK, R, X3_BK).permute(1, 0, 2).reshape(R, Kd)


def x3_kt(on=None):
    """ACT_X3_KT (default on): frozen weight planes are kept K-tile-major and the composites hand activation planes on that way.  ``on`` None: query;
    else set -> the previous setting.  Off is the row-major step, the same bits."""
    return bool(lib.act_x3_kt(-1 if on is None else int(bool(on))))


def repack_ktile(planes):
    """16-bit planes [..., R, K] (contiguous, K % 32 == 0) -> a tensor of the same shape and dtype whose every [R, K] plane holds the K-tile-major layout"""
    planes = planes.contiguous()
    R, Kd = planes.shape[-2:]
    if planes.element_size() != 2 or Kd % X3_BK:
        raise _C.ActHipError("repack_ktile: 16-bit planes with K % 32 == 0 expected")
    out = torch.empty_like(planes)
    src, dst = planes.reshape(-1, R, Kd), out.view(-1, R, Kd)
    for i in range(src.shape[0]):
        check(lib.act_repack_ktile_u16(ptr(src[i]), ptr(dst[i]), R, Kd, stream()), "act_repack_ktile_u16")
    return out


def split_f16x2_kt(x, scale=1.0, out=None, rows_total=None):
    """split_f16x2 (no row scales) whose planes [2, rows_total, K] leave K-tile-major; x fills rows 0 .. R of them (rows_total None: R)"""
    x = _f32rows(x, "x")
    R, Kd = x.shape
    rows_total = R if rows_total is None else int(rows_total)
    if out is None:
        out = torch.empty(2, rows_total, Kd, dtype=torch.float16, device=x.device)
    check(lib.act_split_f16x2_kt_f32(_C.ptr_rows(x), R, Kd, x.stride(0), float(scale), ptr(out[0]), ptr(out[1]), rows_total, stream()), "act_split_f16x2_kt_f32")
    return out


def gemm_nt_f16x3_layout(M, N, Kd, a, a_scale, b, b_inv_scale, a_layout=0, lda=0, a_rows_total=0, b_layout=0, b_rows_total=0, bias=None, act=EPI_NONE,
                         res=None, out=None, want_c=True, planes_out=None, out_scale=1.0, out_layout=0, tile=0):
    """gemm_nt_f16x3 with the layout of each operand and of the planes-out given (act_sgemm_nt_f16x3_planes_layout_f32).  ``a`` / ``b``: a pair of f16
    tensors whose first elements are the operand's first element in its (h1, h2) planes -- a slice of a wider or K-tile-major buffer starts where the caller
    says.  X3_KTILE: the operand is rows and K tiles of the K-tile-major planes of a [rows_total][..] matrix.  ``want_c`` False: only ``planes_out`` leaves."""
    b_inv_scale = _f32c(b_inv_scale)
    if want_c and out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a[0].device)
    e = GemmEpilogue(alpha=1.0, act=act, accumulate=0, rows_per_scale=0, ldr=(res.stride(0) if res is not None else 0), ldaux=0, res_row_div=0,
                     bias=ptr(bias), rowscale=None, res=ptr(res), aux=None)
    o1, o2 = (ptr(planes_out[0]), ptr(planes_out[1])) if planes_out is not None else (None, None)
    check(lib.act_sgemm_nt_f16x3_planes_layout_f32(M, N, Kd, ptr(a[0]), ptr(a[1]), int(a_layout), int(lda), int(a_rows_total), float(a_scale), ptr(b[0]), ptr(b[1]),
                                                   int(b_layout), int(b_rows_total), ptr(b_inv_scale), ptr(out) if want_c else None,
                                                   out.stride(0) if want_c else N, o1, o2, float(out_scale), int(out_layout), ctypes.byref(e), stream(),
                                                   int(tile)), "act_sgemm_nt_f16x3_planes_layout_f32")
    return out if want_c else planes_out


# ---- GEMM autotuner: the step has ~40 distinct (layout, M, N, K) shapes; each is timed once (tile shape x split-K) on first
# use -- i.e. during the warm-up steps -- and the winner is cached, so steady-state steps never synchronise.
_GEMM_CACHE = {}
AUTOTUNE = os.environ.get("ACT_GEMM_AUTOTUNE", "1") != "0"
# ACT_GEMM_AUTOTUNE=1 (default): an unlisted shape is timed on first use over candidates that are BIT-IDENTICAL to each other (stable_candidates:
# one tile family, one deterministic split-K), so which of them the stopwatch prefers never changes a result bit.  "full": every tile family x split-K
# (a different split-K is a different fp32 summation order: results may differ in the last bits between runs) -- what benchmarks/tune_table.py
# uses to BUILD the shipped table, whose entries are then fixed.  "0": shipped table + built-in cost model only.
AUTOTUNE_FULL = os.environ.get("ACT_GEMM_AUTOTUNE", "1") == "full"
# Shipped winners for the shapes of the benchmarked workloads (measured on one MI355X by this same autotuner and dumped with
# ACT_GEMM_TUNE_SAVE=<file>): first use of a listed shape costs nothing; unlisted shapes are still tuned on first use.
_TUNE_FILE = os.environ.get("ACT_GEMM_TUNE_FILE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_tune_gfx950.json")
_GEMM_TABLE = {}
_MAX_SPLIT = int(os.environ.get("ACT_GEMM_MAX_SPLIT", "0"))              # experiment knob: cap split-K (table entries above the cap are re-tuned on first use)
if os.environ.get("ACT_GEMM_TUNE_TABLE", "1") != "0" and os.path.exists(_TUNE_FILE):
    import json as _json
    with open(_TUNE_FILE) as _fh:
        _GEMM_TABLE = {tuple(int(v) for v in k.split(",")): tuple(c) for k, c in _json.load(_fh)["configs"].items()}
    if _MAX_SPLIT > 0:
        _GEMM_TABLE = {k: c for k, c in _GEMM_TABLE.items() if c[1] <= _MAX_SPLIT or k[4] > 8192}
_NEW_TUNED = {}
if os.environ.get("ACT_GEMM_TUNE_SAVE"):
    import atexit as _atexit

    def _dump_tuned(path=os.environ["ACT_GEMM_TUNE_SAVE"].replace("%p", str(os.getpid()))):      # "%p" -> pid: one file per process of a test session
        import json
        merged = dict(_GEMM_TABLE); merged.update(_NEW_TUNED)
        with open(path, "w") as f:
            json.dump({"arch": "gfx950", "key": "a_kmajor,b_kmajor,M,N,K", "value": "[tile id, split-K]",
                       "configs": {",".join(str(v) for v in k): list(c) for k, c in sorted(merged.items())}}, f, indent=0)
    _atexit.register(_dump_tuned)


def stable_split(M, N, K, ws_bytes):
    """split-K of the first-use tuner: a function of the shape only.  No split while the 64 x 64 tile grid alone gives every CU work or K is short;
    else about two workgroups per CU, K ranges of >= 256, at most 8 ranges, partial sums within the workspace."""
    nb = -(-M // 64) * -(-N // 64)
    if nb >= 384 or K < 1024:
        return 1
    s = max(1, min(8, K // 256, int(round(512.0 / nb))))
    while s > 1 and s * M * N * 4 > ws_bytes:
        s -= 1
    return s


_TILE_BN = {}


def tile_bn(tile):
    """BN of a tile id, from the library's tile table (csrc/gemm.hip through act_gemm_tile_info); read once"""
    if not _TILE_BN:
        bn = ctypes.c_int()
        for t in range(1, 64):
            if lib.act_gemm_tile_info(t, None, ctypes.byref(bn), None, None) == 0:
                _TILE_BN[t] = bn.value
    return _TILE_BN[tile]


def stable_candidates(a, b, ak, bk, M, N, K, ws):
    """(tile id, split-K) configurations of ONE tile family at ONE deterministic split-K: every candidate adds the same fp32 products in the same order
    per output element (tests/test_gpu_dense.py: tiles 30 / 31 / 32 / 10 / 11 / 12 / 20 / 21 for NT, the quad-fragment tiles 13..16 for NN), so the
    timing-based choice between them cannot change a bit of the result.  [] = no fast family applies: built-in cost model, no timing at all."""
    aligned = ((a.data_ptr() | b.data_ptr()) & 15) == 0 and a.stride(0) % 4 == 0 and b.stride(0) % 4 == 0
    if not aligned or K % 32 != 0:
        return []
    sp = stable_split(M, N, K, ws.numel() * 4)             # (the library rounds the K range up to a multiple of 32 and recounts the ranges: same for every tile)
    if ak and bk:                                             # NT: hand-scheduled loop first, compiler loop as the alternative; M tails allowed
        return [(t, sp) for t in (30, 31, 32, 10, 11, 12) if N % tile_bn(t) == 0]
    if ak and not bk:                                         # NN: quad-fragment tiles, hand-scheduled loop first
        return [(t, sp) for t in (33, 34, 36, 35, 13, 14, 16, 15) if N % tile_bn(t) == 0]
    if not ak and not bk and M % 128 == 0 and N % 128 == 0:   # TN: the quad-fragment tile, hand-scheduled or compiler-scheduled
        return [(33, sp), (13, sp)]
    return []


def first_use_config(a, b, ak, bk, M, N, K, ws):
    """the launch configuration of a shape that is in no table: (tile id, split-K)"""
    if AUTOTUNE_FULL:
        return gemm_tune(a, b, ak, bk, M, N, K, ws)[0]
    cands = stable_candidates(a, b, ak, bk, M, N, K, ws)
    if not cands:
        return 0, 0
    if len(cands) == 1:
        return cands[0]
    best, t = gemm_tune(a, b, ak, bk, M, N, K, ws, cands=cands)
    return best if t < float("inf") else (0, 0)


def gemm_candidates(ak, bk, M, N, K, ws_bytes, max_split=0):
    """every (tile id, split-K) configuration gemm_tune tries for this product, in trial order (a tie in the timing goes to the earlier one).
    A function of these integers only: no tensor, no device (tests/test_gemm_candidates.py pins the lists).
    ws_bytes bounds the split-K partial sums; max_split > 0 caps split-K where K <= 8192 (ACT_GEMM_MAX_SPLIT)."""
    k32 = K % 32 == 0

    def fits(s):
        return s * M * N * 4 <= ws_bytes

    def capped(sp):
        return [s for s in sp if s <= max_split] if max_split > 0 and K <= 8192 else sp

    def quad_splits(nbq):
        """split-K counts of a quad-fragment tile whose grid has nbq workgroups"""
        sp = [1]
        if K >= 1024 and nbq < 2048:
            sp += [s for s in (2, 3, 4, 6, 8, 12, 16, 24, 32) if K // s >= 256 and fits(s) and nbq * s <= 8192]
        if K >= 65536 and nbq <= 64:                                  # weight gradients over a few hundred thousand rows on a handful of tiles
            sp += [s for s in (48, 64, 96, 128, 192, 256) if fits(s) and nbq * s <= 1024]
        if K >= 512 and nbq < 128:                                    # a handful of tiles: K ranges down to 128 rows, up to one round of 512 workgroups
            sp += [s for s in (5, 7, 9, 10, 12, 14, 16) if s not in sp and K // s >= 128 and fits(s) and nbq * s <= 512]
        return capped(sp)

    cands = []
    for tile, (bm, bn) in ((1, (128, 128)), (2, (128, 64)), (3, (64, 64))):
        nb = -(-M // bm) * -(-N // bn)
        if nb > 16384 and tile > 1:
            continue
        sp = [1]
        if K >= 1024 and nb < 2048:
            sp += [s for s in (2, 3, 4, 6, 8, 12, 16, 24, 32) if K // s >= 256 and fits(s) and nb * s <= 8192]
        # prune hopeless configurations (a long serial K loop on a handful of workgroups takes tens of ms per trial)
        sp = capped([s for s in sp if not (K // s > 8192 and nb * s < 256) or s == sp[-1]])
        cands += [(tile, s) for s in sp]
        if k32 and N % bn == 0:
            if M % bm == 0:
                cands += [(tile + 3, s) for s in sp if s <= 4]                        # software-pipelined main loop
            if M % bm == 0 or ak:                                                     # the 16x16x4 kernels take an M tail (K-major A)
                cands += [(tile + 6, s) for s in sp]                                  # v_mfma_f32_16x16x4_f32 main loop
                if ak and bk:
                    cands += [(tile + 9, s) for s in sp]                              # NT: K-contiguous LDS image, b128 fragments
                    cands += [(29 + tile, s) for s in sp]                             # NT: the hand-scheduled main loop (30: 128x128, 31: 128x64, 32: 64x64)
                    if tile in (1, 2) and M % bm == 0:                                # ... with 32-deep K tiles (20: 128x128, 21: 128x64): full 128-byte rows per load
                        cands += [(19 + tile, s) for s in sp]
                    if tile == 1 and M % bm == 0 and K >= 1536:                       # ... with the software-pipelined main loop (17: 128x128; 18 = 128x64
                        cands += [(17, s) for s in sp]                                # exists but never won a shape): pays on long K only
        if k32 and not bk and N % 128 == 0 and ((tile == 1 and (ak or M % 128 == 0)) or (tile == 2 and ak)):
            qsp = quad_splits(-(-M // (128 if tile == 1 else 64)) * (N // 128))
            cands += [(12 + tile, s) for s in qsp]                                    # NN / TN: quad fragments (13: 128x128, 14: 64x128)
            cands += [(32 + tile, s) for s in qsp]                                    # ... on the hand-scheduled main loop (33: 128x128, 34: 64x128)
        if k32 and ak and not bk and N % 64 == 0 and tile in (2, 3):                  # NN, 64-column quad tiles (4 x 1 waves): 16 = 128x64, 15 = 64x64
            qsp = quad_splits(-(-M // (128 if tile == 2 else 64)) * (N // 64))
            cands += [(16 if tile == 2 else 15, s) for s in qsp]
            cands += [(36 if tile == 2 else 35, s) for s in qsp]                      # ... hand-scheduled (36: 128x64, 35: 64x64)
    return cands


def gemm_tune(a, b, ak, bk, M, N, K, ws, reps=3, rounds=1, trace=None, cands=None):
    """time every (tile id, split-K) candidate for this product (``cands``: only these, else gemm_candidates) -> (best config, best ms per launch);
    ``trace`` (a list) receives every (tile, splits, ms) measured."""
    cands = list(cands) if cands is not None else gemm_candidates(ak, bk, M, N, K, ws.numel() * 4, _MAX_SPLIT)
    scratch = torch.empty(M, N, dtype=torch.float32, device=a.device)
    e = GemmEpilogue(alpha=1.0)
    best, best_t = (0, 0), float("inf")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for tile, sp in cands:
        def run():
            return lib.act_sgemm_ex_f32(int(ak), int(bk), M, N, K, _C.ptr_rows(a), a.stride(0), _C.ptr_rows(b), b.stride(0), ptr(scratch), N,
                                        ctypes.byref(e), ptr(ws), ws.numel() * 4, tile, sp, stream())
        if run() != 0:
            continue
        t = float("inf")
        for _ in range(rounds):
            ev[0].record()
            for _ in range(reps):
                run()
            ev[1].record()
            ev[1].synchronize()
            t = min(t, ev[0].elapsed_time(ev[1]) / reps)
        if trace is not None:
            trace.append((tile, sp, t))
        if t < best_t:
            best, best_t = (tile, sp), t
    return best, best_t


def gemm_config(ak, bk, M, N, K, device, a=None, b=None, ws=None, publish=False):
    """THE launch-configuration decision for the product (a_kmajor, b_kmajor, M, N, K) on ``device``: (tile id, split-K), (0, 0) = the library's
    built-in cost model; None = cannot be decided now (the shape needs timing and the stream is being captured) -- nothing is recorded then.
    Order: size cut-off, skinny-TN exemption, cache, shipped table, first-use timing -- on the operands ``a`` / ``b`` where the caller has them
    (gemm), else on random ones (composite.ensure_tuned, which knows shapes only).  A freshly timed shape is recorded in _NEW_TUNED and published to
    the C-side table the composite entry points read; ``publish``: hand the decision to that table in any case (it may have been cleared since)."""
    if not AUTOTUNE or M * N * K < (1 << 24):
        return 0, 0                                            # tiny products: built-in cost model
    if not ak and not bk and min(M, N) <= 8:
        return 0, 0                                            # skinny weight gradients: streaming-reduction kernel (gemm.hip)
    key = (int(ak), int(bk), M, N, K, device.index)
    cfg = _GEMM_CACHE.get(key)
    if cfg is not None and not publish:
        return cfg
    if cfg is None:
        cfg = _GEMM_TABLE.get(key[:5])
        if cfg is None:
            if torch.cuda.is_current_stream_capturing():
                return None
            if a is None:
                # operands of the timing only: the device generator is put back afterwards, so that a first-use timing does not move the caller's random
                # stream (the masks, dropout and noise of the step would differ between a build whose shapes are all listed and one that times a new one)
                idx = device.index if device.index is not None else (torch.cuda.current_device() if torch.cuda.is_available() else None)
                rng = torch.cuda.get_rng_state(idx) if torch.cuda.is_available() else None
                a = torch.randn((M, K) if ak else (K, M), dtype=torch.float32, device=device)
                b = torch.randn((N, K) if bk else (K, N), dtype=torch.float32, device=device)
                if rng is not None:
                    torch.cuda.set_rng_state(rng, idx)
            cfg = _NEW_TUNED[key[:5]] = first_use_config(a, b, ak, bk, M, N, K, ws if ws is not None else workspace(device))
            publish = True
        _GEMM_CACHE[key] = cfg
    if publish:
        lib.act_gemm_tune_set(key[0], key[1], M, N, K, int(cfg[0]), int(cfg[1]))
    return cfg


def _gemm_config(a, b, ak, bk, M, N, K, ws):
    """gemm_config for a product whose operands exist; during stream capture an undecided shape runs on the cost model and is decided later"""
    cfg = gemm_config(ak, bk, M, N, K, a.device, a, b, ws)
    return cfg if cfg is not None else (0, 0)


def publish_table():
    """the shipped table -> the C-side table (composite entry points)"""
    for (ak, bk, M, N, K), (tile, sp) in _GEMM_TABLE.items():
        lib.act_gemm_tune_set(ak, bk, M, N, K, tile, sp)


def layernorm_fwd(x, pos, gamma, beta, eps, want_xin=True, want_stats=True):
    x = _f32c(x)
    T, D = x.shape
    pos = _f32c(pos) if pos is not None else None
    y = torch.empty_like(x)
    xin = torch.empty_like(x) if (pos is not None and want_xin) else None
    mean = torch.empty(T, dtype=torch.float32, device=x.device) if want_stats else None
    rstd = torch.empty(T, dtype=torch.float32, device=x.device) if want_stats else None
    check(lib.act_layernorm_fwd_f32(ptr(x), ptr(pos), ptr(gamma), ptr(beta), ptr(xin), ptr(y), ptr(mean), ptr(rstd), T, D,
                                    float(eps), stream()), "act_layernorm_fwd_f32")
    return y, (xin if xin is not None else x), mean, rstd


def layernorm_bwd(dy, xin, gamma, mean, rstd, dres=None, want_params=True):
    dy = _f32c(dy)
    T, D = dy.shape
    dx = torch.empty_like(dy)
    dg = torch.empty(D, dtype=torch.float32, device=dy.device) if want_params else None
    db = torch.empty(D, dtype=torch.float32, device=dy.device) if want_params else None
    ws = workspace(dy.device, lib.act_layernorm_bwd_workspace(T, D)) if want_params else None
    check(lib.act_layernorm_bwd_f32(ptr(dy), ptr(xin), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres), ptr(dx), ptr(dg), ptr(db), 0,
                                    ptr(ws), (ws.numel() * 4 if ws is not None else 0), T, D, stream()), "act_layernorm_bwd_f32")
    return dx, dg, db


def colsum(x):
    x = _f32c(x)
    R, C = x.shape
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = workspace(x.device, lib.act_colsum_workspace(R, C))
    check(lib.act_colsum_f32(ptr(x), R, C, x.stride(0), ptr(out), 0, ptr(ws), ws.numel() * 4, stream()), "act_colsum_f32")
    return out


def attention_fwd(qkv, B, S, H, hd, want_lse=True):
    out = torch.empty(B * S, H * hd, dtype=torch.float32, device=qkv.device)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=qkv.device) if want_lse else None
    check(lib.act_attention_fwd_f32(ptr(qkv), ptr(out), ptr(lse), B, S, H, hd, float(hd) ** -0.5, stream()), "act_attention_fwd_f32")
    return out, lse


def attention_bwd(qkv, out, dout, lse, B, S, H, hd):
    dqkv = torch.empty_like(qkv)
    check(lib.act_attention_bwd_f32(ptr(qkv), ptr(out), ptr(_f32c(dout)), ptr(lse), ptr(dqkv), B, S, H, hd, float(hd) ** -0.5,
                                    stream()), "act_attention_bwd_f32")
    return dqkv


# ---- autograd Functions -----------------------------------------------------------------------------------
class LinearFn(torch.autograd.Function):
    """y = x @ w^T + b on [T,in] rows (nn.Linear / Conv1d k=1)."""

    @staticmethod
    def forward(ctx, x, w, b):
        shp = x.shape
        x2 = _f32c(x).reshape(-1, shp[-1])
        y = gemm(x2, w, True, True, bias=b)
        ctx.save_for_backward(x2, w)
        ctx.has_bias = b is not None
        ctx.shp = shp
        return y.reshape(*shp[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        dy2 = _f32c(dy).reshape(-1, w.shape[0])
        want_dw, want_db = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        # LINEAR_OVERLAP_DW (Stage-I autoencoder step, runner_autoencoder.train_step): dW / db on auxiliary stream 1 while the input gradient
        # runs on the main stream -- two chip-filling GEMMs side by side fill each other's partial last round of workgroups; joined before
        # returning (autograd accumulates the gradients on the main stream right away)
        par = LINEAR_OVERLAP_DW and OVERLAP_DW and dy2.is_cuda and ctx.needs_input_grad[0] and (want_dw or want_db) and dy2.shape[0] >= 4096
        if par:
            with fork_side(dy2.device):
                dw = gemm(dy2, x2, False, False) if want_dw else None
                db = colsum(dy2) if want_db else None
            dx = gemm(dy2, w, True, False).reshape(ctx.shp)
            join_side(dy2.device, dw, db)
            return dx, dw, db
        dx = gemm(dy2, w, True, False).reshape(ctx.shp) if ctx.needs_input_grad[0] else None
        dw = gemm(dy2, x2, False, False) if want_dw else None
        db = colsum(dy2) if want_db else None
        return dx, dw, db


def linear(x, w, b=None):
    return LinearFn.apply(x, w, b)


class MlpFn(torch.autograd.Function):
    """fc2(gelu(fc1(x))) with the GELU fused in fc1's epilogue and gelu' fused in fc2's input-gradient GEMM."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        shp = x.shape
        x2 = _f32c(x).reshape(-1, shp[-1])
        hpre = torch.empty(x2.shape[0], w1.shape[0], dtype=torch.float32, device=x.device)
        a = gemm(x2, w1, True, True, bias=b1, act=EPI_GELU, aux=hpre)
        y = gemm(a, w2, True, True, bias=b2)
        ctx.save_for_backward(x2, w1, w2, hpre, a)
        ctx.shp = shp
        return y.reshape(*shp[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w1, w2, hpre, a = ctx.saved_tensors
        dy2 = _f32c(dy).reshape(-1, w2.shape[0])
        dh = gemm(dy2, w2, True, False, act=EPI_MUL_GELU_GRAD, aux=hpre)
        dw2 = gemm(dy2, a, False, False) if ctx.needs_input_grad[3] else None
        db2 = colsum(dy2) if ctx.needs_input_grad[4] else None
        dx = gemm(dh, w1, True, False).reshape(ctx.shp) if ctx.needs_input_grad[0] else None
        dw1 = gemm(dh, x2, False, False) if ctx.needs_input_grad[1] else None
        db1 = colsum(dh) if ctx.needs_input_grad[2] else None
        return dx, dw1, db1, dw2, db2


def mlp(x, w1, b1, w2, b2):
    return MlpFn.apply(x, w1, b1, w2, b2)


class MlpRelu3Fn(torch.autograd.Function):
    """Linear-ReLU-Linear-ReLU-Linear (the FoldingNet coarse MLP, models/dvae.py:226-232): ReLU fused in the producing GEMM's epilogue,
    the ReLU mask of the backward fused in the input-gradient GEMM of the following layer (ACT_EPI_MUL_RELU_MASK)."""

    @staticmethod
    def forward(ctx, x, w0, b0, w1, b1, w2, b2):
        x2 = _f32c(x).reshape(-1, x.shape[-1])
        h1 = gemm(x2, w0, True, True, bias=b0, act=EPI_RELU)
        h2 = gemm(h1, w1, True, True, bias=b1, act=EPI_RELU)
        y = gemm(h2, w2, True, True, bias=b2)
        ctx.save_for_backward(x2, h1, h2, w0, w1, w2)
        ctx.shp = x.shape
        return y.reshape(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, h1, h2, w0, w1, w2 = ctx.saved_tensors
        dy = _f32c(dy).reshape(-1, w2.shape[0])
        dw2, db2 = gemm(dy, h2, False, False), colsum(dy)
        d2 = gemm(dy, w2, True, False, act=EPI_MUL_RELU_MASK, aux=h2)        # gradient before the second ReLU
        dw1, db1 = gemm(d2, h1, False, False), colsum(d2)
        d1 = gemm(d2, w1, True, False, act=EPI_MUL_RELU_MASK, aux=h1)
        dw0, db0 = gemm(d1, x2, False, False), colsum(d1)
        dx = gemm(d1, w0, True, False).reshape(ctx.shp) if ctx.needs_input_grad[0] else None
        return dx, dw0, db0, dw1, db1, dw2, db2


def mlp_relu3(x, w0, b0, w1, b1, w2, b2):
    return MlpRelu3Fn.apply(x, w0, b0, w1, b1, w2, b2)


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        shp = x.shape
        x2 = _f32c(x).reshape(-1, shp[-1])
        y, _, mean, rstd = layernorm_fwd(x2, None, gamma, beta, eps)
        ctx.save_for_backward(x2, gamma, mean, rstd)
        ctx.shp = shp
        return y.reshape(shp)

    @staticmethod
    def backward(ctx, dy):
        x2, gamma, mean, rstd = ctx.saved_tensors
        dy2 = _f32c(dy).reshape(x2.shape)
        want = ctx.needs_input_grad[1]
        dx, dg, db = layernorm_bwd(dy2, x2, gamma, mean, rstd, None, want_params=want)
        return dx.reshape(ctx.shp), dg, db, None


def layer_norm(x, gamma, beta, eps=1e-5):
    return LayerNormFn.apply(x, gamma, beta, eps)


class BlockFnPerKernel(torch.autograd.Function):
    """One pre-LN Transformer block applied to (x + pos)  -- models/act.py:72-90 called as blk(x + pos) (:109-112), issued from the
    host one kernel at a time.  The product path is composite.BlockFn (one host call per direction, same kernels, bit-identical
    results); this form stays for ACT_COMPOSITE=0 A/B measurements and the bit-identity test.

    forward : xin = x+pos ; x1 = xin + g1*(proj(attn(LN1(xin)))+b) ; x2 = x1 + g2*(fc2(gelu(fc1(LN2(x1))))+b)
    g1/g2 are the per-sample DropPath gates (floor(keep+U)/keep) or None.  7 launches forward.
    """

    @staticmethod
    def forward(ctx, x, pos, gate1, gate2, n1w, n1b, wqkv, bqkv, wproj, bproj, n2w, n2b, w1, b1, w2, b2, heads, eps, train_w):
        B, S, D = x.shape
        hd = D // heads
        x2d = _f32c(x).reshape(B * S, D)
        pos2d = _f32c(pos).reshape(B * S, D) if pos is not None else None
        need_grad = any(ctx.needs_input_grad)
        n1, xin, mean1, rstd1 = layernorm_fwd(x2d, pos2d, n1w, n1b, eps, want_stats=need_grad)
        qkv = gemm(n1, wqkv, True, True, bias=bqkv)
        att, lse = attention_fwd(qkv, B, S, heads, hd, want_lse=need_grad)
        x1 = gemm(att, wproj, True, True, bias=bproj, rowscale=gate1, rows_per_scale=S, res=xin)
        n2, _, mean2, rstd2 = layernorm_fwd(x1, None, n2w, n2b, eps, want_stats=need_grad)
        hpre = torch.empty(B * S, w1.shape[0], dtype=torch.float32, device=x.device) if need_grad else None
        a = gemm(n2, w1, True, True, bias=b1, act=EPI_GELU, aux=hpre)
        x2 = gemm(a, w2, True, True, bias=b2, rowscale=gate2, rows_per_scale=S, res=x1)
        if need_grad:
            ctx.save_for_backward(xin, mean1, rstd1, n1, qkv, att, lse, x1, mean2, rstd2, n2, hpre, a, gate1, gate2,
                                  n1w, wqkv, wproj, n2w, w1, w2)
            ctx.dims = (B, S, D, heads, hd)
            ctx.has_bqkv = bqkv is not None
            ctx.has_pos = pos is not None
            ctx.train_w = train_w
        return x2.reshape(B, S, D)

    @staticmethod
    def backward(ctx, dx2):
        (xin, mean1, rstd1, n1, qkv, att, lse, x1, mean2, rstd2, n2, hpre, a, gate1, gate2,
         n1w, wqkv, wproj, n2w, w1, w2) = ctx.saved_tensors
        B, S, D, heads, hd = ctx.dims
        tw = bool(ctx.train_w)
        dx2 = _f32c(dx2).reshape(B * S, D)
        dy2 = dx2 if gate2 is None else scale_rows(dx2, gate2, S)
        dev = dx2.device
        # train_w == 2: weight gradients on the auxiliary stream, concurrent with the dX chain (measured: +1 % on the Stage-II step,
        # -7 % on the finetune step, so only ACT_PointDistillation asks for it)
        par = ctx.train_w == 2 and OVERLAP_DW and dx2.is_cuda
        dw2 = db2 = dw1 = db1 = dwproj = dbproj = dwqkv = dbqkv = None

        def wgrad(dy, x, want_bias=True):
            """dW = dy^T x, db = column sums of dy"""
            if not tw:
                return None, None
            if par:
                with fork_side(dev):
                    return gemm(dy, x, False, False), (colsum(dy) if want_bias else None)
            return gemm(dy, x, False, False), (colsum(dy) if want_bias else None)

        # two Linears at a time through the grouped launch (csrc/gemm_grouped.hip), as act_block_bwd_f32 does -- same kernels, same K-range
        # counts, so the per-kernel path stays bit-identical to the composite one
        T = B * S
        grouped = tw and GROUPED_DW and D % 128 == 0 and w1.shape[0] % 128 == 0 and T % 16 == 0

        def wgrad2(p0, p1, bias1=True):
            def run():
                dws, dbs = gemm_tn_grouped([p0, p1], want_bias=True)
                return dws[0], dbs[0], dws[1], (dbs[1] if bias1 else None)
            if par:
                with fork_side(dev):
                    return run()
            return run()

        if not grouped:
            dw2, db2 = wgrad(dy2, a)
        dh = gemm(dy2, w2, True, False, act=EPI_MUL_GELU_GRAD, aux=hpre)
        if grouped:
            dw2, db2, dw1, db1 = wgrad2((dy2, a), (dh, n2))
        else:
            dw1, db1 = wgrad(dh, n2)
        dn2 = gemm(dh, w1, True, False)
        dx1, dg2, dbt2 = layernorm_bwd(dn2, x1, n2w, mean2, rstd2, dres=dx2, want_params=tw)
        dy1 = dx1 if gate1 is None else scale_rows(dx1, gate1, S)
        if not grouped:
            dwproj, dbproj = wgrad(dy1, att)
        datt = gemm(dy1, wproj, True, False)
        dqkv = attention_bwd(qkv, att, datt, lse, B, S, heads, hd)
        if grouped:
            dwproj, dbproj, dwqkv, dbqkv = wgrad2((dy1, att), (dqkv, n1), ctx.has_bqkv)
        else:
            dwqkv, dbqkv = wgrad(dqkv, n1, ctx.has_bqkv)
        dn1 = gemm(dqkv, wqkv, True, False)
        dxin, dg1, dbt1 = layernorm_bwd(dn1, xin, n1w, mean1, rstd1, dres=dx1, want_params=tw)
        if par:
            join_side(dev, dw2, db2, dw1, db1, dwproj, dbproj, dwqkv, dbqkv)
        dxin = dxin.reshape(B, S, D)
        return (dxin, dxin if ctx.has_pos else None, None, None, dg1, dbt1, dwqkv, dbqkv, dwproj, dbproj, dg2, dbt2,
                dw1, db1, dw2, db2, None, None, None)


def scale_rows(x, gate, rows_per_scale):
    """x[r,:] * gate[r // rows_per_scale]  (DropPath gate on a gradient)."""
    T, D = x.shape
    return (x.view(-1, rows_per_scale, D) * gate.view(-1, 1, 1)).view(T, D)


class CosineLossFn(torch.autograd.Function):
    """mean over rows of 1 - cos(student, teacher)   (models/act.py:1243-1254 with loss='cosine')."""

    @staticmethod
    def forward(ctx, student, teacher):
        D = student.shape[-1]
        s2 = _f32c(student).reshape(-1, D)
        t2 = _f32c(teacher).reshape(-1, D)
        R = s2.shape[0]
        loss = torch.empty(1, dtype=torch.float32, device=s2.device)
        row = torch.empty(R, dtype=torch.float32, device=s2.device)
        stats = torch.empty(R, 3, dtype=torch.float32, device=s2.device)
        check(lib.act_cosine_loss_fwd_f32(ptr(s2), ptr(t2), R, D, 1e-8, ptr(loss), ptr(row), ptr(stats), stream()),
              "act_cosine_loss_fwd_f32")
        ctx.save_for_backward(s2, t2, stats)
        ctx.shp = student.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        s2, t2, stats = ctx.saved_tensors
        R, D = s2.shape
        ds = torch.empty_like(s2)
        check(lib.act_cosine_loss_bwd_f32(ptr(s2), ptr(t2), ptr(stats), ptr(_f32c(g).reshape(-1)), R, D, 1e-8, ptr(ds), stream()),
              "act_cosine_loss_bwd_f32")
        return ds.reshape(ctx.shp), None


def cosine_distill_loss(student, teacher):
    return CosineLossFn.apply(student, teacher).reshape(())


def pairwise_distill_loss(student, teacher, kind, num_mask, temperature=0.07, lambda_param=5e-3):
    """loss: 'ntxent' | 'barlow' of ACT_PointDistillation (models/act.py:1192-1195,1250-1254): per cloud lightly's NTXentLoss(temperature=0.07) /
    BarlowTwinsLoss(lambda_param=5e-3) on (student[b], teacher[b]) -- the masked tokens of one cloud are the "batch" of the contrastive loss -- divided by
    num_mask, summed over the clouds, / batch size.  lightly 1.2.28 is not importable here: the algorithms are the published ones (oracle/layers.py
    restates them the same way; parity against the package itself is unpinned).  Not in any shipped recipe, so not a tuned path: the matrix products run
    on the library's GEMMs through K.linear (forward and both gradients), the row-wise pieces are a handful of elementwise / reduction ops.
      ntxent: the 2n x 2n similarity blocks of 16 clouds at a time are the diagonal blocks of ONE [16 * 2n, C] x [16 * 2n, C]^T product.
      barlow: one [D, n] x [D, n]^T product per cloud -- O(B) launches plus a transposed copy per cloud (there is no batched GEMM entry point in the
      library; acceptable for a loss that no shipped recipe selects, a cost to know about before selecting it at B = 128).
    Returns a 0-dim tensor like every other loss of this module (the reference's ``loss.mean() / batch_size``)."""
    B, n, C = student.shape
    s = _f32c(student); t = _f32c(teacher)
    if kind == "ntxent":
        z = torch.cat([torch.nn.functional.normalize(s, dim=2), torch.nn.functional.normalize(t, dim=2)], dim=1)       # [B, 2n, C]
        m = 2 * n
        eye = torch.eye(m, dtype=torch.bool, device=s.device)
        partner = torch.cat([torch.arange(n, m, device=s.device), torch.arange(0, n, device=s.device)])
        total = s.new_zeros(())
        for c0 in range(0, B, 16):
            zc = z[c0:c0 + 16].reshape(-1, C)
            g = zc.shape[0] // m
            sim = linear(zc, zc).view(g, m, g, m)
            blk = torch.diagonal(sim, dim1=0, dim2=2).permute(2, 0, 1) / temperature                                   # [g, 2n, 2n]
            pos = blk.gather(2, partner.view(1, m, 1).expand(g, m, 1)).squeeze(2)
            lse = torch.logsumexp(blk.masked_fill(eye, float("-inf")), dim=2)
            total = total + (lse - pos).mean(dim=1).sum()
        return (total / num_mask / B).reshape(())
    if kind == "barlow":
        za = (s - s.mean(1, keepdim=True)) / s.std(1, keepdim=True)                                                    # unbiased std along the tokens
        zb = (t - t.mean(1, keepdim=True)) / t.std(1, keepdim=True)
        eye = torch.eye(C, device=s.device)
        w = torch.full((C, C), lambda_param, device=s.device); w.fill_diagonal_(1.0)
        total = s.new_zeros(())
        for b in range(B):
            c = linear(za[b].t().contiguous(), zb[b].t().contiguous()) / n                                             # z_a^T z_b / n  [C, C]
            total = total + ((c - eye).pow(2) * w).sum()
        return (total / num_mask / B).reshape(())
    raise _C.ActHipError(f"pairwise_distill_loss: unknown kind {kind!r}")


class RegressionLossFn(torch.autograd.Function):
    """loss: 'l2' (nn.MSELoss) / 'smoothl1' (nn.SmoothL1Loss), mean over all elements (models/act.py:1186-1191,1255)."""

    @staticmethod
    def forward(ctx, student, teacher, kind):
        D = student.shape[-1]
        s2 = _f32c(student).reshape(-1, D); t2 = _f32c(teacher).reshape(-1, D)
        R = s2.shape[0]
        loss = torch.empty(1, dtype=torch.float32, device=s2.device)
        row = torch.empty(R, dtype=torch.float32, device=s2.device)
        check(lib.act_regression_loss_fwd_f32(ptr(s2), ptr(t2), R, D, int(kind), ptr(loss), ptr(row), stream()), "act_regression_loss_fwd_f32")
        ctx.save_for_backward(s2, t2)
        ctx.kind, ctx.shp = int(kind), student.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        s2, t2 = ctx.saved_tensors
        R, D = s2.shape
        ds = torch.empty_like(s2)
        check(lib.act_regression_loss_bwd_f32(ptr(s2), ptr(t2), ptr(_f32c(g).reshape(-1)), R, D, ctx.kind, ptr(ds), stream()),
              "act_regression_loss_bwd_f32")
        return ds.reshape(ctx.shp), None, None


def regression_distill_loss(student, teacher, kind):
    return RegressionLossFn.apply(student, teacher, {"l2": 0, "smoothl1": 1}[kind]).reshape(())


class SoftmaxXentFn(torch.autograd.Function):
    """nn.CrossEntropyLoss() (mean) + top-1 accuracy fraction of the same logits (models/act.py:823-830)."""

    @staticmethod
    def forward(ctx, logits, labels):
        z = _f32c(logits)
        R, C = z.shape
        lab = labels.to(torch.int64).contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=z.device)
        acc = torch.empty(1, dtype=torch.float32, device=z.device)                 # fraction of correct rows
        buf = torch.empty(3, R, dtype=torch.float32, device=z.device)
        check(lib.act_softmax_xent_fwd_f32(ptr(z), ptr(lab), R, C, ptr(loss), ptr(buf), ptr(acc), stream()),
              "act_softmax_xent_fwd_f32")
        ctx.save_for_backward(z, lab, buf)
        ctx.mark_non_differentiable(acc)
        return loss, acc

    @staticmethod
    def backward(ctx, g, _gacc):
        z, lab, buf = ctx.saved_tensors
        R, C = z.shape
        dz = torch.empty_like(z)
        check(lib.act_softmax_xent_bwd_f32(ptr(z), ptr(lab), ptr(buf), ptr(_f32c(g).reshape(-1)), R, C, ptr(dz), stream()),
              "act_softmax_xent_bwd_f32")
        return dz, None


def softmax_xent(logits, labels):
    """-> (mean cross-entropy loss, fraction of rows with arg-max == label), both 0-d tensors on the device."""
    loss, acc = SoftmaxXentFn.apply(logits, labels)
    return loss.reshape(()), acc.reshape(())


# ---- mini-PointNet / FoldingNet row kernels (csrc/pointnet.hip) --------------------------------------------------
class BNActFn(torch.autograd.Function):
    """BatchNorm1d over the rows of x [R,C] (+ optional ReLU).  train: batch statistics (biased variance), running stats
    updated in place (momentum, unbiased variance) like nn.BatchNorm1d; eval: running statistics."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, relu):
        x = _f32c(x)
        R, C = x.shape
        dev = x.device
        y = torch.empty_like(x)
        if training:
            mean, rstd, scale, shift = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(4))
            ws = workspace(dev, lib.act_colstats_workspace(R, C))
            check(lib.act_bn_stats_f32(ptr(x), R, C, ptr(gamma), ptr(beta), float(eps), float(momentum), ptr(running_mean),
                                       ptr(running_var), ptr(mean), ptr(rstd), ptr(scale), ptr(shift), ptr(ws), ws.numel() * 4,
                                       stream()), "act_bn_stats_f32")
        else:
            rstd = torch.rsqrt(running_var + eps)
            mean = running_mean
            scale = gamma * rstd
            shift = beta - running_mean * scale
        check(lib.act_affine_act_f32(ptr(x), ptr(scale), ptr(shift), int(relu), R, C, ptr(y), stream()), "act_affine_act_f32")
        ctx.save_for_backward(x, scale, shift, mean, rstd)
        ctx.training, ctx.relu = training, relu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, scale, shift, mean, rstd = ctx.saved_tensors
        dy = _f32c(dy)
        R, C = x.shape
        if not ctx.training:
            raise NotImplementedError("BatchNorm backward in eval mode is off the training path")
        dx = torch.empty_like(x)
        dg = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = workspace(x.device, lib.act_colstats_workspace(R, C))
        check(lib.act_bn_bwd_f32(ptr(x), ptr(dy), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), int(ctx.relu), R, C, ptr(dx), ptr(dg),
                                 ptr(db), ptr(ws), ws.numel() * 4, stream()), "act_bn_bwd_f32")
        return dx, dg, db, None, None, None, None, None, None


class SyncBNActFn(torch.autograd.Function):
    """nn.SyncBatchNorm (+ReLU) on rows [R,C] in train mode: batch statistics over the rows of ALL ranks of ``group`` (the reference's
    --sync_bn path, tools/runner_pretrain.py:86-88).  Per rank: one statistics pass (mean, biased variance, row count), an all-gather of
    3 x C floats, Chan's combination of the per-rank moments, the affine apply; backward: the two local column sums are all-reduced
    before dx is formed (dgamma / dbeta stay local sums, DDP averages them like every other gradient -- torch's SyncBatchNorm does the same)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, relu, group):
        import torch.distributed as dist
        x = _f32c(x)
        R, C = x.shape
        dev = x.device
        local = torch.empty(3, C, dtype=torch.float32, device=dev)         # mean | var | count
        ws = workspace(dev, lib.act_colstats_workspace(R, C))
        check(lib.act_col_mean_var_f32(ptr(x), R, C, ptr(local[0]), ptr(local[1]), ptr(ws), ws.numel() * 4, stream()), "act_col_mean_var_f32")
        local[2].fill_(float(R))
        world = dist.get_world_size(group)
        gathered = torch.empty(world, 3, C, dtype=torch.float32, device=dev)
        dist.all_gather_into_tensor(gathered, local, group=group) if dist.get_backend(group) == "nccl" else \
            dist.all_gather(list(gathered.unbind(0)), local, group=group)
        n = gathered[:, 2]                                                  # [world, C]
        total = n.sum(0)
        mean = (gathered[:, 0] * n).sum(0) / total
        var = ((gathered[:, 1] + (gathered[:, 0] - mean) ** 2) * n).sum(0) / total          # biased variance over all rows
        rstd = torch.rsqrt(var + eps)
        scale = (gamma * rstd).contiguous()
        shift = (beta - mean * scale).contiguous()
        if running_mean is not None:
            with torch.no_grad():
                running_mean.mul_(1 - momentum).add_(mean, alpha=momentum)
                running_var.mul_(1 - momentum).add_(var * (total / (total - 1).clamp_min(1)), alpha=momentum)
        y = torch.empty_like(x)
        check(lib.act_affine_act_f32(ptr(x), ptr(scale), ptr(shift), int(relu), R, C, ptr(y), stream()), "act_affine_act_f32")
        ctx.save_for_backward(x, scale, shift, mean.contiguous(), rstd.contiguous(), total[:1].contiguous())
        ctx.relu, ctx.group = relu, group
        return y

    @staticmethod
    def backward(ctx, dy):
        import torch.distributed as dist
        x, scale, shift, mean, rstd, total = ctx.saved_tensors
        dy = _f32c(dy)
        R, C = x.shape
        dev = x.device
        sums = torch.empty(2, C, dtype=torch.float32, device=dev)           # sum dy | sum dy * xhat  (this rank)
        ws = workspace(dev, lib.act_colstats_workspace(R, C))
        check(lib.act_bn_bwd_sums_f32(ptr(x), ptr(dy), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), int(ctx.relu), R, C, ptr(sums[0]), ptr(sums[1]),
                                      ptr(ws), ws.numel() * 4, stream()), "act_bn_bwd_sums_f32")
        db, dg = sums[0].clone(), sums[1].clone()
        dist.all_reduce(sums, group=ctx.group)
        dx = torch.empty_like(x)
        # the kernel divides by a HOST scalar; the true row count over all ranks lives on the device (``total``, gathered in forward).  Rescale
        # the sums by (R * world) / total there: exactly 1.0 for equal shards (bit-identical to dividing by R * world), and the right
        # normalisation for ragged last batches / non-drop_last loaders -- without a host synchronisation.
        count = float(R * dist.get_world_size(ctx.group))
        sums.mul_(count / total)
        check(lib.act_bn_bwd_apply_f32(ptr(x), ptr(dy), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), ptr(sums[0]), ptr(sums[1]), count, int(ctx.relu),
                                       R, C, ptr(dx), stream()), "act_bn_bwd_apply_f32")
        return dx, dg, db, None, None, None, None, None, None


def _sync_group(bn):
    """process group of a SyncBatchNorm module when its statistics must be synchronised right now, else None"""
    if not isinstance(bn, torch.nn.SyncBatchNorm):
        return None
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return None
    group = bn.process_group if bn.process_group is not None else dist.group.WORLD
    return group if dist.get_world_size(group) > 1 else None


def batch_norm_act(x, bn, training, relu=True, slope=None):
    """functional nn.BatchNorm1d / nn.SyncBatchNorm (+ReLU) on rows [R,C] with the module's parameters and buffers.  ``slope`` (a float): LeakyReLU
    of that slope follows instead (``relu`` is then ignored; csrc/edgeconv.hip); None: exactly the ReLU / identity path."""
    group = _sync_group(bn) if training else None
    if slope is not None and group is not None:
        raise NotImplementedError("batch_norm_act: slope= with a SyncBatchNorm across ranks is not implemented")
    if training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    if slope is not None:
        return BNLreluFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, bn.momentum, bn.eps, float(slope))
    if group is not None:
        return SyncBNActFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, relu, group)
    return BNActFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, bn.momentum, bn.eps, relu)


class GroupMaxFn(torch.autograd.Function):
    """x [G*n, C] -> max over the n rows of every group, [G, C]   (torch.max(feature, dim=2) of models/dvae.py:211,214)."""

    @staticmethod
    def forward(ctx, x, n):
        x = _f32c(x)
        R, C = x.shape
        G = R // n
        out = torch.empty(G, C, dtype=torch.float32, device=x.device)
        arg = torch.empty(G, C, dtype=torch.int32, device=x.device)
        check(lib.act_group_max_f32(ptr(x), G, n, C, ptr(out), ptr(arg), stream()), "act_group_max_f32")
        ctx.save_for_backward(arg)
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, dout):
        (arg,) = ctx.saved_tensors
        dout = _f32c(dout)
        G, C = dout.shape
        din = torch.empty(G * ctx.n, C, dtype=torch.float32, device=dout.device)
        check(lib.act_group_max_bwd_f32(ptr(dout), ptr(arg), G, ctx.n, C, 0, ptr(din), stream()), "act_group_max_bwd_f32")
        return din, None


def group_max(x, n):
    return GroupMaxFn.apply(x, n)


class LinearGroupAddFn(torch.autograd.Function):
    """y[r,:] = x[r,:] @ w^T + g[r // n, :]  -- the per-point half of a conv over cat(per-group feature, per-point feature)
    with the per-group half g added in the GEMM epilogue (models/dvae.py:212-213, :266-271)."""

    @staticmethod
    def forward(ctx, x, w, g, n):
        x = _f32c(x); g = _f32c(g)
        y = gemm(x, w, True, True, res=g, res_row_div=n)
        ctx.save_for_backward(x, w)
        ctx.n = n
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _f32c(dy)
        dx = gemm(dy, w, True, False) if ctx.needs_input_grad[0] else None
        dw = gemm(dy, x, False, False) if ctx.needs_input_grad[1] else None
        dg = None
        if ctx.needs_input_grad[2]:
            R, C = dy.shape
            dg = torch.empty(R // ctx.n, C, dtype=torch.float32, device=dy.device)
            check(lib.act_group_sum_f32(ptr(dy), R // ctx.n, ctx.n, C, ptr(dg), stream()), "act_group_sum_f32")
        return dx, dw, dg, None


def linear_group_add(x, w, g, n):
    return LinearGroupAddFn.apply(x, w, g, n)


# ---- DGCNN / tokenizer glue (csrc/dgcnn.hip) -------------------------------------------------------------------------
def edge_gn_lrelu_max(yz, zoff, idx, B, G, k, C, gn, out=None, ooff=0, slope=0.2):
    """inference-only tail of a DGCNN layer (see csrc/dgcnn.hip); yz [B*G, ld], -> out[:, ooff:ooff+C]."""
    yz = _f32c(yz)
    if out is None:
        out = torch.empty(B * G, C, dtype=torch.float32, device=yz.device)
    stats = torch.empty(18 * B * gn.num_groups, dtype=torch.float32, device=yz.device)
    check(lib.act_edge_gn_lrelu_max_f32(ptr(yz), yz.stride(0), int(zoff), ptr(idx), B, G, k, C, gn.num_groups, ptr(gn.weight),
                                        ptr(gn.bias), float(gn.eps), float(slope), ptr(stats), ptr(out), out.stride(0), int(ooff),
                                        stream()), "act_edge_gn_lrelu_max_f32")
    return out


class EdgeGnLreluMaxFn(torch.autograd.Function):
    """differentiable tail of a DGCNN layer: out[b*G+g, c] = max_j LeakyReLU(GroupNorm(Y[b, idx[b,j,g], c] + Z[b,g,c])) with
    yz = [Y | Z] (zoff = column of Z, -1: none); idx None: the k = 1 GroupNorm + LeakyReLU head.  Backward = three HIP launches
    (csrc/dgcnn.hip) + two column sums for dgamma / dbeta."""

    @staticmethod
    def forward(ctx, yz, gamma, beta, idx, zoff, B, G, k, C, groups, eps, slope):
        yz = _f32c(yz)
        out = torch.empty(B * G, C, dtype=torch.float32, device=yz.device)
        stats = torch.empty(18 * B * groups, dtype=torch.float32, device=yz.device)
        check(lib.act_edge_gn_lrelu_max_f32(ptr(yz), yz.stride(0), int(zoff), ptr(idx), B, G, k, C, groups, ptr(gamma), ptr(beta),
                                            float(eps), float(slope), ptr(stats), ptr(out), C, 0, stream()), "act_edge_gn_lrelu_max_f32")
        ctx.save_for_backward(yz, gamma, beta, idx, stats)
        ctx.cfg = (int(zoff), B, G, k, C, groups, float(slope))
        return out

    @staticmethod
    def backward(ctx, dout):
        yz, gamma, beta, idx, stats = ctx.saved_tensors
        zoff, B, G, k, C, groups, slope = ctx.cfg
        dout = _f32c(dout)
        dyz = torch.empty_like(yz)
        part = torch.empty(2, B, C, dtype=torch.float32, device=yz.device)
        mstat = torch.empty(2 * B * groups, dtype=torch.float32, device=yz.device)
        check(lib.act_edge_gn_lrelu_max_bwd_f32(ptr(yz), yz.stride(0), zoff, ptr(idx), B, G, k, C, groups, ptr(gamma), ptr(beta),
                                                ptr(stats), slope, ptr(dout), dout.stride(0), ptr(dyz), ptr(part), ptr(mstat),
                                                stream()), "act_edge_gn_lrelu_max_bwd_f32")
        return (dyz, colsum(part[0]), colsum(part[1])) + (None,) * 9


def edge_gn_lrelu_max_train(yz, zoff, idx, B, G, k, C, gn, slope=0.2):
    return EdgeGnLreluMaxFn.apply(yz, gn.weight, gn.bias, idx, zoff, B, G, k, C, gn.num_groups, gn.eps, slope)


class GumbelSoftmaxFn(torch.autograd.Function):
    """F.gumbel_softmax(logits, tau, hard=False, dim=-1) on rows [R,C]; noise: given gumbel draws or None -> in-kernel Philox."""

    @staticmethod
    def forward(ctx, logits, noise, seed, tau):
        z = _f32c(logits)
        C = z.shape[-1]
        z2 = z.reshape(-1, C)
        y = torch.empty_like(z2)
        nz = _f32c(noise).reshape(-1, C) if noise is not None else None
        check(lib.act_gumbel_softmax_fwd_f32(ptr(z2), z2.shape[0], C, ptr(nz), int(seed), float(tau), ptr(y), stream()),
              "act_gumbel_softmax_fwd_f32")
        ctx.save_for_backward(y)
        ctx.tau, ctx.shp = float(tau), logits.shape
        return y.reshape(logits.shape)

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        R, C = y.shape
        dy = _f32c(dy).reshape(R, C)
        dl = torch.empty_like(y)
        check(lib.act_gumbel_softmax_bwd_f32(ptr(y), ptr(dy), R, C, ctx.tau, ptr(dl), stream()), "act_gumbel_softmax_bwd_f32")
        return dl.reshape(ctx.shp), None, None, None


def gumbel_softmax(logits, tau, noise=None, seed=0):
    return GumbelSoftmaxFn.apply(logits, noise, seed, tau)


class KLUniformFn(torch.autograd.Function):
    """KL(mean_g softmax(logits[b,g,:]) || uniform), 'batchmean' (models/dvae.py:470-476); logits [B,G,C] -> scalar."""

    @staticmethod
    def forward(ctx, logits):
        z = _f32c(logits)
        B, G, C = z.shape
        lse = torch.empty(B * G, dtype=torch.float32, device=z.device)
        qbar = torch.empty(B, C, dtype=torch.float32, device=z.device)
        out = torch.empty(1, dtype=torch.float32, device=z.device)
        check(lib.act_kl_uniform_fwd_f32(ptr(z), B, G, C, ptr(lse), ptr(qbar), ptr(out), stream()), "act_kl_uniform_fwd_f32")
        ctx.save_for_backward(z, lse, qbar)
        return out

    @staticmethod
    def backward(ctx, g):
        z, lse, qbar = ctx.saved_tensors
        B, G, C = z.shape
        dl = torch.empty_like(z)
        check(lib.act_kl_uniform_bwd_f32(ptr(z), ptr(lse), ptr(qbar), ptr(_f32c(g).reshape(-1)), B, G, C, ptr(dl), stream()),
              "act_kl_uniform_bwd_f32")
        return dl


def kl_to_uniform(logits):
    return KLUniformFn.apply(logits).reshape(())


def gn_gumbel_argmax_gather(h, B, G, gn, codebook, noise=None, seed=0, tau=1.0, want_logits=False, slope=0.2, seed_dev=None):
    """fused layer5 GroupNorm + LeakyReLU + hard gumbel-softmax + codebook lookup -> (codes [B,G,D], index [B,G], logits|None)."""
    h = _f32c(h)
    C = h.shape[1]
    D = codebook.shape[1]
    dev = h.device
    stats = torch.empty(18 * B * gn.num_groups, dtype=torch.float32, device=dev)
    index = torch.empty(B, G, dtype=torch.int64, device=dev)
    out = torch.empty(B, G, D, dtype=torch.float32, device=dev)
    logits = torch.empty(B, G, C, dtype=torch.float32, device=dev) if want_logits else None
    noise = _f32c(noise) if noise is not None else None
    check(lib.act_gn_gumbel_argmax_gather_f32(ptr(h), B, G, C, gn.num_groups, ptr(gn.weight), ptr(gn.bias), float(gn.eps), float(slope),
                                              ptr(noise), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(seed_dev), float(tau), ptr(_f32c(codebook)), D, ptr(stats),
                                              ptr(index), ptr(out), ptr(logits), stream()), "act_gn_gumbel_argmax_gather_f32")
    return out, index, logits


def attention_fwd_prefix(kv0, S0, qkv1, Sq, B, H, hd, want_lse=False):
    """queries = the Sq rows of qkv1 [B*Sq, 3*H*hd]; keys/values = S0 rows of kv0 [B*S0, 2*H*hd] then the rows of qkv1."""
    out = torch.empty(B * Sq, H * hd, dtype=torch.float32, device=qkv1.device)
    lse = torch.empty(B, H, Sq, dtype=torch.float32, device=qkv1.device) if want_lse else None
    check(lib.act_attention_fwd_prefix_f32(ptr(_f32c(kv0)), S0, ptr(_f32c(qkv1)), Sq, ptr(out), ptr(lse), B, H, hd, float(hd) ** -0.5,
                                           stream()), "act_attention_fwd_prefix_f32")
    return (out, lse) if want_lse else out


def attention_bwd_prefix(kv0, S0, qkv1, Sq, out, dout, lse, B, H, hd):
    """-> (dkv0 [B*S0, 2*H*hd], dqkv1 [B*Sq, 3*H*hd])"""
    dkv0 = torch.empty_like(kv0)
    dqkv1 = torch.empty_like(qkv1)
    check(lib.act_attention_bwd_prefix_f32(ptr(kv0), S0, ptr(qkv1), Sq, ptr(out), ptr(_f32c(dout)), ptr(lse), ptr(dkv0), ptr(dqkv1),
                                           B, H, hd, float(hd) ** -0.5, stream()), "act_attention_bwd_prefix_f32")
    return dkv0, dqkv1


class PrefixBlockFnPerKernel(torch.autograd.Function):
    """Pre-LN block on G patch tokens per cloud with P prompt tokens acting as keys/values only, WITH backward to the patch
    tokens, their positions and the prompts (Stage-I prompt tuning of the frozen Transformer, models/dvae.py:536-576: every
    layer replaces the prompt rows of its input and the output drops them, so prompt rows never need queries / proj / MLP).
    The block weights are frozen (freeze_visual_embed: True); inputs x2d [B*G,D], pos2d [B*G,D], prm2d [B*P,D] = prompt+pos."""

    @staticmethod
    def forward(ctx, x2d, pos2d, prm2d, B, P, G, n1w, n1b, wqkv, bqkv, wproj, bproj, n2w, n2b, w1, b1, w2, b2, heads, eps):
        D = x2d.shape[1]
        hd = D // heads
        n1p, _, meanp, rstdp = layernorm_fwd(_f32c(prm2d), None, n1w, n1b, eps, want_stats=True)
        kvp = gemm(n1p, wqkv[D:], True, True, bias=(bqkv[D:] if bqkv is not None else None))
        n1x, xin, mean1, rstd1 = layernorm_fwd(_f32c(x2d), _f32c(pos2d), n1w, n1b, eps, want_stats=True)
        qkvx = gemm(n1x, wqkv, True, True, bias=bqkv)
        att, lse = attention_fwd_prefix(kvp, P, qkvx, G, B, heads, hd, want_lse=True)
        x1 = gemm(att, wproj, True, True, bias=bproj, res=xin)
        n2, _, mean2, rstd2 = layernorm_fwd(x1, None, n2w, n2b, eps, want_stats=True)
        hpre = torch.empty(B * G, w1.shape[0], dtype=torch.float32, device=x2d.device)
        a = gemm(n2, w1, True, True, bias=b1, act=EPI_GELU, aux=hpre)
        x2 = gemm(a, w2, True, True, bias=b2, res=x1)
        ctx.save_for_backward(prm2d, meanp, rstdp, kvp, xin, mean1, rstd1, qkvx, att, lse, x1, mean2, rstd2, hpre,
                              n1w, wqkv, wproj, n2w, w1, w2)
        ctx.dims = (B, P, G, D, heads, hd)
        return x2

    @staticmethod
    def backward(ctx, dx2):
        (prm2d, meanp, rstdp, kvp, xin, mean1, rstd1, qkvx, att, lse, x1, mean2, rstd2, hpre,
         n1w, wqkv, wproj, n2w, w1, w2) = ctx.saved_tensors
        B, P, G, D, heads, hd = ctx.dims
        dx2 = _f32c(dx2)
        dh = gemm(dx2, w2, True, False, act=EPI_MUL_GELU_GRAD, aux=hpre)
        dn2 = gemm(dh, w1, True, False)
        dx1, _, _ = layernorm_bwd(dn2, x1, n2w, mean2, rstd2, dres=dx2, want_params=False)
        datt = gemm(dx1, wproj, True, False)
        dkvp, dqkvx = attention_bwd_prefix(kvp, P, qkvx, G, att, datt, lse, B, heads, hd)
        dn1x = gemm(dqkvx, wqkv, True, False)
        dxin, _, _ = layernorm_bwd(dn1x, xin, n1w, mean1, rstd1, dres=dx1, want_params=False)
        dn1p = gemm(dkvp, wqkv[D:], True, False)
        dprm, _, _ = layernorm_bwd(dn1p, prm2d, n1w, meanp, rstdp, dres=None, want_params=False)
        return (dxin, dxin, dprm) + (None,) * 17


class PromptRowsFn(torch.autograd.Function):
    """prompt rows of a trained prompt layer: y[b*P+p, :] = dropout(tok[p, :]) + ppos[p, :] (models/dvae.py:485-498, 556-566), one launch per
    direction.  mask: 0/1 keep mask [B, P, D] (injected / recorded draws) or None -> in-kernel Philox(seed), regenerated in the backward."""

    @staticmethod
    def forward(ctx, tok, ppos, B, drop_p, seed, mask):
        P, D = tok.shape
        tok, ppos = _f32c(tok), _f32c(ppos)
        mask = _f32c(mask).reshape(B * P, D) if mask is not None else None
        y = torch.empty(B * P, D, dtype=torch.float32, device=tok.device)
        check(lib.act_prompt_rows_fwd_f32(ptr(tok), ptr(ppos), ptr(mask), B, P, D, float(drop_p), int(seed), ptr(y), stream()), "act_prompt_rows_fwd_f32")
        ctx.save_for_backward(mask)
        ctx.cfg = (B, P, D, float(drop_p), int(seed))
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        B, P, D, drop_p, seed = ctx.cfg
        dy = _f32c(dy)
        dtok = torch.empty(P, D, dtype=torch.float32, device=dy.device); dppos = torch.empty_like(dtok)
        check(lib.act_prompt_rows_bwd_f32(ptr(dy), ptr(mask), B, P, D, drop_p, seed, ptr(dtok), ptr(dppos), stream()), "act_prompt_rows_bwd_f32")
        return dtok, dppos, None, None, None, None


def prompt_rows(tok, ppos, B, drop_p=0.0, seed=0, mask=None):
    return PromptRowsFn.apply(tok, ppos, B, drop_p, seed, mask)


def prompt_layernorm(tok, ppos, B, drop_p, seed, gamma, beta, eps, seed_dev=None):
    """LN(dropout(tok) + ppos) for the B x P prompt rows of one layer of the frozen teacher, dropout mask from in-kernel Philox."""
    P, D = tok.shape
    y = torch.empty(B * P, D, dtype=torch.float32, device=tok.device)
    check(lib.act_prompt_layernorm_fwd_f32(ptr(_f32c(tok)), ptr(_f32c(ppos)), B, P, D, float(drop_p), int(seed), ptr(seed_dev), ptr(gamma), ptr(beta),
                                           float(eps), ptr(y), stream()), "act_prompt_layernorm_fwd_f32")
    return y


_E_UNSUPPORTED = -3


def prompt_kv(tok, ppos, B, drop_p, seed, gamma, beta, eps, w, bias=None, seed_dev=None):
    """LN(dropout(tok) + ppos) . w^T + bias for the B x P prompt rows of one layer of the frozen teacher, [B*P, N]: rows and mask of prompt_layernorm;
    w [N, D] = the K,V rows of the qkv Linear.  One small product for the cloud-independent part + a sparse walk over the dropped channels
    (csrc/prompt_kv.hip); a shape that entry does not take, or ACT_PROMPT_KV_SPARSE=0, runs prompt_layernorm + the dense product."""
    P, D = tok.shape
    N = w.shape[0]
    dev = tok.device
    tok, ppos, w = _f32c(tok), _f32c(ppos), _f32c(w)
    nbytes = int(lib.act_prompt_kv_workspace(B, P, D, N))
    if nbytes:
        gemm_config(True, True, P + 2, N, D, dev, publish=True)                  # the base product's configuration, as the composite path decides it
        kvp = torch.empty(B * P, N, dtype=torch.float32, device=dev)
        scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        ws = workspace(dev)
        rc = lib.act_prompt_kv_fwd_f32(ptr(tok), ptr(ppos), B, P, D, N, float(drop_p), int(seed), ptr(seed_dev), ptr(gamma), ptr(beta), float(eps),
                                       ptr(w), ptr(bias), ptr(kvp), ptr(scratch), nbytes, ptr(ws), ws.numel() * 4, stream())
        if rc == 0:
            return kvp
        if rc != _E_UNSUPPORTED:
            check(rc, "act_prompt_kv_fwd_f32")
    n1p = prompt_layernorm(tok, ppos, B, drop_p, seed, gamma, beta, eps, seed_dev=seed_dev)
    return gemm(n1p, w, True, True, bias=bias)


def prompt_layernorm_f16_planes(tok, ppos, B, drop_p, seed, gamma, beta, eps, scale, seed_dev=None):
    """the rows of prompt_layernorm (same mask) written as f16 planes [2, B*P, D] at ``scale`` (bit-identical to split_f16x2(prompt_layernorm(...), scale))"""
    P, D = tok.shape
    planes = torch.empty(2, B * P, D, dtype=torch.float16, device=tok.device)
    check(lib.act_prompt_layernorm_fwd_f16_planes_f32(ptr(_f32c(tok)), ptr(_f32c(ppos)), B, P, D, float(drop_p), int(seed), ptr(seed_dev), ptr(gamma), ptr(beta),
                                                      float(eps), ptr(planes[0]), ptr(planes[1]), float(scale), stream()),
          "act_prompt_layernorm_fwd_f16_planes_f32")
    return planes


def prompt_kv_f16x3(tok, ppos, B, drop_p, seed, gamma, beta, eps, w_planes, w_inv_scale, a_scale, bias=None, seed_dev=None, tile=0, out=None, planes=None):
    """prompt_kv as ONE dense split-f16 product (act_prompt_kv_fwd_f16x3_f32, the default teacher's form): w_planes [2, N, D] f16 and w_inv_scale [N] as
    gemm_nt_f16x3 takes them, a_scale = the static scale of the LayerNorm rows.  ``planes``: the f16 scratch the rows are split into (>= 2 B P D elements;
    allocated when None).  -> kv [B*P, N], or None when the entry answers ACT_E_UNSUPPORTED (nothing launched, ``out`` untouched)."""
    P, D = tok.shape
    N = w_planes.shape[1]
    if out is None:
        out = torch.empty(B * P, N, dtype=torch.float32, device=tok.device)
    if planes is None:
        planes = torch.empty(2 * B * P * D, dtype=torch.float16, device=tok.device)
    rc = lib.act_prompt_kv_fwd_f16x3_f32(ptr(_f32c(tok)), ptr(_f32c(ppos)), B, P, D, N, float(drop_p), int(seed), ptr(seed_dev), ptr(gamma), ptr(beta),
                                         float(eps), ptr(w_planes[0]), ptr(w_planes[1]), ptr(w_inv_scale), float(a_scale), ptr(bias), ptr(out), ptr(planes),
                                         planes.numel(), int(tile), stream())
    if rc == _E_UNSUPPORTED:
        return None
    check(rc, "act_prompt_kv_fwd_f16x3_f32")
    return out


def block_forward_prefix_perkernel(x2d, pos2d, prm2d, B, P, G, n1w, n1b, wqkv, bqkv, wproj, bproj, n2w, n2b, w1, b1, w2, b2, heads, eps, n1p=None,
                                   kvp=None):
    """Inference-only pre-LN block on G 'patch' tokens per cloud with P extra 'prompt' tokens that act as keys/values only
    (their outputs are discarded by the caller): x2d [B*G, D] (+ pos2d), prm2d [B*P, D] = prompt + prompt_pos (or n1p = its
    LayerNorm, already computed by prompt_layernorm; or kvp [B*P, 2D] = its keys / values, already computed by prompt_kv).
    Exactly the patch-token rows of  blk(cat(prompt, x) + cat(prompt_pos, pos))  of models/dvae.py:549-571."""
    D = x2d.shape[1]
    hd = D // heads
    if kvp is None:
        if n1p is None:
            n1p, _, _, _ = layernorm_fwd(prm2d, None, n1w, n1b, eps, want_stats=False)
        kvp = gemm(n1p, wqkv[D:], True, True, bias=(bqkv[D:] if bqkv is not None else None))          # K,V of the prompts
    n1x, xin, _, _ = layernorm_fwd(x2d, pos2d, n1w, n1b, eps, want_stats=False)
    qkvx = gemm(n1x, wqkv, True, True, bias=bqkv)
    att = attention_fwd_prefix(kvp, P, qkvx, G, B, heads, hd)
    x1 = gemm(att, wproj, True, True, bias=bproj, res=xin)
    n2, _, _, _ = layernorm_fwd(x1, None, n2w, n2b, eps, want_stats=False)
    a = gemm(n2, w1, True, True, bias=b1, act=EPI_GELU)
    return gemm(a, w2, True, True, bias=b2, res=x1)


# ---- dense per-point prediction (csrc/seg.hip): log-softmax, weighted NLL, confusion matrix ------------------------------------------------
class LogSoftmaxFn(torch.autograd.Function):
    """F.log_softmax over the last dim of rows [R,C], C <= 64"""

    @staticmethod
    def forward(ctx, z):
        z = _f32c(z)
        R, C = z.shape
        out = torch.empty_like(z)
        check(lib.act_log_softmax_fwd_f32(ptr(z), R, C, ptr(out), stream()), "act_log_softmax_fwd_f32")
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        R, C = out.shape
        dz = torch.empty_like(out)
        check(lib.act_log_softmax_bwd_f32(ptr(out), ptr(_f32c(g)), R, C, ptr(dz), stream()), "act_log_softmax_bwd_f32")
        return dz


def log_softmax(z):
    return LogSoftmaxFn.apply(z)


class NllWeightedFn(torch.autograd.Function):
    """F.nll_loss(logp, target, weight) (weighted mean) + the count of rows whose arg-max equals the target (int64, on the device)"""

    @staticmethod
    def forward(ctx, logp, target, weight):
        logp = _f32c(logp)
        R, C = logp.shape
        dev = logp.device
        tgt = target.to(torch.int64).contiguous()
        wt = _f32c(weight) if weight is not None else None
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        wsum = torch.empty(1, dtype=torch.float32, device=dev)
        correct = torch.empty(1, dtype=torch.int64, device=dev)
        ws = workspace(dev, lib.act_nll_weighted_workspace(R))
        check(lib.act_nll_weighted_fwd_f32(ptr(logp), ptr(tgt), ptr(wt), R, C, ptr(loss), ptr(wsum), ptr(correct), ptr(ws), ws.numel() * 4,
                                           stream()), "act_nll_weighted_fwd_f32")
        ctx.save_for_backward(tgt, wt, wsum)
        ctx.shape = (R, C)
        ctx.mark_non_differentiable(correct)
        return loss, correct

    @staticmethod
    def backward(ctx, g, _gc):
        tgt, wt, wsum = ctx.saved_tensors
        R, C = ctx.shape
        dl = torch.empty(R, C, dtype=torch.float32, device=tgt.device)
        check(lib.act_nll_weighted_bwd_f32(ptr(tgt), ptr(wt), ptr(wsum), ptr(_f32c(g).reshape(-1)), R, C, ptr(dl), stream()),
              "act_nll_weighted_bwd_f32")
        return dl, None, None


def nll_weighted(logp, target, weight=None):
    """-> (weighted-mean NLL, 0-d; number of rows with arg-max == target, int64 0-d), both on the device"""
    loss, correct = NllWeightedFn.apply(logp, target, weight)
    return loss.reshape(()), correct.reshape(())


def confusion(pred, target, C, out=None):
    """int64 [C,C] counts of (target, arg-max of pred) accumulated into ``out`` (new zeros if None); integer atomics, exact"""
    pred = _f32c(pred)
    tgt = target.to(torch.int64).contiguous()
    if out is None:
        out = torch.zeros(C, C, dtype=torch.int64, device=pred.device)
    check(lib.act_confusion_i64(ptr(pred), ptr(tgt), pred.shape[0], C, ptr(out), stream()), "act_confusion_i64")
    return out


class GroupMeanFn(torch.autograd.Function):
    """x [G*n, C] -> mean over the n rows of every group, [G, C]  (torch.mean(x, 2) of semantic_segmentation/models/pt.py)"""

    @staticmethod
    def forward(ctx, x, n):
        x = _f32c(x)
        R, C = x.shape
        out = torch.empty(R // n, C, dtype=torch.float32, device=x.device)
        check(lib.act_group_sum_f32(ptr(x), R // n, n, C, ptr(out), stream()), "act_group_sum_f32")
        ctx.n = n
        return out.div_(n)

    @staticmethod
    def backward(ctx, dout):
        G, C = dout.shape
        return (dout / ctx.n).unsqueeze(1).expand(G, ctx.n, C).reshape(G * ctx.n, C), None


def group_mean(x, n):
    return GroupMeanFn.apply(x, n)


# ---- part segmentation (csrc/partseg.hip): category label branch, category-masked evaluation -------------------------------------------
PART_COUNT_STRIDE = 16          # int32 per shape in the part-evaluation counts: [0,6) intersections, [6,12) unions, [12] category, [13] parts


class LabelBranchFn(torch.autograd.Function):
    """label_conv_cls of part_segmentation/models/pt.py: LeakyReLU(BatchNorm1d(cls [B,16] . W^T)) -> [B,64], one launch each way.  train: batch
    statistics over the B rows, running stats updated in place (momentum, unbiased variance with count B); eval: running statistics.  ``cls`` is
    taken as given (any [B,16] rows, not only one-hot) and gets no gradient; the backward gives dW, dgamma, dbeta (fixed-order sums over B,
    float64 inside the kernels, one rounding per output)."""

    @staticmethod
    def forward(ctx, cls, W, gamma, beta, running_mean, running_var, training, momentum, eps, slope):
        cls = _f32c(cls)
        B = cls.shape[0]
        if cls.dim() != 2 or cls.shape[1] != 16 or tuple(W.shape) != (64, 16):
            raise _C.ActHipError(f"label branch: expected cls [B,16] and W [64,16], got {tuple(cls.shape)} / {tuple(W.shape)}")
        if training and B < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {[B, 16, 1]}")
        dev = cls.device
        W = _f32c(W)
        y = torch.empty(B, 64, dtype=torch.float32, device=dev)
        check(lib.act_label_branch_fwd_f32(ptr(cls), ptr(W), ptr(gamma), ptr(beta), B, int(training), float(eps), float(momentum), float(slope),
                                           ptr(running_mean), ptr(running_var), ptr(y), stream()), "act_label_branch_fwd_f32")
        ctx.save_for_backward(cls, W, gamma, beta)
        ctx.training, ctx.slope, ctx.eps = training, float(slope), float(eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        cls, W, gamma, beta = ctx.saved_tensors
        if not ctx.training:
            raise NotImplementedError("label branch backward in eval mode is off the training path")
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("label branch: the category rows are constants (no gradient)")
        B = cls.shape[0]
        dW = torch.empty(64, 16, dtype=torch.float32, device=cls.device)
        dg = torch.empty(64, dtype=torch.float32, device=cls.device)
        db = torch.empty(64, dtype=torch.float32, device=cls.device)
        check(lib.act_label_branch_bwd_f32(ptr(cls), ptr(W), ptr(gamma), ptr(beta), ptr(_f32c(dy)), B, ctx.eps, ctx.slope, ptr(dW), ptr(dg), ptr(db),
                                           stream()), "act_label_branch_bwd_f32")
        return None, dW, dg, db, None, None, None, None, None, None


def label_branch(cls, conv, bn, act, training):
    """nn.Sequential(Conv1d(16, 64, 1, bias=False), BatchNorm1d(64), LeakyReLU(slope)) on cls [B,16] with the modules' parameters / buffers"""
    if training and bn.num_batches_tracked is not None and cls.shape[0] >= 2:
        bn.num_batches_tracked.add_(1)
    return LabelBranchFn.apply(cls, conv.weight.view(64, 16), bn.weight, bn.bias, bn.running_mean, bn.running_var, training, bn.momentum, bn.eps,
                               act.negative_slope)


def part_tables(seg_classes, num_part=50, device=None):
    """{category: [parts]} -> (part -> category int32 [num_part], category -> first part int32 [ncat + 1]) with the categories in sorted
    order (the order of synsetoffset2category.txt); every category's parts must be one contiguous range"""
    cats = sorted(seg_classes)
    p2c = torch.full((num_part,), -1, dtype=torch.int32)
    first = [0]
    for ci, c in enumerate(cats):
        parts = sorted(seg_classes[c])
        if parts != list(range(first[-1], first[-1] + len(parts))):
            raise ValueError(f"part ranges must be contiguous in category order: {c} {parts}")
        p2c[parts] = ci
        first.append(first[-1] + len(parts))
    return p2c.to(device), torch.tensor(first, dtype=torch.int32, device=device)


_PART_TABLES = {}


def partseg_eval(logp, target, counts, seen, correct, shape_offset, pred=None, tables=None):
    """category-masked evaluation of one batch (main.py:235-299): logp [B,N,P] (or [B*N,P]) log-probs, target [B,N] int.  Writes the per-shape
    int32 records counts[shape_offset : shape_offset + B] (counts [S,16]: intersections, unions, category, parts), adds the per-part int64
    seen / correct counts ([P]) in place, and writes the masked arg-max into ``pred`` (int32 [B*N]) when given.  ``tables``: part_tables(...)
    (default: the ShapeNetPart categories of datasets.ShapeNetPartDataset.seg_classes)."""
    if target.dim() != 2:
        raise _C.ActHipError("partseg_eval: target must be [B, N]")
    B, N = target.shape
    P = logp.shape[-1]
    lp = _f32c(logp).reshape(B * N, P)
    tgt = target.to(torch.int64).contiguous()
    if tables is None:
        key = lp.device
        if key not in _PART_TABLES:
            from .datasets.ShapeNetPartDataset import seg_classes
            _PART_TABLES[key] = part_tables(seg_classes, device=lp.device)
        tables = _PART_TABLES[key]
    p2c, first = tables
    if p2c.numel() != P:
        raise _C.ActHipError(f"partseg_eval: {P} log-prob columns against a {p2c.numel()}-part table")
    for t, width, dt in ((counts, PART_COUNT_STRIDE, torch.int32), (seen, P, torch.int64), (correct, P, torch.int64)):
        if t.dtype != dt or not t.is_contiguous() or t.shape[-1] != width or t.device != lp.device:
            raise _C.ActHipError(f"partseg_eval: bad output buffer {tuple(t.shape)} {t.dtype}")
    if pred is not None and (pred.dtype != torch.int32 or pred.numel() != B * N or not pred.is_contiguous()):
        raise _C.ActHipError("partseg_eval: pred must be int32 [B*N]")
    check(lib.act_part_eval_f32(ptr(lp), ptr(tgt), B, N, P, ptr(p2c), ptr(first), first.numel() - 1, ptr(pred), ptr(counts), int(shape_offset),
                                counts.shape[0], ptr(seen), ptr(correct), stream()), "act_part_eval_f32")
    return pred


# ---- the product forms of the block-level Functions live in act_amd.composite (one host call per module); resolved lazily so that
# either module may be imported first.  ACT_COMPOSITE=0 selects the per-kernel host path above.
def __getattr__(name):
    if name == "block_stack":
        from . import composite
        return composite.block_stack
    if name in ("BlockFn", "PrefixBlockFn", "block_forward_prefix"):
        from . import composite
        if composite.ENABLED:
            return getattr(composite, name)
        return {"BlockFn": BlockFnPerKernel, "PrefixBlockFn": PrefixBlockFnPerKernel, "block_forward_prefix": block_forward_prefix_perkernel}[name]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# ---- whole-room sliding-window testing (csrc/wholescene.hip): membership, keyed row build, gather, vote, finish -------------------------------
def _i32c(t):
    return t.to(torch.int32).contiguous()


def scene_member_count(xyz, table, gx, gy):
    """room xyz float64 [P,3], block table float64 [gy*gx,6] -> (counts int32 [gx*gy], offsets int32 [gx*gy+1], workspace) on the device"""
    xyz, table = xyz.to(torch.float64).contiguous(), table.to(torch.float64).contiguous()
    P, nblk = xyz.shape[0], gx * gy
    if table.shape != (nblk, 6):
        raise _C.ActHipError(f"scene membership: table {tuple(table.shape)} is not [{nblk}, 6]")
    counts = torch.empty(nblk, dtype=torch.int32, device=xyz.device)
    offsets = torch.empty(nblk + 1, dtype=torch.int32, device=xyz.device)
    nbytes = lib.act_scene_member_workspace(P, gx, gy)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=xyz.device)
    check(lib.act_scene_member_count(ptr(xyz), P, ptr(table), gx, gy, ptr(counts), ptr(offsets), ptr(ws), ws.numel() * 4, stream()),
          "act_scene_member_count")
    return counts, offsets, ws


def scene_member_fill(xyz, table, gx, gy, offsets, total, ws):
    """-> members int32 [total]: block b's points at [offsets[b], offsets[b+1]) in increasing order (``total`` = sum of the counts, from the host)"""
    xyz, table = xyz.to(torch.float64).contiguous(), table.to(torch.float64).contiguous()
    members = torch.empty(max(int(total), 1), dtype=torch.int32, device=xyz.device)
    check(lib.act_scene_member_fill(ptr(xyz), xyz.shape[0], ptr(table), gx, gy, ptr(offsets), ptr(members), ptr(ws), ws.numel() * 4, stream()),
          "act_scene_member_fill")
    return members[:int(total)]


def scene_members(xyz, table, gx, gy):
    """np.where of every block at once -> (counts numpy int64 [gx*gy] (the one host read), offsets int32 [gx*gy+1], members int32)"""
    counts, offsets, ws = scene_member_count(xyz, table, gx, gy)
    counts_h = counts.cpu().numpy().astype(np.int64)
    return counts_h, offsets, scene_member_fill(xyz, table, gx, gy, offsets, counts_h.sum(), ws)


def scene_rows(members, offsets, block_ids, row_off, R, block_points, seed, room, vote, out=None):
    """keyed fill + shuffle of one vote -> rows int32 [R]; block_ids int32 [nb] (non-empty blocks), row_off int32 [nb+1] (device tensors)"""
    nb = block_ids.numel()
    rows = out if out is not None else torch.empty(R, dtype=torch.int32, device=members.device)
    check(lib.act_scene_rows(ptr(members), ptr(offsets), ptr(block_ids), ptr(row_off), nb, R, block_points, seed & 0xFFFFFFFF, room & 0xFFFFFFFF,
                             vote & 0xFFFFFFFF, ptr(rows), stream()), "act_scene_rows")
    return rows


def scene_gather(xyz, table, rows, block_ids, row_off, out=None):
    """-> float32 [R,3]: (x - cx, y - cy, z) of every row's point with its block's centre (float64, one rounding)"""
    R = rows.numel()
    o = out if out is not None else torch.empty(R, 3, dtype=torch.float32, device=rows.device)
    check(lib.act_scene_gather(ptr(xyz), xyz.shape[0], ptr(table), ptr(rows), ptr(block_ids), ptr(row_off), block_ids.numel(), R, ptr(o), stream()),
          "act_scene_gather")
    return o


def scene_vote(logp, rows, label, labelweights, votes):
    """votes int32 [P,C] += one vote per row of logp [n, C] (rows int32 [n]) at its arg-max, where the point's label weight is non-zero and
    finite (main_test.py add_vote)"""
    logp = _f32c(logp)
    C = logp.shape[-1]
    n = logp.numel() // C
    check(lib.act_scene_vote(ptr(logp), ptr(rows), n, votes.shape[0], C, ptr(label), ptr(labelweights), ptr(votes), stream()), "act_scene_vote")
    return votes


def scene_finish(votes, label, cm=None):
    """-> (pred int32 [P] = arg-max of the votes (ties: lowest class; none: 0), cm int64 [C,C] += (label, pred) counts)"""
    P, C = votes.shape
    if cm is None:
        cm = torch.zeros(C, C, dtype=torch.int64, device=votes.device)
    pred = torch.empty(P, dtype=torch.int32, device=votes.device)
    check(lib.act_scene_finish(ptr(votes), ptr(label), P, C, ptr(pred), ptr(cm), stream()), "act_scene_finish")
    return pred, cm


# ---- S3DIS training blocks from resident rooms (csrc/s3dis_sample.hip) ------------------------------------------------------------------------
_S3DIS_INDEX = (("xyz", torch.float64, 2), ("labels", torch.int32, 1), ("room_off", torch.int64, 1), ("grid_origin", torch.float64, 2),
                ("grid_dims", torch.int64, 2), ("cell_off", torch.int64, 1), ("cell_pts", torch.int32, 1))


def s3dis_sample_workspace(index, B):
    """int32 workspace of a batch of B items: B * max_window member slots"""
    n = lib.act_s3dis_sample_workspace(int(B), int(index.max_window))
    return torch.empty((n + 3) // 4, dtype=torch.int32, device=index.xyz.device)


def s3dis_sample(index, room_ids, item_ids, num_point, seed, epoch, center_idx=None, ws=None, validate=True):
    """one launch: a block of ``num_point`` points for every item (room_ids / item_ids int32 [B] on the device) from the resident rooms of
    ``index`` (act_amd.datasets.S3DISDevice.build_index) -> (xyz float32 [B,num_point,3], labels int64 [B,num_point], rows int32 [B,num_point],
    count, center_idx, info int32 [B]).  ``center_idx`` int32 [B] fixes every item's centre point (one attempt, accepted whatever its count).
    Bad arguments raise ValueError; ``validate`` also reads the ids back (one host synchronisation) and refuses a room id or a centre out of range."""
    for name, dtype, dim in _S3DIS_INDEX:
        t = getattr(index, name)
        if t.dtype != dtype or t.dim() != dim:
            raise ValueError(f"s3dis_sample: index.{name} must be {dtype} with {dim} dimension(s), got {t.dtype} {tuple(t.shape)}")
    R, dev = int(index.room_off.numel()) - 1, index.xyz.device
    if R <= 0 or index.xyz.shape[1] != 3 or index.labels.numel() != index.xyz.shape[0] or index.cell_pts.numel() != index.xyz.shape[0] or \
            tuple(index.grid_origin.shape) != (R, 2) or tuple(index.grid_dims.shape) != (R, 3):
        raise ValueError("s3dis_sample: the index's tensors do not describe one set of rooms")
    if int(num_point) <= 0:
        raise ValueError(f"s3dis_sample: num_point must be positive, got {num_point}")
    if not (index.block_size > 0 and index.cell > 0 and index.min_points >= 0 and 0 < index.max_tries <= 65536 and index.max_window > 0):
        raise ValueError("s3dis_sample: block_size, cell, max_tries and max_window must be positive (max_tries <= 65536), min_points >= 0")
    ids = [("room_ids", room_ids), ("item_ids", item_ids)] + ([("center_idx", center_idx)] if center_idx is not None else [])
    for name, t in ids:
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or t.device != dev:
            raise ValueError(f"s3dis_sample: {name} must be an int32 [B] tensor on {dev}")
    B = int(room_ids.numel())
    if B == 0 or any(t.numel() != B for _, t in ids):
        raise ValueError("s3dis_sample: room_ids, item_ids and center_idx must have one entry per item (B > 0)")
    if validate:
        if int(room_ids.min()) < 0 or int(room_ids.max()) >= R:
            raise ValueError(f"s3dis_sample: room id outside [0, {R})")
        if center_idx is not None:
            size = (index.room_off[1:] - index.room_off[:-1])[room_ids.long()]
            if bool(((center_idx < 0) | (center_idx >= size)).any()):
                raise ValueError("s3dis_sample: center_idx outside its room")
    if ws is None:
        ws = s3dis_sample_workspace(index, B)
    need = lib.act_s3dis_sample_workspace(B, int(index.max_window))
    if ws.dtype != torch.int32 or ws.device != dev or ws.numel() * 4 < need:
        raise ValueError(f"s3dis_sample: the workspace must be int32 on {dev} with at least {need} bytes")
    room_ids, item_ids = room_ids.contiguous(), item_ids.contiguous()
    center_idx = center_idx.contiguous() if center_idx is not None else None
    xyz = torch.empty(B, num_point, 3, dtype=torch.float32, device=dev)
    labels = torch.empty(B, num_point, dtype=torch.int64, device=dev)
    rows = torch.empty(B, num_point, dtype=torch.int32, device=dev)
    count, center, info = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    check(lib.act_s3dis_sample_f32(ptr(index.xyz), ptr(index.labels), ptr(index.room_off), R, ptr(index.grid_origin), ptr(index.grid_dims),
                                   ptr(index.cell_off), ptr(index.cell_pts), float(index.block_size), float(index.cell), int(index.min_points),
                                   int(index.max_tries), int(index.max_window), ptr(room_ids), ptr(item_ids), ptr(center_idx), B, int(num_point),
                                   int(seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, ptr(xyz), ptr(labels), ptr(rows), ptr(count), ptr(center),
                                   ptr(info), ptr(ws), ws.numel() * 4, stream()), "act_s3dis_sample_f32")
    return xyz, labels, rows, count, center, info


# ---- object-dataset batches from a resident split (csrc/cloud_sample.hip) ----------------------------------------------------------------------
CLOUD_PERMUTE, CLOUD_NORMALIZE = 1, 2


def cloud_sample(clouds, item_ids, draw_ids, n, seed, epoch, permute=True, normalize=True, want_rows=False, validate=True):
    """one launch: out float32 [B,n,C] from the resident ``clouds`` float32 [M,N,C] (C = 3 or 6, xyz first).  Item b reads cloud item_ids[b]
    with draws keyed by (seed, epoch, draw_ids[b]) (both int32 [B] on the device).  ``permute``: n distinct rows in random order (else rows
    0 .. n-1); ``normalize``: numpy's pc_norm of xyz, bit for bit.  ``want_rows`` -> (out, src_rows int32 [B,n]).  Bad arguments raise ValueError;
    ``validate`` also reads the item ids back (one host synchronisation) and refuses one outside [0, M)."""
    if not torch.is_tensor(clouds) or not clouds.is_cuda or clouds.dtype != torch.float32 or clouds.dim() != 3:
        raise ValueError("cloud_sample: clouds must be a float32 [M,N,C] tensor on the GPU")
    M, N, C = clouds.shape
    dev = clouds.device
    if C not in (3, 6) or M < 1 or N < 1:
        raise ValueError(f"cloud_sample: clouds must be [M,N,3] or [M,N,6] with M, N > 0, got {tuple(clouds.shape)}")
    n = int(n)
    if n < 1 or n > N or n > lib.act_cloud_sample_max_points():
        raise ValueError(f"cloud_sample: n must be in [1, min(N, {lib.act_cloud_sample_max_points()})], got n = {n} with N = {N}")
    for name, t in (("item_ids", item_ids), ("draw_ids", draw_ids)):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or t.device != dev:
            raise ValueError(f"cloud_sample: {name} must be an int32 [B] tensor on {dev}")
    B = int(item_ids.numel())
    if B < 1 or draw_ids.numel() != B:
        raise ValueError("cloud_sample: item_ids and draw_ids must have one entry per item (B > 0)")
    if validate and (int(item_ids.min()) < 0 or int(item_ids.max()) >= M):
        raise ValueError(f"cloud_sample: item id outside [0, {M})")
    clouds, item_ids, draw_ids = clouds.contiguous(), item_ids.contiguous(), draw_ids.contiguous()
    out = torch.empty(B, n, C, dtype=torch.float32, device=dev)
    rows = torch.empty(B, n, dtype=torch.int32, device=dev) if want_rows else None
    flags = (CLOUD_PERMUTE if permute else 0) | (CLOUD_NORMALIZE if normalize else 0)
    rc = lib.act_cloud_sample_f32(ptr(clouds), M, N, C, ptr(item_ids), ptr(draw_ids), B, n, int(seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, flags,
                                  ptr(out), ptr(rows), stream())
    if rc == -1:
        raise ValueError("cloud_sample: act_cloud_sample_f32 refused the shape")
    check(rc, "act_cloud_sample_f32")
    return (out, rows) if want_rows else out


# ---- Stage-I reconstruction evaluation (csrc/recon_eval.hip): four Chamfer losses, CDL1 / CDL2 with ignore_zeros, F-Score counts, one row per cloud ----
RECON_FIELDS = 12
(RECON_SPARSE_L1, RECON_SPARSE_L2, RECON_DENSE_L1, RECON_DENSE_L2, RECON_CDL1, RECON_CDL2, RECON_PRECISION_HITS, RECON_RECALL_HITS, RECON_FSCORE,
 RECON_NZ_DENSE, RECON_NZ_GT) = range(11)


def recon_eval(coarse, dense, gt, out, row0, th=0.01):
    """coarse [B,nc,3], dense [B,nd,3], gt [B,N,3] float32 -> rows out[row0 : row0 + B] of the float64 [rows, RECON_FIELDS] device buffer ``out``
    (field order: the RECON_* indices; values unscaled, see include/act_hip.h).  One launch; nothing outside those rows is written."""
    for t in (coarse, dense, gt):
        if not t.is_cuda:
            raise _C.ActHipError("act_amd kernels run on the GPU only (got a CPU tensor); there is no CPU fallback")
        if t.dtype != torch.float32 or t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] != gt.shape[0]:
            raise _C.ActHipError(f"recon_eval: expected float32 [B, n, 3] clouds of one batch size, got {tuple(t.shape)} {t.dtype}")
    if not out.is_cuda or out.dtype != torch.float64 or out.dim() != 2 or out.shape[1] != RECON_FIELDS or not out.is_contiguous() \
            or out.device != gt.device:
        raise _C.ActHipError(f"recon_eval: out must be a contiguous float64 [rows, {RECON_FIELDS}] tensor on the clouds' device")
    coarse, dense, gt = coarse.contiguous(), dense.contiguous(), gt.contiguous()
    B = gt.shape[0]
    check(lib.act_recon_eval_f32(ptr(coarse), ptr(dense), ptr(gt), B, coarse.shape[1], dense.shape[1], gt.shape[1], float(th), ptr(out), int(row0),
                                 out.shape[0], stream()), "act_recon_eval_f32")
    return out


# ---- linear-SVM validation of pretrained features (csrc/svm.hip): scores, hinge, transposed product, one batched Newton iteration ----------------
SVM_MAX_CLASSES = 64


def _svm_rows(x, name):
    if not x.is_cuda:
        raise _C.ActHipError("act_amd kernels run on the GPU only (got a CPU tensor); there is no CPU fallback")
    if x.dtype != torch.float32 or x.dim() != 2:
        raise _C.ActHipError(f"{name}: expected a float32 matrix, got {tuple(x.shape)} {x.dtype}")
    return x.contiguous()


def _svm_ids(t, n, name):
    if not t.is_cuda:
        raise _C.ActHipError("act_amd kernels run on the GPU only (got a CPU tensor); there is no CPU fallback")
    if t.dim() != 1 or t.numel() != n or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise _C.ActHipError(f"{name}: expected {n} integers, got {tuple(t.shape)} {t.dtype}")
    return t.to(torch.int64).contiguous()


def _svm_workspace(device, nbytes):
    """the stream's scratch buffer; its base address is 256-byte aligned (caching allocator)"""
    return workspace(device, max(int(nbytes), 4))


def svm_scores(x, w, b=None, mask=None, out=None):
    """x [N,D] . w [K,D]^T (+ b [K]) -> [N,K]; ``mask`` [N,K]: zero where mask == 0 (K <= 64)"""
    x, w = _svm_rows(x, "svm_scores x"), _svm_rows(w, "svm_scores w")
    (N, D), K = x.shape, w.shape[0]
    if w.shape[1] != D or (b is not None and (b.dtype != torch.float32 or b.numel() != K)) or \
            (mask is not None and (mask.dtype != torch.float32 or tuple(mask.shape) != (N, K))):
        raise _C.ActHipError("svm_scores: operand shapes do not agree")
    if out is None:
        out = torch.empty(N, K, dtype=torch.float32, device=x.device)
    check(lib.act_svm_scores_f32(ptr(x), ptr(w), ptr(b.contiguous() if b is not None else None), ptr(mask.contiguous() if mask is not None else None),
                                 N, D, K, ptr(out), stream()), "act_svm_scores_f32")
    return out


def svm_hinge(scores, labels, classes):
    """scores fp32 [N,K], labels int [N], classes int [K] -> (R [N,K] = y max(0, 1 - y m), float64 [K] sums of h^2), y = +1 where label == class"""
    m = _svm_rows(scores, "svm_hinge scores")
    N, K = m.shape
    labels, classes = _svm_ids(labels, N, "svm_hinge labels"), _svm_ids(classes, K, "svm_hinge classes")
    R = torch.empty_like(m)
    sums = torch.empty(K, dtype=torch.float64, device=m.device)
    ws = _svm_workspace(m.device, lib.act_svm_hinge_workspace(N, K))
    check(lib.act_svm_hinge_f32(ptr(m), ptr(labels), ptr(classes), N, K, ptr(R), ptr(sums), ptr(ws), ws.numel() * 4, stream()), "act_svm_hinge_f32")
    return R, sums


def svm_tprod(p, x):
    """p [N,K], x [N,D] -> (p^T . x [K,D], column sums of p [K])"""
    p, x = _svm_rows(p, "svm_tprod p"), _svm_rows(x, "svm_tprod x")
    (N, K), D = p.shape, x.shape[1]
    if x.shape[0] != N:
        raise _C.ActHipError("svm_tprod: row counts differ")
    out = torch.empty(K, D, dtype=torch.float32, device=x.device)
    colsum = torch.empty(K, dtype=torch.float32, device=x.device)
    ws = _svm_workspace(x.device, lib.act_svm_tprod_workspace(N, D, K))
    check(lib.act_svm_tprod_f32(ptr(p), ptr(x), N, D, K, ptr(out), ptr(colsum), ptr(ws), ws.numel() * 4, stream()), "act_svm_tprod_f32")
    return out, colsum


def svm_state(K, device):
    """fresh solver state: (istate int32 [3,K]: flag, Newton steps, CG iterations; dstate float64 [2,K]: objective, gradient norm)"""
    return torch.zeros(3, K, dtype=torch.int32, device=device), torch.zeros(2, K, dtype=torch.float64, device=device)


def svm_newton(x, labels, classes, W, b, istate, dstate, C=1.0, tol=1e-4, max_cg=60):
    """one Newton iteration of every class, in place on W [K,D], b [K] and the state of svm_state (see include/act_hip.h); no host read"""
    N, D = x.shape
    K = W.shape[0]
    ws = _svm_workspace(x.device, lib.act_svm_newton_workspace(N, D, K))
    check(lib.act_svm_newton_f32(ptr(x), ptr(labels), ptr(classes), N, D, K, float(C), float(tol), int(max_cg), ptr(W), ptr(b), ptr(istate),
                                 ptr(dstate), ptr(ws), ws.numel() * 4, stream()), "act_svm_newton_f32")


# ---- exact t-SNE of classifier features (csrc/tsne.hip): kNN graph, perplexity search, CSR symmetrisation, steps, KL, PCA initialisation ----------
TSNE_MAX_NEIGHBORS = 1024
TSNE_MAX_PCA_DIM = 1024


def _tsne_i32(t, shape, name):
    if not t.is_cuda:
        raise _C.ActHipError("act_amd kernels run on the GPU only (got a CPU tensor); there is no CPU fallback")
    if t.dtype != torch.int32 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise _C.ActHipError(f"{name}: expected int32 {shape if shape is not None else ''}, got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


def _tsne_state(t, N, name):
    """Y / update / gains: updated in place, so no copy is made for the caller"""
    if not t.is_cuda:
        raise _C.ActHipError("act_amd kernels run on the GPU only (got a CPU tensor); there is no CPU fallback")
    if t.dtype != torch.float32 or tuple(t.shape) != (N, 2) or not t.is_contiguous():
        raise _C.ActHipError(f"{name}: expected a contiguous float32 [{N}, 2], got {tuple(t.shape)} {t.dtype}")
    return t


def tsne_knn_cosine(x, k):
    """x [N,D] -> (idx int32 [N,k], dist [N,k]): the k nearest other rows under 1 - cos, ascending, ties towards the lower index; a zero row
    has distance 1 to every row"""
    x = _svm_rows(x, "tsne_knn_cosine x")
    N, D = x.shape
    k = int(k)
    if not 1 <= k <= min(N - 1, TSNE_MAX_NEIGHBORS):
        raise _C.ActHipError(f"tsne_knn_cosine: k = {k} outside 1 .. min(N - 1, {TSNE_MAX_NEIGHBORS}) for N = {N}")
    idx = torch.empty(N, k, dtype=torch.int32, device=x.device)
    dist = torch.empty(N, k, dtype=torch.float32, device=x.device)
    ws = _svm_workspace(x.device, lib.act_tsne_knn_workspace(N, D))
    check(lib.act_tsne_knn_cosine_f32(ptr(x), N, D, k, ptr(idx), ptr(dist), ptr(ws), ws.numel() * 4, stream()), "act_tsne_knn_cosine_f32")
    return idx, dist


def tsne_conditional_p(dist, perplexity, want_beta=False):
    """dist [N,k] -> p [N,k], every row summing to 1 with entropy log(perplexity) (bisection on beta in float64)"""
    dist = _svm_rows(dist, "tsne_conditional_p dist")
    N, k = dist.shape
    p = torch.empty_like(dist)
    beta = torch.empty(N, dtype=torch.float32, device=dist.device) if want_beta else None
    check(lib.act_tsne_conditional_p_f32(ptr(dist), N, k, float(perplexity), ptr(p), ptr(beta), stream()), "act_tsne_conditional_p_f32")
    return (p, beta) if want_beta else p


def tsne_symmetrize(idx, p):
    """idx int32 [N,k], p [N,k] -> CSR (indptr int32 [N+1], indices int32 [nnz], values [nnz]) of (P + P^T) / 2N, columns ascending within a row.
    One host read: the number of entries"""
    p = _svm_rows(p, "tsne_symmetrize p")
    N, k = p.shape
    idx = _tsne_i32(idx, (N, k), "tsne_symmetrize idx")
    cap = 2 * N * k
    indptr = torch.empty(N + 1, dtype=torch.int32, device=p.device)
    indices = torch.empty(cap, dtype=torch.int32, device=p.device)
    values = torch.empty(cap, dtype=torch.float32, device=p.device)
    ws = _svm_workspace(p.device, lib.act_tsne_symmetrize_workspace(N, k))
    check(lib.act_tsne_symmetrize_f32(ptr(idx), ptr(p), N, k, ptr(indptr), ptr(indices), ptr(values), cap, ptr(ws), ws.numel() * 4, stream()),
          "act_tsne_symmetrize_f32")
    nnz = int(indptr[N])
    return indptr, indices[:nnz].clone(), values[:nnz].clone()


def _tsne_csr(csr, N, name):
    indptr, indices, values = csr
    indptr = _tsne_i32(indptr, (N + 1,), name + " indptr")
    indices = _tsne_i32(indices, None, name + " indices")
    if values.dtype != torch.float32 or values.shape != indices.shape or not values.is_cuda:
        raise _C.ActHipError(f"{name}: values must be float32 {tuple(indices.shape)} on the device")
    return indptr, indices, values.contiguous()


def tsne_steps(csr, Y, update, gains, n, exaggeration, momentum, lr):
    """n optimisation steps inside one C call, in place on Y, update, gains [N,2]; nothing is read back"""
    N = Y.shape[0]
    indptr, indices, values = _tsne_csr(csr, N, "tsne_steps")
    for t, nm in ((Y, "Y"), (update, "update"), (gains, "gains")):
        _tsne_state(t, N, "tsne_steps " + nm)
    ws = _svm_workspace(Y.device, lib.act_tsne_step_workspace(N))
    check(lib.act_tsne_steps_f32(ptr(indptr), ptr(indices), ptr(values), N, int(n), float(exaggeration), float(momentum), float(lr), ptr(Y),
                                 ptr(update), ptr(gains), ptr(ws), ws.numel() * 4, stream()), "act_tsne_steps_f32")
    return Y


def tsne_step(csr, Y, update, gains, exaggeration, momentum, lr):
    """one optimisation step (exact all-pairs repulsion, attraction along the CSR rows, gains, momentum, centring), in place"""
    N = Y.shape[0]
    indptr, indices, values = _tsne_csr(csr, N, "tsne_step")
    for t, nm in ((Y, "Y"), (update, "update"), (gains, "gains")):
        _tsne_state(t, N, "tsne_step " + nm)
    ws = _svm_workspace(Y.device, lib.act_tsne_step_workspace(N))
    check(lib.act_tsne_step_f32(ptr(indptr), ptr(indices), ptr(values), N, float(exaggeration), float(momentum), float(lr), ptr(Y), ptr(update),
                                ptr(gains), ptr(ws), ws.numel() * 4, stream()), "act_tsne_step_f32")
    return Y


def tsne_kl(csr, Y, out=None):
    """KL(P || Q) of the embedding Y [N,2] -> one device double (read it when the number is wanted)"""
    N = Y.shape[0]
    indptr, indices, values = _tsne_csr(csr, N, "tsne_kl")
    _tsne_state(Y, N, "tsne_kl Y")
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=Y.device)
    ws = _svm_workspace(Y.device, lib.act_tsne_step_workspace(N))
    check(lib.act_tsne_kl_f32(ptr(indptr), ptr(indices), ptr(values), ptr(Y), N, ptr(out), ptr(ws), ws.numel() * 4, stream()), "act_tsne_kl_f32")
    return out


def tsne_pca_init(x, want_info=False):
    """x [N,D] -> Y0 [N,2]: projection on the two leading principal axes, column 0 scaled to standard deviation 1e-4.  info float64 [4]: the two
    eigenvalues of the centred Gram matrix, the sweeps of the orthogonal iteration, its last subspace change"""
    x = _svm_rows(x, "tsne_pca_init x")
    N, D = x.shape
    if not 2 <= D <= TSNE_MAX_PCA_DIM or N < 2:
        raise _C.ActHipError(f"tsne_pca_init: needs N >= 2 and 2 <= D <= {TSNE_MAX_PCA_DIM}, got {tuple(x.shape)}")
    Y = torch.empty(N, 2, dtype=torch.float32, device=x.device)
    info = torch.empty(4, dtype=torch.float64, device=x.device)
    ws = _svm_workspace(x.device, lib.act_tsne_pca_workspace(N, D))
    check(lib.act_tsne_pca_init_f32(ptr(x), N, D, ptr(Y), ptr(info), ptr(ws), ws.numel() * 4, stream()), "act_tsne_pca_init_f32")
    return (Y, info) if want_info else Y


# ---- weighted k-NN validation of frozen features (csrc/knn_probe.hip): fused similarity + streaming top-k, weighted class vote -------------------
KNN_PROBE_MAX_K = 256
KNN_PROBE_MAX_CLASSES = 1024
KNN_PROBE_MAX_KS = 16


def knn_probe_normalize(x):
    """x [N,D] -> x / max(|x|, 1e-12) per row (a zero row stays zero)"""
    x = _svm_rows(x, "knn_probe_normalize x")
    out = torch.empty_like(x)
    check(lib.act_knn_probe_normalize_f32(ptr(x), x.shape[0], x.shape[1], ptr(out), stream()), "act_knn_probe_normalize_f32")
    return out


def knn_probe_search(q, bank, k, normalize=True, exclude_self=False, splits=0):
    """q [Nq,D], bank [Nb,D] -> (sim fp32 [Nq,k], idx int32 [Nq,k]): the k most similar bank rows of every query, best first, ties towards the
    lower bank index; ``exclude_self``: query i never selects bank row i; ``splits``: bank ranges searched separately (0 = chosen by the library;
    the result does not depend on it)"""
    q, bank = _svm_rows(q, "knn_probe_search q"), _svm_rows(bank, "knn_probe_search bank")
    (Nq, D), Nb = q.shape, bank.shape[0]
    k = int(k)
    if bank.shape[1] != D or Nq < 1 or D < 1:
        raise _C.ActHipError(f"knn_probe_search: q {tuple(q.shape)} and bank {tuple(bank.shape)} do not agree")
    if not 1 <= k <= min(Nb - bool(exclude_self), KNN_PROBE_MAX_K):
        raise _C.ActHipError(f"knn_probe_search: k = {k} outside 1 .. min({Nb} bank rows - {int(bool(exclude_self))}, {KNN_PROBE_MAX_K})")
    idx = torch.empty(Nq, k, dtype=torch.int32, device=q.device)
    sim = torch.empty(Nq, k, dtype=torch.float32, device=q.device)
    nbytes = lib.act_knn_probe_workspace(Nq, Nb, D, k, int(splits))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=q.device)      # the padded copy of a large bank outgrows the persistent scratch
    check(lib.act_knn_probe_search_f32(ptr(q), Nq, ptr(bank), Nb, D, k, int(bool(normalize)), int(bool(exclude_self)), int(splits), ptr(idx),
                                       ptr(sim), ptr(ws), ws.numel() * 4, stream()), "act_knn_probe_search_f32")
    return sim, idx


def knn_probe_vote(sim, idx, bank_cls, num_classes, ks, T, q_cls=None, want_scores=True):
    """sim / idx [Nq,kmax] of knn_probe_search, bank_cls int32 [Nb] class indices, ks ascending -> (scores fp32 [Nq,len(ks),C] or None,
    pred int64 [Nq,len(ks)] class indices, counts int64 [len(ks),2] top-1 / top-5 hits against q_cls, or None without it)"""
    sim = _svm_rows(sim, "knn_probe_vote sim")
    Nq, kmax = sim.shape
    idx = _tsne_i32(idx, (Nq, kmax), "knn_probe_vote idx")
    bank_cls = _tsne_i32(bank_cls, None, "knn_probe_vote bank_cls")
    ks = [int(v) for v in ks]
    C = int(num_classes)
    if not ks or len(ks) > KNN_PROBE_MAX_KS or ks[0] < 1 or ks[-1] > kmax or any(b <= a for a, b in zip(ks, ks[1:])):
        raise _C.ActHipError(f"knn_probe_vote: ks = {ks} must be 1 .. {KNN_PROBE_MAX_KS} ascending values in 1 .. {kmax}")
    if not 1 <= C <= KNN_PROBE_MAX_CLASSES or bank_cls.dim() != 1 or not float(T) > 0:
        raise _C.ActHipError(f"knn_probe_vote: {C} classes (supported: 1 .. {KNN_PROBE_MAX_CLASSES}), T = {T}")
    if q_cls is not None:
        q_cls = _tsne_i32(q_cls, (Nq,), "knn_probe_vote q_cls")
    scores = torch.empty(Nq, len(ks), C, dtype=torch.float32, device=sim.device) if want_scores else None
    pred = torch.empty(Nq, len(ks), dtype=torch.int64, device=sim.device)
    counts = torch.zeros(len(ks), 2, dtype=torch.int64, device=sim.device) if q_cls is not None else None
    check(lib.act_knn_probe_vote_f32(ptr(sim), ptr(idx), Nq, kmax, ptr(bank_cls), bank_cls.numel(), ptr(q_cls), C, (ctypes.c_int * len(ks))(*ks),
                                     len(ks), float(T), ptr(scores), ptr(pred), ptr(counts), stream()), "act_knn_probe_vote_f32")
    return scores, pred, counts


# ---- frozen post-LayerNorm language teacher (csrc/bert.hip) ---------------------------------------------------------------------------
def dropout_add_layernorm_fwd(t, res, gamma, beta, eps, p=0.0, seed=0, mask=None, seed_dev=None, want_rstd=True):
    """y = LN(keep o t / (1-p) + res) * gamma + beta on rows [T, D]; keep: ``mask`` (0/1 floats [T, D]) or in-kernel Philox(seed, seed_dev)."""
    t, res = _f32c(t), _f32c(res)
    T, D = t.shape
    mask = _f32c(mask).reshape(T, D) if (mask is not None and p > 0) else None
    y = torch.empty_like(t)
    rstd = torch.empty(T, dtype=torch.float32, device=t.device) if want_rstd else None
    check(lib.act_dropout_add_layernorm_fwd_f32(ptr(t), ptr(res), ptr(mask), T, D, float(p), int(seed), ptr(seed_dev), ptr(gamma), ptr(beta),
                                                float(eps), ptr(y), ptr(rstd), stream()), "act_dropout_add_layernorm_fwd_f32")
    return y, rstd


def dropout_add_layernorm_bwd(dy, y, gamma, beta, rstd, p=0.0, seed=0, mask=None, seed_dev=None):
    """-> (dt, dres) of dropout_add_layernorm_fwd; the mask is regenerated from its key (or the given one), the normalised row from y."""
    dy = _f32c(dy)
    T, D = dy.shape
    mask = _f32c(mask).reshape(T, D) if (mask is not None and p > 0) else None
    dt, dres = torch.empty_like(dy), torch.empty_like(dy)
    check(lib.act_dropout_add_layernorm_bwd_f32(ptr(dy), ptr(y), ptr(mask), T, D, float(p), int(seed), ptr(seed_dev), ptr(gamma), ptr(beta),
                                                ptr(rstd), ptr(dt), ptr(dres), stream()), "act_dropout_add_layernorm_bwd_f32")
    return dt, dres


def _attn_mask_u8(mask, B, S, H):
    if mask is None:
        return None
    if mask.dtype != torch.uint8 or tuple(mask.shape) != (B, H, S, S):
        raise _C.ActHipError(f"attention dropout mask: expected uint8 [{B}, {H}, {S}, {S}], got {mask.dtype} {tuple(mask.shape)}")
    return mask.contiguous()


def attention_dropout_fwd(qkv, B, S, H, hd, p, seed=0, mask=None, seed_dev=None, want_lse=True):
    """out = (softmax(q k^t hd^-1/2) o keep / (1-p)) v on packed qkv [B,S,3,H,hd]; keep: ``mask`` (uint8 [B,H,S,S]) or in-kernel Philox."""
    out = torch.empty(B * S, H * hd, dtype=torch.float32, device=qkv.device)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=qkv.device) if want_lse else None
    check(lib.act_attention_dropout_fwd_f32(ptr(qkv), ptr(_attn_mask_u8(mask, B, S, H)), ptr(out), ptr(lse), B, S, H, hd, float(hd) ** -0.5, float(p),
                                            int(seed), ptr(seed_dev), stream()), "act_attention_dropout_fwd_f32")
    return out, lse


def attention_dropout_bwd(qkv, out, dout, lse, B, S, H, hd, p, seed=0, mask=None, seed_dev=None):
    dqkv = torch.empty_like(qkv)
    delta = torch.empty(B, H, S, dtype=torch.float32, device=qkv.device)
    check(lib.act_attention_dropout_bwd_f32(ptr(qkv), ptr(_attn_mask_u8(mask, B, S, H)), ptr(out), ptr(_f32c(dout)), ptr(lse), ptr(delta), ptr(dqkv),
                                            B, S, H, hd, float(hd) ** -0.5, float(p), int(seed), ptr(seed_dev), stream()),
          "act_attention_dropout_bwd_f32")
    return dqkv


class BertLayerFn(torch.autograd.Function):
    """One FROZEN post-LayerNorm (BERT) layer on x [B,S,D] (reference models/dvae.py:753-754 through transformers' BertLayer):

        qkv = x Wqkv + b ; ctx = (dropout_pa(softmax(q k^t hd^-1/2))) v ; a = LN(dropout_ph(ctx Wo + bo) + x) ; y = LN(dropout_ph(gelu(a Wi + bi) Wo2 + bo2) + a)

    seeds = (attention, hidden1, hidden2) Philox seeds, masks = the same three as injected keep masks (uint8 [B,H,S,S], floats [B,S,D] twice) or None
    each; seed_dev: the device-resident counter of the no_grad teacher path.  Kept for the backward: qkv, ctx, lse, a, the GELU input, y (the
    normalised rows come back from a and y), the two rstd vectors and the seeds (injected masks as given) -- no mask is stored.  The backward produces the
    input gradient only: the weights are frozen.  Under no_grad nothing is kept.  At p_attn == 0 the attention is act_attention_fwd_f32 / _bwd_f32."""

    @staticmethod
    def forward(ctx, x, wqkv, bqkv, wo, bo, g1, b1, wi, bi, wo2, bo2, g2, b2, heads, eps, p_attn, p_hidden, seeds, masks, seed_dev):
        B, S, D = x.shape
        hd = D // heads
        x2 = _f32c(x).reshape(B * S, D)
        need_grad = ctx.needs_input_grad[0]
        m_attn, m_h1, m_h2 = masks if masks is not None else (None, None, None)
        qkv = gemm(x2, wqkv, True, True, bias=bqkv)
        if p_attn > 0:
            att, lse = attention_dropout_fwd(qkv, B, S, heads, hd, p_attn, seeds[0], m_attn, seed_dev, want_lse=need_grad)
        else:
            att, lse = attention_fwd(qkv, B, S, heads, hd, want_lse=need_grad)
        t1 = gemm(att, wo, True, True, bias=bo)
        a, rstd1 = dropout_add_layernorm_fwd(t1, x2, g1, b1, eps, p_hidden, seeds[1], m_h1, seed_dev, want_rstd=need_grad)
        hpre = torch.empty(B * S, wi.shape[0], dtype=torch.float32, device=x.device) if need_grad else None
        h = gemm(a, wi, True, True, bias=bi, act=EPI_GELU, aux=hpre)
        t2 = gemm(h, wo2, True, True, bias=bo2)
        y, rstd2 = dropout_add_layernorm_fwd(t2, a, g2, b2, eps, p_hidden, seeds[2], m_h2, seed_dev, want_rstd=need_grad)
        if need_grad:
            ctx.save_for_backward(qkv, att, lse, a, hpre, y, rstd1, rstd2, wqkv, wo, g1, b1, wi, wo2, g2, b2, m_attn,
                                  m_h1 if p_hidden > 0 else None, m_h2 if p_hidden > 0 else None, seed_dev)
            ctx.cfg = (B, S, D, heads, hd, float(p_attn), float(p_hidden), tuple(int(s) for s in seeds))
        return y.reshape(B, S, D)

    @staticmethod
    def backward(ctx, dy):
        qkv, att, lse, a, hpre, y, rstd1, rstd2, wqkv, wo, g1, b1, wi, wo2, g2, b2, m_attn, m_h1, m_h2, seed_dev = ctx.saved_tensors
        B, S, D, heads, hd, p_attn, p_hidden, seeds = ctx.cfg
        dy2 = _f32c(dy).reshape(B * S, D)
        dt2, dres2 = dropout_add_layernorm_bwd(dy2, y, g2, b2, rstd2, p_hidden, seeds[2], m_h2, seed_dev)
        dh = gemm(dt2, wo2, True, False, act=EPI_MUL_GELU_GRAD, aux=hpre)
        da = gemm(dh, wi, True, False, res=dres2)                       # + the residual branch of the second LayerNorm
        dt1, dres1 = dropout_add_layernorm_bwd(da, a, g1, b1, rstd1, p_hidden, seeds[1], m_h1, seed_dev)
        datt = gemm(dt1, wo, True, False)
        if p_attn > 0:
            dqkv = attention_dropout_bwd(qkv, att, datt, lse, B, S, heads, hd, p_attn, seeds[0], m_attn, seed_dev)
        else:
            dqkv = attention_bwd(qkv, att, datt, lse, B, S, heads, hd)
        dx = gemm(dqkv, wqkv, True, False, res=dres1)
        return (dx.reshape(B, S, D),) + (None,) * 19


def bert_layer(x, wqkv, bqkv, wo, bo, g1, b1, wi, bi, wo2, bo2, g2, b2, heads, eps=1e-12, p_attn=0.0, p_hidden=0.0, seeds=(0, 0, 0), masks=None,
               seed_dev=None):
    return BertLayerFn.apply(x, wqkv, bqkv, wo, bo, g1, b1, wi, bi, wo2, bo2, g2, b2, heads, eps, p_attn, p_hidden, seeds, masks, seed_dev)


# ---- frozen CLIP image teacher (csrc/clip.hip) -------------------------------------------------------------------------------------------
def quickgelu_fwd(pre, out=None):
    """pre * sigmoid(1.702 pre) on dense fp32 of any shape"""
    pre = _f32c(pre, "pre")
    out = torch.empty_like(pre) if out is None else out
    cols = pre.shape[-1] if pre.dim() else 1
    check(lib.act_quickgelu_fwd_f32(ptr(pre), ptr(out), pre.numel() // max(cols, 1), cols, stream()), "act_quickgelu_fwd_f32")
    return out


def quickgelu_bwd(pre, dy, out=None):
    """dy * s * (1 + 1.702 pre (1 - s)), s = sigmoid(1.702 pre); ``out`` may be ``dy`` (in place)"""
    pre, dy = _f32c(pre, "pre"), _f32c(dy, "dy")
    if dy.shape != pre.shape:
        raise _C.ActHipError(f"quickgelu_bwd: dy {tuple(dy.shape)} vs pre {tuple(pre.shape)}")
    out = torch.empty_like(pre) if out is None else out
    cols = pre.shape[-1] if pre.dim() else 1
    check(lib.act_quickgelu_bwd_f32(ptr(pre), ptr(dy), ptr(out), pre.numel() // max(cols, 1), cols, stream()), "act_quickgelu_bwd_f32")
    return out


class QuickGeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32c(x)
        ctx.save_for_backward(x)
        return quickgelu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return quickgelu_bwd(x, dy)


def quickgelu(x):
    return QuickGeluFn.apply(x)


class ClipBlockFn(torch.autograd.Function):
    """One FROZEN residual block of CLIP's visual Transformer applied to (x + pos) on x [B,S,D], batch first (reference models/dvae.py:505-506 through CLIP's
    ResidualAttentionBlock; the reference's sequence-first permutes are layout only):

        xin = x + pos ; x1 = xin + out_proj(attn(in_proj(LN1(xin)))) ; x2 = x1 + c_proj(quickgelu(c_fc(LN2(x1))))

    ``in_proj_weight`` stacks q, k, v with the heads major inside each -- timm's qkv layout -- so the packed attention kernels apply as they are.  Built from
    the entries BlockFnPerKernel uses, with c_fc under EPI_NONE and QuickGELU as its own pass (act_quickgelu_fwd_f32 / _bwd_f32).  Kept for the backward:
    what BlockFnPerKernel keeps less what only weight gradients read (the MLP activation, the LN outputs), the pre-activation included.  The backward
    produces the gradient of x and pos only: the weights are frozen.  Under no_grad nothing is kept."""

    @staticmethod
    def forward(ctx, x, pos, n1w, n1b, wqkv, bqkv, wo, bo, n2w, n2b, wfc, bfc, wproj, bproj, heads, eps):
        B, S, D = x.shape
        hd = D // heads
        x2d = _f32c(x).reshape(B * S, D)
        pos2d = _f32c(pos).reshape(B * S, D) if pos is not None else None
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        n1, xin, mean1, rstd1 = layernorm_fwd(x2d, pos2d, n1w, n1b, eps, want_stats=need_grad)
        qkv = gemm(n1, wqkv, True, True, bias=bqkv)
        att, lse = attention_fwd(qkv, B, S, heads, hd, want_lse=need_grad)
        x1 = gemm(att, wo, True, True, bias=bo, res=xin)
        n2, _, mean2, rstd2 = layernorm_fwd(x1, None, n2w, n2b, eps, want_stats=need_grad)
        hpre = gemm(n2, wfc, True, True, bias=bfc, act=EPI_NONE)
        a = quickgelu_fwd(hpre, out=None if need_grad else hpre)
        x2 = gemm(a, wproj, True, True, bias=bproj, res=x1)
        if need_grad:
            ctx.save_for_backward(xin, mean1, rstd1, qkv, att, lse, x1, mean2, rstd2, hpre, n1w, wqkv, wo, n2w, wfc, wproj)
            ctx.dims = (B, S, D, heads, hd)
            ctx.has_pos = pos is not None
        return x2.reshape(B, S, D)

    @staticmethod
    def backward(ctx, dx2):
        xin, mean1, rstd1, qkv, att, lse, x1, mean2, rstd2, hpre, n1w, wqkv, wo, n2w, wfc, wproj = ctx.saved_tensors
        B, S, D, heads, hd = ctx.dims
        dx2 = _f32c(dx2).reshape(B * S, D)
        da = gemm(dx2, wproj, True, False)
        dh = quickgelu_bwd(hpre, da, out=da)
        dn2 = gemm(dh, wfc, True, False)
        dx1, _, _ = layernorm_bwd(dn2, x1, n2w, mean2, rstd2, dres=dx2, want_params=False)
        datt = gemm(dx1, wo, True, False)
        dqkv = attention_bwd(qkv, att, datt, lse, B, S, heads, hd)
        dn1 = gemm(dqkv, wqkv, True, False)
        dxin, _, _ = layernorm_bwd(dn1, xin, n1w, mean1, rstd1, dres=dx1, want_params=False)
        dxin = dxin.reshape(B, S, D)
        return (dxin if ctx.needs_input_grad[0] else None, dxin if ctx.has_pos and ctx.needs_input_grad[1] else None) + (None,) * 14


def clip_block(x, pos, n1w, n1b, wqkv, bqkv, wo, bo, n2w, n2b, wfc, bfc, wproj, bproj, heads, eps=1e-5):
    return ClipBlockFn.apply(x, pos, n1w, n1b, wqkv, bqkv, wo, bo, n2w, n2b, wfc, bfc, wproj, bproj, heads, eps)


# ---- fused augmentation chain (csrc/augment.hip) ----------------------------------------------------------------------------------------
AUG_SCALE, AUG_TRANSLATE, AUG_SCALE_TRANSLATE, AUG_ROTATE_Y, AUG_JITTER, AUG_DROPOUT, AUG_FLIP = 1, 2, 3, 4, 5, 6, 7
AUG_GLOBAL = 1
# shape of the (up to two) injected draw tensors of each kind for a batch [B, N, 3]
_AUG_DRAW_SHAPES = {AUG_SCALE: lambda B, N: ((B, 3),), AUG_TRANSLATE: lambda B, N: ((B, 3),), AUG_SCALE_TRANSLATE: lambda B, N: ((B, 3), (B, 3)),
                    AUG_ROTATE_Y: lambda B, N: ((B,),), AUG_JITTER: lambda B, N: ((B, N, 3),), AUG_DROPOUT: lambda B, N: ((B,), (B, N)),
                    AUG_FLIP: lambda B, N: ((B, 3),)}


def augment(pc, ops, draws=None, seed=0, seed_dev=None, force_global=False):
    """An ordered chain of 1..8 augmentation ops on pc f32 [B,N,3], in place, by one launch (act_augment_f32).  ``ops``: (kind, p0, p1, p2) per op;
    ``draws`` (nullable): per op None or a tuple of the op's injected draw tensors (None entries: Philox keyed by ``seed`` and the device-resident
    counter ``seed_dev``); ``force_global``: skip the LDS staging at any N."""
    if pc.dim() != 3 or pc.shape[2] != 3 or pc.dtype != torch.float32:
        raise _C.ActHipError("augment expects a float32 tensor [B, N, 3]")
    B, N, _ = pc.shape
    table = (_C._abi.AugmentOp * max(1, len(ops)))()
    keep = []
    for i, (kind, p0, p1, p2) in enumerate(ops):
        inj = tuple(draws[i] or ()) if draws is not None and i < len(draws) else ()
        shapes = _AUG_DRAW_SHAPES.get(int(kind), lambda B, N: ())(B, N)
        ptrs = [None, None]
        for j, t in enumerate(inj[:2]):
            if t is None:
                continue
            t = torch.as_tensor(t, device=pc.device).to(torch.float32).contiguous()
            if j >= len(shapes) or tuple(t.shape) != shapes[j]:
                raise _C.ActHipError(f"augment: draw {j} of op {i} has shape {tuple(t.shape)}, expected {shapes[j] if j < len(shapes) else None}")
            keep.append(t)
            ptrs[j] = ptr(t)
        table[i].kind, table[i].p0, table[i].p1, table[i].p2 = int(kind), float(p0), float(p1), float(p2)
        table[i].draws, table[i].draws2 = ptrs
    check(lib.act_augment_f32(ptr(pc), B, N, table, len(ops), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(seed_dev), AUG_GLOBAL if force_global else 0,
                              stream()), "act_augment_f32")
    return pc


# ---- PointNet++ set abstraction (csrc/sa.hip): radius search, grouped rows and their deterministic backward -----------------------------------
def _sa_f32(t, name, shape):
    """float32 CUDA operand ``name`` whose shape matches ``shape`` (None entries are free), made contiguous"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _C.ActHipError(f"{name}: expected a CUDA tensor (the HIP kernels have no CPU fallback)")
    if t.dtype != torch.float32:
        raise _C.ActHipError(f"{name}: expected float32, got {t.dtype}")
    if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise _C.ActHipError(f"{name}: expected shape {['*' if s is None else s for s in shape]}, got {list(t.shape)}")
    return t if t.is_contiguous() else t.contiguous()


def _sa_idx(idx, name, B):
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda:
        raise _C.ActHipError(f"{name}: expected a CUDA tensor (the HIP kernels have no CPU fallback)")
    if idx.dtype not in (torch.int32, torch.int64):
        raise _C.ActHipError(f"{name}: expected int32 (or int64) indices, got {idx.dtype}")
    if idx.dim() != 3 or idx.shape[0] != B or idx.shape[1] < 1 or idx.shape[2] < 1:
        raise _C.ActHipError(f"{name}: expected shape [{B}, S, nsample], got {list(idx.shape)}")
    return _i32c(idx)


def ball_query(xyz, new_xyz, radius, nsample, inclusive=False, want_cnt=False):
    """xyz [B,N,3], new_xyz [B,S,3] -> idx int32 [B,S,nsample] (and cnt int32 [B,S] = min(hits, nsample) with ``want_cnt``): the lowest
    ``nsample`` indices within the radius in ascending order, the rest of the row repeating the first hit, zeros when nothing is in reach.
    ``inclusive=False``: d2 < r^2 (upstream pointnet2_ops); ``inclusive=True``: d2 <= r^2 (the reference's query_ball_point).  d2 is the fp32
    difference form, r^2 the fp32 product."""
    xyz = _sa_f32(xyz, "ball_query: xyz", (None, None, 3))
    B, N, _ = xyz.shape
    new_xyz = _sa_f32(new_xyz, "ball_query: new_xyz", (B, None, 3))
    S = new_xyz.shape[1]
    nsample = int(nsample)
    if nsample < 1:
        raise _C.ActHipError(f"ball_query: nsample must be >= 1, got {nsample}")
    if not float(radius) >= 0.0:
        raise _C.ActHipError(f"ball_query: radius must be >= 0, got {radius}")
    if B < 1 or N < 1 or S < 1:
        raise _C.ActHipError(f"ball_query: xyz {list(xyz.shape)} / new_xyz {list(new_xyz.shape)} must not be empty")
    idx = torch.empty(B, S, nsample, dtype=torch.int32, device=xyz.device)
    cnt = torch.empty(B, S, dtype=torch.int32, device=xyz.device) if want_cnt else None
    check(lib.act_ball_query_f32(ptr(xyz), ptr(new_xyz), B, N, S, float(radius), nsample, int(bool(inclusive)), ptr(idx), ptr(cnt), stream()),
          "act_ball_query_f32")
    return (idx, cnt) if want_cnt else idx


def _adj_workspace(dev, B, N, S, ns):
    return workspace(dev, lib.act_group_rows_bwd_workspace(B, N, S, ns))


class GroupRowsFn(torch.autograd.Function):
    """sample_and_group's gather in row form: rows [B*S*nsample, (3 if use_xyz) + D], row (b,s,j) = xyz[b,i] - new_xyz[b,s] | feat[b,i];
    the backward gathers over the inverse adjacency in ascending (s, j) order (no atomics, bit-identical run to run).  xyz, new_xyz and idx are
    constants: the cloud is a leaf, as in InterpRowsFn."""

    @staticmethod
    def forward(ctx, feat, xyz, new_xyz, idx, use_xyz):
        B, S, ns = idx.shape
        N = xyz.shape[1] if xyz is not None else feat.shape[1]
        D = 0 if feat is None else feat.shape[2]
        dev = idx.device
        rows = torch.empty(B * S * ns, (3 if use_xyz else 0) + D, dtype=torch.float32, device=dev)
        check(lib.act_group_rows_fwd_f32(ptr(xyz) if use_xyz else None, ptr(new_xyz) if use_xyz else None, ptr(feat), ptr(idx), B, N, S, ns, D,
                                         int(use_xyz), ptr(rows), stream()), "act_group_rows_fwd_f32")
        ctx.save_for_backward(idx)
        ctx.dims = (B, N, S, ns, D, int(use_xyz))
        return rows

    @staticmethod
    def backward(ctx, drows):
        (idx,) = ctx.saved_tensors
        B, N, S, ns, D, use_xyz = ctx.dims
        if D == 0 or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        drows = _f32c(drows, "group_rows: grad")
        dfeat = torch.empty(B, N, D, dtype=torch.float32, device=drows.device)
        ws = _adj_workspace(drows.device, B, N, S, ns)
        check(lib.act_group_rows_bwd_f32(ptr(drows), ptr(idx), B, N, S, ns, D, use_xyz, ptr(dfeat), ptr(ws), ws.numel() * 4, stream()),
              "act_group_rows_bwd_f32")
        return dfeat, None, None, None, None


def group_rows(xyz, new_xyz, feat, idx, use_xyz=True):
    """xyz [B,N,3], new_xyz [B,S,3], feat [B,N,D] or None, idx int [B,S,nsample] -> rows [B*S*nsample, (3 if use_xyz) + D], differentiable
    in ``feat``"""
    if feat is None and not use_xyz:
        raise _C.ActHipError("group_rows: feat is None and use_xyz is False: nothing to group")
    if use_xyz:
        xyz = _sa_f32(xyz, "group_rows: xyz", (None, None, 3))
        B, N = xyz.shape[0], xyz.shape[1]
        idx = _sa_idx(idx, "group_rows: idx", B)
        new_xyz = _sa_f32(new_xyz, "group_rows: new_xyz", (B, idx.shape[1], 3))
        if feat is not None:
            feat = _sa_f32(feat, "group_rows: feat", (B, N, None))
    else:
        feat = _sa_f32(feat, "group_rows: feat", (None, None, None))
        idx = _sa_idx(idx, "group_rows: idx", feat.shape[0])
        xyz = new_xyz = None
    if feat is not None and feat.shape[2] < 1:
        raise _C.ActHipError(f"group_rows: feat: expected at least one channel, got {list(feat.shape)}")
    return GroupRowsFn.apply(feat, xyz, new_xyz, idx, bool(use_xyz))


class GroupingOperationFn(torch.autograd.Function):
    """upstream pointnet2_ops grouping_operation: features [B,C,N], idx int32 [B,S,nsample] -> [B,C,S,nsample]; the backward sums, per point and
    channel, the incoming gradients in ascending (s, j) order (no atomics)."""

    @staticmethod
    def forward(ctx, features, idx):
        features = _sa_f32(features, "grouping_operation: features", (None, None, None))
        B, C, N = features.shape
        idx = _sa_idx(idx, "grouping_operation: idx", B)
        _, S, ns = idx.shape
        if C < 1 or N < 1:
            raise _C.ActHipError(f"grouping_operation: features: expected a non-empty [B, C, N], got {list(features.shape)}")
        out = torch.empty(B, C, S, ns, dtype=torch.float32, device=features.device)
        check(lib.act_group_gather_f32(ptr(features), ptr(idx), B, C, N, S, ns, ptr(out), stream()), "act_group_gather_f32")
        ctx.save_for_backward(idx)
        ctx.dims = (B, C, N, S, ns)
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        B, C, N, S, ns = ctx.dims
        dout = _f32c(dout, "grouping_operation: grad")
        df = torch.empty(B, C, N, dtype=torch.float32, device=dout.device)
        ws = _adj_workspace(dout.device, B, N, S, ns)
        check(lib.act_group_gather_bwd_f32(ptr(dout), ptr(idx), B, C, N, S, ns, ptr(df), ptr(ws), ws.numel() * 4, stream()),
              "act_group_gather_bwd_f32")
        return df, None


def grouping_operation(features, idx):
    return GroupingOperationFn.apply(features, idx)


# ---- three-NN feature propagation (csrc/sa.hip): search, inverse adjacency, row interpolation with skipped slots -----------------------------
def _sa_i32(t, name, shape=None, count=None):
    """int32 (or int64, converted) CUDA operand ``name`` of the given shape or element count, made contiguous"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _C.ActHipError(f"{name}: expected a CUDA tensor (the HIP kernels have no CPU fallback)")
    if t.dtype not in (torch.int32, torch.int64) or (shape is not None and tuple(t.shape) != tuple(shape)) or (
            count is not None and t.numel() != count):
        raise _C.ActHipError(f"{name}: expected int32 {list(shape) if shape is not None else '[%d entries]' % count}, got {t.dtype} {list(t.shape)}")
    return _i32c(t)


def _xyz_rows(xyz, name, R):
    """xyz [R,3] or [B,N,3] with B * N == R -> contiguous [R,3]"""
    xyz = _sa_f32(xyz, name, (None, None, 3) if isinstance(xyz, torch.Tensor) and xyz.dim() == 3 else (R, 3))
    if xyz.numel() != 3 * R:
        raise _C.ActHipError(f"{name}: expected 3 values for each of {R} rows, got {list(xyz.shape)}")
    return xyz.view(R, 3)


def three_nn(unknown, known, want_adj=True, want_d2=False):
    """unknown [B,n,3], known [B,m,3], any n >= 1 and m >= 1 -> (idx int32 [B,n,3], weight [B,n,3], adj_off int32 [B,m+1] | None, adj_ent int32
    [B,3n] | None), plus d2 [B,n,3] with ``want_d2``: the three nearest known points of every unknown point in ascending (difference-form
    distance, index) order, their normalised inverse-distance weights (semantic_segmentation/models/pointnet2_utils.py:293-299) and the inverse
    adjacency the interpolation backward gathers over.  m < 3: the missing slots carry idx 0, d2 = +inf and weight exactly 0 (the reference's
    S == 2 / S == 1 forms); the interpolation skips them."""
    unknown = _sa_f32(unknown, "three_nn: unknown", (None, None, 3))
    B, n, _ = unknown.shape
    known = _sa_f32(known, "three_nn: known", (B, None, 3))
    m = known.shape[1]
    if B < 1 or n < 1 or m < 1:
        raise _C.ActHipError(f"three_nn: unknown {list(unknown.shape)} / known {list(known.shape)} must not be empty")
    dev = unknown.device
    idx = torch.empty(B, n, 3, dtype=torch.int32, device=dev)
    w = torch.empty(B, n, 3, dtype=torch.float32, device=dev)
    d2 = torch.empty(B, n, 3, dtype=torch.float32, device=dev) if want_d2 else None
    off = torch.empty(B, m + 1, dtype=torch.int32, device=dev) if want_adj else None
    ent = torch.empty(B, 3 * n, dtype=torch.int32, device=dev) if want_adj else None
    check(lib.act_three_nn_f32(ptr(unknown), ptr(known), B, n, m, ptr(idx), ptr(w), ptr(d2), ptr(off), ptr(ent), stream()), "act_three_nn_f32")
    return (idx, w, off, ent, d2) if want_d2 else (idx, w, off, ent)


def three_adjacency(idx, m):
    """idx int [B,n,3] with values in [0,m) -> (adj_off int32 [B,m+1], adj_ent int32 [B,3n]): the inverse adjacency of caller-supplied indices"""
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda:
        raise _C.ActHipError("three_adjacency: idx: expected a CUDA tensor (the HIP kernels have no CPU fallback)")
    if idx.dtype not in (torch.int32, torch.int64) or idx.dim() != 3 or idx.shape[2] != 3 or idx.shape[0] < 1 or idx.shape[1] < 1:
        raise _C.ActHipError(f"three_adjacency: idx: expected int32 [B, n, 3], got {idx.dtype} {list(idx.shape)}")
    if int(m) < 1:
        raise _C.ActHipError(f"three_adjacency: m must be >= 1, got {m}")
    idx = _i32c(idx)
    B, n, _ = idx.shape
    off = torch.empty(B, int(m) + 1, dtype=torch.int32, device=idx.device)
    ent = torch.empty(B, 3 * n, dtype=torch.int32, device=idx.device)
    check(lib.act_three_adj_i32(ptr(idx), B, n, int(m), ptr(off), ptr(ent), stream()), "act_three_adj_i32")
    return off, ent


def interp_rows_fwd(P, idx, w, B, N, G, xyz=None, wxyz=None, bias=None):
    """P [B*G,C], any C >= 1 -> Y [B*N,C] = sum over the slots of non-zero weight of w * P[idx] (+ xyz . wxyz^T + bias)"""
    P = _sa_f32(P, "interp_rows_fwd: P", (B * G, None))
    w = _sa_f32(w, "interp_rows_fwd: weight", (B, N, 3))
    idx = _sa_i32(idx, "interp_rows_fwd: idx", shape=(B, N, 3))
    C = P.shape[1]
    if B < 1 or N < 1 or G < 1 or C < 1:
        raise _C.ActHipError("interp_rows_fwd: B, N, G and C must be >= 1")
    if wxyz is not None:
        xyz = _xyz_rows(xyz, "interp_rows_fwd: xyz", B * N)
        wxyz = _sa_f32(wxyz, "interp_rows_fwd: wxyz", (C, 3))
    if bias is not None:
        bias = _sa_f32(bias, "interp_rows_fwd: bias", (C,))
    Y = torch.empty(B * N, C, dtype=torch.float32, device=P.device)
    check(lib.act_interp_rows_fwd_f32(ptr(P), ptr(idx), ptr(w), ptr(xyz) if wxyz is not None else None, ptr(wxyz), ptr(bias), B, N, G, C, ptr(Y),
                                      stream()), "act_interp_rows_fwd_f32")
    return Y


def interp_rows_bwd(dY, off, ent, w, B, N, G):
    dY = _sa_f32(dY, "interp_rows_bwd: dY", (B * N, None))
    w = _sa_f32(w, "interp_rows_bwd: weight", (B, N, 3))
    off = _sa_i32(off, "interp_rows_bwd: adj_off", count=B * (G + 1))
    ent = _sa_i32(ent, "interp_rows_bwd: adj_ent", count=3 * B * N)
    C = dY.shape[1]
    dP = torch.empty(B * G, C, dtype=torch.float32, device=dY.device)
    check(lib.act_interp_rows_bwd_f32(ptr(dY), ptr(off), ptr(ent), ptr(w), B, N, G, C, ptr(dP), stream()), "act_interp_rows_bwd_f32")
    return dP


def interp_xyz_grad(dY, xyz, want_w=True, want_b=True):
    """-> (dY^T xyz [C,3] | None, column sums of dY [C] | None)"""
    dY = _sa_f32(dY, "interp_xyz_grad: dY", (None, None))
    R, C = dY.shape
    xyz = _xyz_rows(xyz, "interp_xyz_grad: xyz", R)
    dw = torch.empty(C, 3, dtype=torch.float32, device=dY.device) if want_w else None
    db = torch.empty(C, dtype=torch.float32, device=dY.device) if want_b else None
    ws = workspace(dY.device, lib.act_interp_xyz_grad_workspace(R, C))
    check(lib.act_interp_xyz_grad_f32(ptr(dY), ptr(xyz), R, C, ptr(dw), ptr(db), ptr(ws), ws.numel() * 4, stream()), "act_interp_xyz_grad_f32")
    return dw, db


def _nn3_adjacency(idx, off, ent, G):
    """the adjacency of ``nn3``, built here when the search was asked for none"""
    return (off, ent) if off is not None else three_adjacency(idx, G)


class InterpRowsFn(torch.autograd.Function):
    """three-NN interpolation of per-known-point rows to the unknown points at any G and C, with caller-supplied or kernel weights: x [B*G,C] ->
    [B*N,C] (pointnet2_utils.py:300).  Slots of weight exactly 0 are skipped in both directions.  The backward gathers over the inverse adjacency
    (built here when ``nn3`` carries none): deterministic, bit-identical run to run.  Indices and weights are constants: the reference's distances
    come from the input cloud, a leaf."""

    @staticmethod
    def forward(ctx, x, nn3, B, N, G):
        idx, w, off, ent = nn3
        y = interp_rows_fwd(x, idx, w, B, N, G)
        ctx.save_for_backward(idx, w, off, ent)
        ctx.dims = (B, N, G)
        return y

    @staticmethod
    def backward(ctx, dy):
        idx, w, off, ent = ctx.saved_tensors
        off, ent = _nn3_adjacency(idx, off, ent, ctx.dims[2])
        return interp_rows_bwd(dy, off, ent, w, *ctx.dims), None, None, None, None


def interp_rows(x, nn3, B, N, G):
    """x [B*G,C] rows of the known points, nn3 = (idx, weight, adj_off | None, adj_ent | None) -> [B*N,C]; differentiable in ``x``"""
    return InterpRowsFn.apply(x, nn3, B, N, G)


class InterpConvFn(torch.autograd.Function):
    """the first conv of PointNetFeaturePropagation on cat(xyz, interp(x)) in the per-group form: W [C, 3+K] (xyz columns first), x [B*G,K],
    xyz [B*N,3].  P = x . W[:,3:]^T once per centre (B*G rows instead of B*N), then Y = sum_k w_k P[idx_k] + xyz . W[:,:3]^T + b in one kernel.
    Equal in real arithmetic to the plain form W . cat(xyz, sum_k w_k x[idx_k]) + b (the weights enter linearly)."""

    @staticmethod
    def forward(ctx, x, W, b, xyz, nn3, B, N, G):
        idx, w, off, ent = nn3
        x = _f32c(x)
        xyz = _xyz_rows(xyz, "interp_conv: xyz", B * N)
        wf = W[:, 3:].contiguous()
        wxyz = W[:, :3].contiguous()
        P = gemm(x, wf, True, True)
        y = interp_rows_fwd(P, idx, w, B, N, G, xyz=xyz, wxyz=wxyz, bias=b)
        ctx.save_for_backward(x, wf, xyz, idx, w, off, ent)
        ctx.dims = (B, N, G)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wf, xyz, idx, w, off, ent = ctx.saved_tensors
        dy = _f32c(dy)
        off, ent = _nn3_adjacency(idx, off, ent, ctx.dims[2])
        dP = interp_rows_bwd(dy, off, ent, w, *ctx.dims)
        dx = gemm(dP, wf, True, False) if ctx.needs_input_grad[0] else None
        dW = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dwxyz, db = interp_xyz_grad(dy, xyz, want_w=ctx.needs_input_grad[1], want_b=ctx.has_bias and ctx.needs_input_grad[2])
            if ctx.needs_input_grad[1]:
                dW = torch.cat((dwxyz, gemm(dP, x, False, False)), dim=1)
        return dx, dW, db, None, None, None, None, None


def interp_conv(x, W, b, xyz, nn3, B, N, G):
    return InterpConvFn.apply(x, W, b, xyz, nn3, B, N, G)


# ---- DGCNN classifier (csrc/edgeconv.hip): feature-space kNN, EdgeConv tail with BatchNorm, LeakyReLU row BatchNorm ------------------------------
KNN_FEAT_MAX_K = 64
KNN_FEAT_MAX_C = 512


def knn_features(x, k, want_d2=False):
    """x [B,N,C] -> idx int32 [B,N,k] (and d2 [B,N,k] with ``want_d2``): per point the k nearest points of its own cloud in feature space, itself
    included, in ascending (d2, index) order; d2 is the fp32 difference form summed over ascending channels.  1 <= C <= 512, 1 <= k <= min(N, 64).
    No gradient."""
    x = _sa_f32(x.detach() if isinstance(x, torch.Tensor) else x, "knn_features: x", (None, None, None))
    B, N, C = x.shape
    k = int(k)
    if B < 1 or N < 1 or not 1 <= C <= KNN_FEAT_MAX_C:
        raise ValueError(f"knn_features: x: expected a non-empty [B, N, C] with C <= {KNN_FEAT_MAX_C}, got {list(x.shape)}")
    if not 1 <= k <= min(N, KNN_FEAT_MAX_K):
        raise ValueError(f"knn_features: k must be in [1, min(N, {KNN_FEAT_MAX_K})] = [1, {min(N, KNN_FEAT_MAX_K)}], got {k}")
    if B > 65535:
        raise ValueError(f"knn_features: B must be <= 65535, got {B}")
    idx = torch.empty(B, N, k, dtype=torch.int32, device=x.device)
    d2 = torch.empty(B, N, k, dtype=torch.float32, device=x.device) if want_d2 else None
    rc = lib.act_knn_feat_f32(ptr(x), B, N, C, k, ptr(idx), ptr(d2), stream())
    if rc in (-1, -2):
        raise ValueError(f"act_knn_feat_f32 refused B={B}, N={N}, C={C}, k={k} (code {rc})")
    check(rc, "act_knn_feat_f32")
    return (idx, d2) if want_d2 else idx


class EdgeBnLreluMaxFn(torch.autograd.Function):
    """out[b*N+i, c] = max_j LeakyReLU(BatchNorm(P[b, idx[b,i,j], c] + Q[b,i,c])) with pq = [P | ... | Q] (Q at column qoff) and the BatchNorm over
    all B*N*k edges; no edge tensor is formed, forward or backward (csrc/edgeconv.hip).  Differentiable in pq, gamma and beta."""

    @staticmethod
    def forward(ctx, pq, gamma, beta, running_mean, running_var, idx, qoff, B, N, k, C, training, momentum, eps, slope):
        pq = _f32c(pq, "edge_conv_bn: pq")
        dev = pq.device
        R = B * N
        out = torch.empty(R, C, dtype=torch.float32, device=dev)
        arg = torch.empty(R, C, dtype=torch.int32, device=dev)
        vsum = torch.empty(R, C, dtype=torch.float32, device=dev)
        mean, mean_lo, rstd = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(3))
        ws = workspace(dev, lib.act_edge_bn_workspace(B, N, k, C))
        check(lib.act_edge_bn_lrelu_max_fwd_f32(ptr(pq), pq.stride(0), int(qoff), ptr(idx), B, N, k, C, ptr(gamma), ptr(beta), ptr(running_mean),
                                                ptr(running_var), int(training), float(momentum), float(eps), float(slope), ptr(out), C, 0,
                                                ptr(arg), ptr(vsum), ptr(mean), ptr(mean_lo), ptr(rstd), ptr(ws), ws.numel() * 4, stream()),
              "act_edge_bn_lrelu_max_fwd_f32")
        ctx.save_for_backward(pq, gamma, beta, idx, arg, vsum, mean, mean_lo, rstd)
        ctx.cfg = (int(qoff), B, N, k, C, bool(training), float(slope))
        ctx.mark_non_differentiable(arg, vsum)
        return out, arg, vsum

    @staticmethod
    def backward(ctx, dout, _darg, _dvsum):
        pq, gamma, beta, idx, arg, vsum, mean, mean_lo, rstd = ctx.saved_tensors
        qoff, B, N, k, C, training, slope = ctx.cfg
        if not training:
            raise NotImplementedError("EdgeConv BatchNorm backward in eval mode is off the training path")
        if qoff < C:
            raise ValueError(f"edge_conv_bn: backward needs P and Q in separate columns (qoff >= C), got qoff={qoff}, C={C}")
        dout = _f32c(dout, "edge_conv_bn: grad")
        dev = pq.device
        dpq = torch.empty_like(pq) if (pq.shape[1] == 2 * C and qoff == C) else torch.zeros_like(pq)
        dg, db = torch.empty(C, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev)
        ws = workspace(dev, lib.act_edge_bn_workspace(B, N, k, C))
        check(lib.act_edge_bn_lrelu_max_bwd_f32(ptr(pq), pq.stride(0), qoff, ptr(idx), B, N, k, C, ptr(gamma), ptr(beta), ptr(mean), ptr(mean_lo), ptr(rstd),
                                                slope, ptr(arg), ptr(vsum), ptr(dout), dout.stride(0), ptr(dpq), ptr(dg), ptr(db), ptr(ws),
                                                ws.numel() * 4, stream()), "act_edge_bn_lrelu_max_bwd_f32")
        return (dpq, dg, db) + (None,) * 12


def edge_conv_bn(pq, qoff, idx, B, N, k, C, bn, training, slope=0.2, validate=True, want_aux=False):
    """pq [B*N, ld] (P at column 0, Q at column ``qoff``), idx int [B,N,k] -> [B*N, C]: the fused tail of an EdgeConv layer with the parameters and
    buffers of the BatchNorm module ``bn`` (see EdgeBnLreluMaxFn).  ``validate``: range-check idx on the device (one host read) and raise ValueError
    for an index outside [0,N); pass False for indices ``knn_features`` made.  ``want_aux``: also return (arg, vsum)."""
    B, N, k, C, qoff = int(B), int(N), int(k), int(C), int(qoff)
    if not isinstance(pq, torch.Tensor) or not pq.is_cuda:
        raise _C.ActHipError("edge_conv_bn: pq: expected a CUDA tensor (the HIP kernels have no CPU fallback)")
    if pq.dtype != torch.float32 or pq.dim() != 2:
        raise _C.ActHipError(f"edge_conv_bn: pq: expected float32 [B*N, ld], got {pq.dtype} {list(pq.shape)}")
    if B < 1 or N < 1 or k < 1 or C < 1 or C % 4:
        raise ValueError(f"edge_conv_bn: need B, N, k >= 1 and C % 4 == 0, got B={B}, N={N}, k={k}, C={C}")
    if B > 65535 or k > 65535:
        raise ValueError(f"edge_conv_bn: B and k must be <= 65535, got B={B}, k={k}")
    if pq.shape[0] != B * N or qoff < 0 or qoff + C > pq.shape[1]:
        raise ValueError(f"edge_conv_bn: pq {list(pq.shape)} does not hold [B*N={B * N}] rows with Q at columns [{qoff}, {qoff + C})")
    if bn.num_features != C or bn.weight is None:
        raise ValueError(f"edge_conv_bn: bn must be an affine BatchNorm over {C} channels")
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda:
        raise _C.ActHipError("edge_conv_bn: idx: expected a CUDA tensor (the HIP kernels have no CPU fallback)")
    if idx.dtype not in (torch.int32, torch.int64) or tuple(idx.shape) != (B, N, k):
        raise ValueError(f"edge_conv_bn: idx: expected int32 [{B}, {N}, {k}], got {idx.dtype} {list(idx.shape)}")
    if validate and bool(((idx < 0) | (idx >= N)).any()):
        raise ValueError(f"edge_conv_bn: idx holds an index outside [0, {N})")
    idx = _i32c(idx)
    if training and _sync_group(bn) is not None:
        raise NotImplementedError("edge_conv_bn: SyncBatchNorm across ranks is not implemented for the EdgeConv tail")
    if not training and bn.running_mean is None:
        raise ValueError("edge_conv_bn: eval mode needs running statistics")
    if training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    momentum = 0.1 if bn.momentum is None else bn.momentum
    out, arg, vsum = EdgeBnLreluMaxFn.apply(pq, bn.weight, bn.bias, bn.running_mean, bn.running_var, idx, qoff, B, N, k, C, bool(training), momentum,
                                            bn.eps, slope)
    return (out, arg, vsum) if want_aux else out


# ---- DGCNN segmentation networks (csrc/edge_mlp2.hip): two-layer EdgeConv tail, 3x3 transform of a cloud ---------------------------------------------
EDGE_MLP2_MAX_K = 64
EDGE_MLP2_MAX_C = 128


class EdgeMlp2Fn(torch.autograd.Function):
    """out[b*N+i, :] = max_j LeakyReLU(BN2(w2 . LeakyReLU(BN1(P[b, idx[b,i,j], :] + Q[b,i,:])))), both BatchNorms over all B*N*k edges; the per-edge
    product runs on the matrix cores from tiles built in LDS and no edge tensor is stored by the forward (csrc/edge_mlp2.hip).  Differentiable in
    pq, gamma1, beta1, w2, gamma2 and beta2."""

    @staticmethod
    def forward(ctx, pq, gamma1, beta1, w2, gamma2, beta2, rm1, rv1, rm2, rv2, idx, qoff, B, N, k, C1, C2, training, mom1, eps1, mom2, eps2, slope):
        pq, w2 = _f32c(pq, "edge_mlp2_bn: pq"), _f32c(w2, "edge_mlp2_bn: w2")
        dev = pq.device
        R = B * N
        out = torch.empty(R, C2, dtype=torch.float32, device=dev)
        arg = torch.empty(R, C2, dtype=torch.int32, device=dev)
        ysel = torch.empty(R, C2, dtype=torch.float32, device=dev)
        st1, st2 = torch.empty(3, C1, dtype=torch.float32, device=dev), torch.empty(3, C2, dtype=torch.float32, device=dev)
        ws = workspace(dev, lib.act_edge_mlp2_workspace(B, N, k, C1, C2))
        check(lib.act_edge_mlp2_fwd_f32(ptr(pq), pq.stride(0), int(qoff), ptr(idx), B, N, k, C1, C2, ptr(gamma1), ptr(beta1), ptr(rm1), ptr(rv1), ptr(w2),
                                        ptr(gamma2), ptr(beta2), ptr(rm2), ptr(rv2), int(training), float(mom1), float(eps1), float(mom2), float(eps2),
                                        float(slope), ptr(out), ptr(arg), ptr(ysel), ptr(st1), ptr(st2), ptr(ws), ws.numel() * 4, stream()),
              "act_edge_mlp2_fwd_f32")
        ctx.save_for_backward(pq, gamma1, beta1, w2, gamma2, beta2, idx, arg, ysel, st1, st2)
        ctx.cfg = (int(qoff), B, N, k, C1, C2, bool(training), float(slope))
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, dout, _darg):
        pq, gamma1, beta1, w2, gamma2, beta2, idx, arg, ysel, st1, st2 = ctx.saved_tensors
        qoff, B, N, k, C1, C2, training, slope = ctx.cfg
        if not training:
            raise NotImplementedError("EdgeConv BatchNorm backward in eval mode is off the training path")
        if qoff < C1:
            raise ValueError(f"edge_mlp2_bn: backward needs P and Q in separate columns (qoff >= C1), got qoff={qoff}, C1={C1}")
        dout = _f32c(dout, "edge_mlp2_bn: grad")
        dev = pq.device
        dpq = torch.empty_like(pq) if (pq.shape[1] == 2 * C1 and qoff == C1) else torch.zeros_like(pq)
        dg1, db1 = (torch.empty(C1, dtype=torch.float32, device=dev) for _ in range(2))
        dg2, db2 = (torch.empty(C2, dtype=torch.float32, device=dev) for _ in range(2))
        dw2 = torch.empty(C2, C1, dtype=torch.float32, device=dev)
        ws = workspace(dev, lib.act_edge_mlp2_workspace(B, N, k, C1, C2))
        check(lib.act_edge_mlp2_bwd_f32(ptr(pq), pq.stride(0), qoff, ptr(idx), B, N, k, C1, C2, ptr(gamma1), ptr(beta1), ptr(w2), ptr(gamma2), ptr(beta2),
                                        ptr(st1), ptr(st2), slope, ptr(arg), ptr(ysel), ptr(dout), dout.stride(0), ptr(dpq), ptr(dg1), ptr(db1), ptr(dw2),
                                        ptr(dg2), ptr(db2), ptr(ws), ws.numel() * 4, stream()), "act_edge_mlp2_bwd_f32")
        return (dpq, dg1, db1, dw2, dg2, db2) + (None,) * 17


def edge_mlp2_bn(pq, qoff, idx, B, N, k, C1, bn1, w2, bn2, training, slope=0.2, validate=True, want_aux=False):
    """pq [B*N, ld] (P [.., C1] at column 0, Q at column ``qoff``), idx int [B,N,k], w2 [C2, C1] (or a 1x1 convolution's [C2, C1, 1, 1]) -> [B*N, C2]:
    the tail of a two-layer EdgeConv with the parameters and buffers of the BatchNorm modules ``bn1`` and ``bn2`` (see EdgeMlp2Fn).  1 <= k <= 64,
    4 <= C1, C2 <= 128 and multiples of 4, slope >= 0.  ``validate``: range-check idx on the device (one host read) and raise ValueError for an
    index outside [0,N).  ``want_aux``: also return arg int32 [B*N, C2], the first j that attains the maximum."""
    B, N, k, C1, qoff = int(B), int(N), int(k), int(C1), int(qoff)
    if not isinstance(pq, torch.Tensor) or not pq.is_cuda:
        raise _C.ActHipError("edge_mlp2_bn: pq: expected a CUDA tensor (the HIP kernels have no CPU fallback)")
    if pq.dtype != torch.float32 or pq.dim() != 2:
        raise _C.ActHipError(f"edge_mlp2_bn: pq: expected float32 [B*N, ld], got {pq.dtype} {list(pq.shape)}")
    if not isinstance(w2, torch.Tensor) or not w2.is_cuda or w2.dtype != torch.float32:
        raise _C.ActHipError("edge_mlp2_bn: w2: expected a float32 CUDA tensor")
    if w2.dim() == 4 and w2.shape[2:] == (1, 1):
        w2 = w2.view(w2.shape[0], w2.shape[1])
    if w2.dim() != 2 or w2.shape[1] != C1:
        raise ValueError(f"edge_mlp2_bn: w2: expected [C2, C1={C1}], got {list(w2.shape)}")
    C2 = int(w2.shape[0])
    if B < 1 or N < 1 or not 1 <= k <= EDGE_MLP2_MAX_K:
        raise ValueError(f"edge_mlp2_bn: need B, N >= 1 and 1 <= k <= {EDGE_MLP2_MAX_K}, got B={B}, N={N}, k={k}")
    if not (4 <= C1 <= EDGE_MLP2_MAX_C and 4 <= C2 <= EDGE_MLP2_MAX_C) or C1 % 4 or C2 % 4:
        raise ValueError(f"edge_mlp2_bn: C1 and C2 must be multiples of 4 in [4, {EDGE_MLP2_MAX_C}], got C1={C1}, C2={C2}")
    if B > 65535:
        raise ValueError(f"edge_mlp2_bn: B must be <= 65535, got {B}")
    if not slope >= 0:
        raise ValueError(f"edge_mlp2_bn: slope must be >= 0 (the backward reads the sign of z1 off h), got {slope}")
    if pq.shape[0] != B * N or qoff < 0 or qoff + C1 > pq.shape[1]:
        raise ValueError(f"edge_mlp2_bn: pq {list(pq.shape)} does not hold [B*N={B * N}] rows with Q at columns [{qoff}, {qoff + C1})")
    if bn1.num_features != C1 or bn1.weight is None or bn2.num_features != C2 or bn2.weight is None:
        raise ValueError(f"edge_mlp2_bn: bn1 / bn2 must be affine BatchNorms over {C1} / {C2} channels")
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda:
        raise _C.ActHipError("edge_mlp2_bn: idx: expected a CUDA tensor (the HIP kernels have no CPU fallback)")
    if idx.dtype not in (torch.int32, torch.int64) or tuple(idx.shape) != (B, N, k):
        raise ValueError(f"edge_mlp2_bn: idx: expected int32 [{B}, {N}, {k}], got {idx.dtype} {list(idx.shape)}")
    if validate and bool(((idx < 0) | (idx >= N)).any()):
        raise ValueError(f"edge_mlp2_bn: idx holds an index outside [0, {N})")
    idx = _i32c(idx)
    if training and (_sync_group(bn1) is not None or _sync_group(bn2) is not None):
        raise NotImplementedError("edge_mlp2_bn: SyncBatchNorm across ranks is not implemented for the EdgeConv tail")
    if not training and (bn1.running_mean is None or bn2.running_mean is None):
        raise ValueError("edge_mlp2_bn: eval mode needs running statistics")
    if training:
        for bn in (bn1, bn2):
            if bn.num_batches_tracked is not None:
                bn.num_batches_tracked.add_(1)
    mom1, mom2 = (0.1 if bn.momentum is None else bn.momentum for bn in (bn1, bn2))
    out, arg = EdgeMlp2Fn.apply(pq, bn1.weight, bn1.bias, w2, bn2.weight, bn2.bias, bn1.running_mean, bn1.running_var, bn2.running_mean,
                                bn2.running_var, idx, qoff, B, N, k, C1, C2, bool(training), mom1, bn1.eps, mom2, bn2.eps, slope)
    return (out, arg) if want_aux else out


class CloudTransform3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, T):
        x, T = _f32c(x, "cloud_transform3: x"), _f32c(T, "cloud_transform3: T")
        B, N, _ = x.shape
        y = torch.empty_like(x)
        check(lib.act_cloud_transform3_fwd_f32(ptr(x), ptr(T), B, N, ptr(y), stream()), "act_cloud_transform3_fwd_f32")
        ctx.save_for_backward(x, T)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, T = ctx.saved_tensors
        dy = _f32c(dy, "cloud_transform3: grad")
        B, N, _ = x.shape
        dx, dT = torch.empty_like(x), torch.empty_like(T)
        check(lib.act_cloud_transform3_bwd_f32(ptr(x), ptr(T), ptr(dy), B, N, ptr(dx), ptr(dT), stream()), "act_cloud_transform3_bwd_f32")
        return dx, dT


def cloud_transform3(x, T):
    """x [B,N,3], T [B,3,3] -> y [B,N,3], y[b,n,:] = x[b,n,:] . T[b]; differentiable in both (dT summed in a fixed order)."""
    for t, name in ((x, "x"), (T, "T")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _C.ActHipError(f"cloud_transform3: {name}: expected a CUDA tensor (the HIP kernels have no CPU fallback)")
        if t.dtype != torch.float32 or t.dim() != 3:
            raise _C.ActHipError(f"cloud_transform3: {name}: expected a float32 tensor of three dimensions, got {t.dtype} {list(t.shape)}")
    if x.shape[2] != 3 or tuple(T.shape[1:]) != (3, 3) or T.shape[0] != x.shape[0] or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"cloud_transform3: expected x [B,N,3] and T [B,3,3], got {list(x.shape)} and {list(T.shape)}")
    return CloudTransform3Fn.apply(x, T)


class BNLreluFn(torch.autograd.Function):
    """BNActFn with LeakyReLU(slope) in place of ReLU: the statistics kernel is shared, the apply and the backward carry the slope."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, slope):
        x = _f32c(x)
        R, C = x.shape
        dev = x.device
        y = torch.empty_like(x)
        if training:
            mean, rstd, scale, shift = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(4))
            ws = workspace(dev, lib.act_colstats_workspace(R, C))
            check(lib.act_bn_stats_f32(ptr(x), R, C, ptr(gamma), ptr(beta), float(eps), float(momentum), ptr(running_mean),
                                       ptr(running_var), ptr(mean), ptr(rstd), ptr(scale), ptr(shift), ptr(ws), ws.numel() * 4,
                                       stream()), "act_bn_stats_f32")
        else:
            rstd = torch.rsqrt(running_var + eps)
            mean = running_mean
            scale = gamma * rstd
            shift = beta - running_mean * scale
        check(lib.act_affine_lrelu_f32(ptr(x), ptr(scale), ptr(shift), float(slope), R, C, ptr(y), stream()), "act_affine_lrelu_f32")
        ctx.save_for_backward(x, scale, shift, mean, rstd)
        ctx.training, ctx.slope = training, float(slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, scale, shift, mean, rstd = ctx.saved_tensors
        dy = _f32c(dy)
        R, C = x.shape
        if not ctx.training:
            raise NotImplementedError("BatchNorm backward in eval mode is off the training path")
        dx = torch.empty_like(x)
        dg = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = workspace(x.device, lib.act_bn_lrelu_bwd_workspace(R, C))
        check(lib.act_bn_lrelu_bwd_f32(ptr(x), ptr(dy), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), ctx.slope, R, C, ptr(dx), ptr(dg), ptr(db),
                                       ptr(ws), ws.numel() * 4, stream()), "act_bn_lrelu_bwd_f32")
        return dx, dg, db, None, None, None, None, None, None


# ---- PointMLP (csrc/pointmlp.hip): geometric affine grouping, residual BatchNorm tail -------------------------------------------------------------------
class GeoAffineGroupFn(torch.autograd.Function):
    """LocalGrouper's normalize="anchor" module in row form: out [B*S*k, D (or 2D with cat)], sigma [B].  Differentiable in feat, alpha and beta; the
    backward gathers per point over the inverse adjacency of idx (no edge tensor, no atomics, bit-identical run to run)."""

    @staticmethod
    def forward(ctx, feat, alpha, beta, fps_idx, idx, eps, cat, validate):
        B, N, D = feat.shape
        _, S, k = idx.shape
        dev = feat.device
        out = torch.empty(B * S * k, 2 * D if cat else D, dtype=torch.float32, device=dev)
        sigma, mean = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
        ws = workspace(dev, lib.act_geo_affine_fwd_workspace(B, N, S, k, D))
        rc = lib.act_geo_affine_group_fwd_f32(ptr(feat), ptr(fps_idx), ptr(idx), ptr(alpha), ptr(beta), float(eps), B, N, S, k, D, int(cat), int(validate),
                                              ptr(out), ptr(sigma), ptr(mean), ptr(ws), ws.numel() * 4, stream())
        if rc == -4:
            raise ValueError(f"geo_affine_group: idx or fps_idx holds an index outside [0, {N})")
        if rc == -1:
            raise ValueError(f"act_geo_affine_group_fwd_f32 refused B={B}, N={N}, S={S}, k={k}, D={D}")
        check(rc, "act_geo_affine_group_fwd_f32")
        ctx.save_for_backward(feat, alpha, fps_idx, idx, sigma, mean)
        ctx.cfg = (float(eps), int(cat))
        ctx.mark_non_differentiable(sigma)
        return out, sigma

    @staticmethod
    def backward(ctx, dout, _dsigma):
        feat, alpha, fps_idx, idx, sigma, mean = ctx.saved_tensors
        eps, cat = ctx.cfg
        B, N, D = feat.shape
        _, S, k = idx.shape
        dev = feat.device
        dout = _f32c(dout, "geo_affine_group: grad")
        dfeat = torch.empty_like(feat)
        da, db = torch.empty(D, dtype=torch.float32, device=dev), torch.empty(D, dtype=torch.float32, device=dev)
        ws = workspace(dev, lib.act_geo_affine_bwd_workspace(B, N, S, k, D))
        check(lib.act_geo_affine_group_bwd_f32(ptr(feat), ptr(fps_idx), ptr(idx), ptr(alpha), ptr(sigma), ptr(mean), eps, ptr(dout), B, N, S, k, D, cat,
                                               ptr(dfeat), ptr(da), ptr(db), ptr(ws), ws.numel() * 4, stream()), "act_geo_affine_group_bwd_f32")
        return dfeat, da, db, None, None, None, None, None


def geo_affine_group(feat, fps_idx, idx, alpha, beta, eps=1e-5, cat=False, want_aux=False, validate=True):
    """feat [B,N,D], fps_idx int [B,S] (the anchors' rows, distinct per cloud), idx int [B,S,k], alpha / beta with D elements -> rows [B*S*k, D]:
    alpha * (feat[idx] - feat[fps_idx]) / (std over the cloud's S*k*D differences + eps) + beta, upstream's three roundings.  ``cat``: [B*S*k, 2D] with
    the anchor's row in the columns [D, 2D) (upstream's layout).  ``want_aux``: also sigma [B].  ``validate``: range-check the indices on the device
    (one host read) and raise ValueError; pass False for indices the library's own FPS / kNN made."""
    feat = _sa_f32(feat, "geo_affine_group: feat", (None, None, None))
    B, N, D = feat.shape
    for t, name in ((fps_idx, "fps_idx"), (idx, "idx")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _C.ActHipError(f"geo_affine_group: {name}: expected a CUDA tensor (the HIP kernels have no CPU fallback)")
        if t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"geo_affine_group: {name}: expected int32 or int64 indices, got {t.dtype}")
    if idx.dim() != 3 or idx.shape[0] != B or fps_idx.dim() != 2 or tuple(fps_idx.shape) != (B, idx.shape[1]):
        raise ValueError(f"geo_affine_group: expected idx [{B}, S, k] and fps_idx [{B}, S], got {list(idx.shape)} and {list(fps_idx.shape)}")
    S, k = idx.shape[1], idx.shape[2]
    if B < 1 or B > 65535 or N < 1 or D < 1 or S < 1 or not 1 <= k <= N or S * k * D < 2:
        raise ValueError(f"geo_affine_group: need 1 <= B <= 65535, D >= 1, 1 <= k <= N and S*k*D >= 2, got B={B}, N={N}, S={S}, k={k}, D={D}")
    if validate and (bool(((idx < 0) | (idx >= N)).any()) or bool(((fps_idx < 0) | (fps_idx >= N)).any())):     # (int64 values are checked before the cast)
        raise ValueError(f"geo_affine_group: idx or fps_idx holds an index outside [0, {N})")
    alpha, beta = (_sa_f32(t.reshape(-1), f"geo_affine_group: {n}", (D,)) for t, n in ((alpha, "alpha"), (beta, "beta")))
    out, sigma = GeoAffineGroupFn.apply(feat, alpha, beta, _i32c(fps_idx), _i32c(idx), float(eps), bool(cat), bool(validate))
    return (out, sigma) if want_aux else out


class BNAddReluFn(torch.autograd.Function):
    """ReLU(BatchNorm(y) + res) on rows [R,C]: the statistics kernel of BNActFn, an apply with the residual, and a backward that takes the ReLU mask from
    the saved output (scale * y + shift alone does not give it) and writes dy and dres in one pass."""

    @staticmethod
    def forward(ctx, y, res, gamma, beta, running_mean, running_var, training, momentum, eps):
        y, res = _f32c(y), _f32c(res)
        R, C = y.shape
        dev = y.device
        out = torch.empty_like(y)
        if training:
            mean, rstd, scale, shift = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(4))
            ws = workspace(dev, lib.act_colstats_workspace(R, C))
            check(lib.act_bn_stats_f32(ptr(y), R, C, ptr(gamma), ptr(beta), float(eps), float(momentum), ptr(running_mean),
                                       ptr(running_var), ptr(mean), ptr(rstd), ptr(scale), ptr(shift), ptr(ws), ws.numel() * 4,
                                       stream()), "act_bn_stats_f32")
        else:
            rstd = torch.rsqrt(running_var + eps)
            mean = running_mean
            scale = (gamma * rstd).contiguous()
            shift = (beta - running_mean * scale).contiguous()
        check(lib.act_affine_add_relu_f32(ptr(y), ptr(res), ptr(scale), ptr(shift), R, C, ptr(out), stream()), "act_affine_add_relu_f32")
        ctx.save_for_backward(y, out, gamma, mean)
        ctx.training, ctx.eps = training, float(eps)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, out, gamma, mean = ctx.saved_tensors
        if not ctx.training:
            raise NotImplementedError("BatchNorm backward in eval mode is off the training path")
        dout = _f32c(dout)
        R, C = y.shape
        dy, dres = torch.empty_like(y), torch.empty_like(y)
        dg = torch.empty(C, dtype=torch.float32, device=y.device)
        db = torch.empty(C, dtype=torch.float32, device=y.device)
        ws = workspace(y.device, lib.act_bn_add_relu_bwd_workspace(R, C))
        check(lib.act_bn_add_relu_bwd_f32(ptr(y), ptr(out), ptr(dout), ptr(gamma), ptr(mean), ctx.eps, R, C, ptr(dy), ptr(dres), ptr(dg), ptr(db),
                                          ptr(ws), ws.numel() * 4, stream()), "act_bn_add_relu_bwd_f32")
        return dy, dres, dg, db, None, None, None, None, None


def batch_norm_add_relu(y, res, bn, training):
    """functional ReLU(nn.BatchNorm1d(y) + res) on rows [R,C] with the module's parameters and buffers: the tail of PointMLP's residual block.  Statistics,
    running statistics and num_batches_tracked move exactly as in ``batch_norm_act``."""
    if y.dim() != 2 or y.shape != res.shape or y.shape[0] < 1 or y.shape[1] != bn.num_features:
        raise ValueError(f"batch_norm_add_relu: expected y and res [R, {bn.num_features}], got {list(y.shape)} and {list(res.shape)}")
    if training and _sync_group(bn) is not None:
        raise NotImplementedError("batch_norm_add_relu: a SyncBatchNorm across ranks is not implemented")
    if training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return BNAddReluFn.apply(y, res, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, bn.momentum, bn.eps)


# ---- PCT (csrc/offset_attn.hip): offset attention ---------------------------------------------------------------------------------------------------------
class OffsetAttentionFn(torch.autograd.Function):
    """PCT's offset attention on rows: softmax over the keys without a scale, L1 over the queries, x_r = P^t v / (1e-9 + colsum), optionally x - x_r.
    Saved for the backward: colsum [B*N] and x_r (the output itself when x is not fused); the backward forms the row statistics again instead of
    trusting lse rounded to float32.  No [N,N] tensor in either direction."""

    @staticmethod
    def forward(ctx, q, k, v, x, B, N):
        Dq, C = q.shape[1], v.shape[1]
        dev = q.device
        out = torch.empty_like(v)
        lse, colsum = torch.empty(B * N, dtype=torch.float32, device=dev), torch.empty(B * N, dtype=torch.float32, device=dev)
        xr = torch.empty_like(v) if x is not None and any(ctx.needs_input_grad[:3]) else None
        ws = workspace(dev, lib.act_offset_attn_workspace(B, N, Dq, C))
        rc = lib.act_offset_attn_fwd_f32(ptr(q), ptr(k), ptr(v), ptr(x), B, N, Dq, C, ptr(out), ptr(lse), ptr(colsum), ptr(xr), ptr(ws), ws.numel() * 4,
                                         stream())
        if rc == -1:
            raise ValueError(f"act_offset_attn_fwd_f32 refused B={B}, N={N}, Dq={Dq}, C={C}")
        check(rc, "act_offset_attn_fwd_f32")
        ctx.save_for_backward(q, k, v, colsum, out if x is None else xr)
        ctx.cfg = (B, N, x is not None)
        ctx.mark_non_differentiable(lse, colsum)
        return out, lse, colsum

    @staticmethod
    def backward(ctx, dout, _dlse, _dcolsum):
        q, k, v, colsum, xr = ctx.saved_tensors
        B, N, fused = ctx.cfg
        dout = _f32c(dout, "offset_attention: grad")
        dx = dout if fused and ctx.needs_input_grad[3] else None
        if not any(ctx.needs_input_grad[:3]):
            return None, None, None, dx, None, None
        Dq, C = q.shape[1], v.shape[1]
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ws = workspace(q.device, lib.act_offset_attn_workspace(B, N, Dq, C))
        check(lib.act_offset_attn_bwd_f32(ptr(q), ptr(k), ptr(v), ptr(colsum), ptr(xr), ptr(dout), int(fused), B, N, Dq, C, ptr(dq), ptr(dk), ptr(dv),
                                          ptr(ws), ws.numel() * 4, stream()), "act_offset_attn_bwd_f32")
        return dq, dk, dv, dx, None, None


def offset_attention(q, k, v, B, N, x=None, want_aux=False):
    """q, k [B*N, Dq], v [B*N, C] and optionally x [B*N, C] -> x_r [B*N, C] (or x - x_r): per cloud P = softmax_j(q_i . k_j) without a scale,
    x_r[j] = sum_i P[i,j] v_i / (1e-9 + sum_i P[i,j]).  Differentiable in q, k, v and x; q and k may be one tensor (autograd adds dq and dk).
    ``want_aux``: also lse [B*N] and the column sums [B*N].  1 <= N <= 1024, Dq % 4 == 0 in [4, 64], C % 4 == 0 in [4, 256], else ValueError."""
    B, N = int(B), int(N)
    for t, name in ((q, "q"), (k, "k"), (v, "v")) + (((x, "x"),) if x is not None else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _C.ActHipError(f"offset_attention: {name}: expected a CUDA tensor (the HIP kernels have no CPU fallback)")
        if t.dtype != torch.float32 or t.dim() != 2:
            raise _C.ActHipError(f"offset_attention: {name}: expected a float32 tensor of two dimensions, got {t.dtype} {list(t.shape)}")
    Dq, C = q.shape[1], v.shape[1]
    if not (1 <= B <= 65535 and 1 <= N <= 1024 and 4 <= Dq <= 64 and Dq % 4 == 0 and 4 <= C <= 256 and C % 4 == 0):
        raise ValueError(f"offset_attention: need 1 <= N <= 1024, Dq % 4 == 0 in [4, 64] and C % 4 == 0 in [4, 256], got B={B}, N={N}, Dq={Dq}, C={C}")
    if tuple(q.shape) != (B * N, Dq) or tuple(k.shape) != (B * N, Dq) or tuple(v.shape) != (B * N, C) or (x is not None and x.shape != v.shape):
        raise ValueError(f"offset_attention: expected q, k [{B * N}, Dq] and v, x [{B * N}, C], got {list(q.shape)}, {list(k.shape)}, {list(v.shape)}"
                         + (f", {list(x.shape)}" if x is not None else ""))
    same = k is q
    q = q.contiguous()
    out, lse, colsum = OffsetAttentionFn.apply(q, q if same else k.contiguous(), v.contiguous(), None if x is None else x.contiguous(), B, N)
    return (out, lse, colsum) if want_aux else out
