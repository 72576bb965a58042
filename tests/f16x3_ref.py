"""numpy restatement of the split-f16 teacher arithmetic (act_amd/csrc/split_planes.h, gemm_bf16x3.hip F16 form, composite.f16x3_*): the plane split, the scale
rules, the three-product GEMM with its two accumulators, and the weight-only range-guard bounds.  Written from the specification, not from the kernels:
tests/test_f16x3_host.py checks it against float64, tests/test_gpu_f16x3.py checks the kernels against it bit for bit."""
import math

import numpy as np

MIN_NORMAL = np.float16(2.0 ** -14)


def f16_plane(v):
    """float32 -> float16, round to nearest even (numpy's astype); a result below 2^-14 in magnitude (zero or an f16 subnormal) is written as +0"""
    h = np.asarray(v, dtype=np.float32).astype(np.float16)
    return np.where(np.abs(h) < MIN_NORMAL, np.float16(0), h)


def split(x, scale=1.0):
    """x * scale ~= h1 + 2^-11 h2.  ``scale``: a power of two, scalar or broadcastable (one per row: scale[:, None])"""
    xs = np.asarray(x, dtype=np.float32) * np.asarray(scale, dtype=np.float32)
    h1 = f16_plane(xs)
    h2 = f16_plane((xs - h1.astype(np.float32)) * np.float32(2048.0))        # flushed h1 -> the residual is the whole value
    return h1, h2


def row_scales(w):
    """one power of two per row lifting the row's largest magnitude into [2^14, 2^15); 1 for an all-zero row"""
    mx = np.abs(np.asarray(w, dtype=np.float32)).max(axis=1)
    e = np.frexp(mx)[1]                                                      # mx = m 2^e, m in [0.5, 1)
    return np.where(mx > 0, np.ldexp(np.float32(1), 15 - e), np.float32(1)).astype(np.float32)


def act_scale(bound):
    """largest power of two s with bound * s <= 2^15; 0 (stay on the f32 kernel) for bound > 2^15 or a non-finite bound"""
    bound = float(bound)
    if not math.isfinite(bound) or bound > 32768.0:
        return 0.0
    if bound < 2.0 ** -15:
        return 2.0 ** 30
    s = 2.0 ** math.floor(math.log2(32768.0 / bound))
    while bound * s > 32768.0:
        s /= 2
    while bound * s * 2 <= 32768.0:
        s *= 2
    return s


def gemm(a, w, a_scale, acc_dtype=np.float32, drop_lolo=True):
    """(a . w^T) the kernel's way: planes of a * a_scale and of w * row scale, acc0 = h1.h1, acc1 = h1.h2 + h2.h1 (acc_dtype accumulation),
    (acc0 + 2^-11 acc1) / s_B[n] / s_A"""
    sb = row_scales(w)
    a1, a2 = (p.astype(acc_dtype) for p in split(a, a_scale))
    b1, b2 = (p.astype(acc_dtype) for p in split(w, sb[:, None]))
    acc0 = a1 @ b1.T
    acc1 = a1 @ b2.T + a2 @ b1.T
    if not drop_lolo:
        acc1 = acc1 + (a2 @ b2.T) / acc_dtype(2048.0)
    v = acc0 + acc1 * acc_dtype(1.0 / 2048.0)
    return (v * (1.0 / sb).astype(acc_dtype)[None, :]) * acc_dtype(1.0 / a_scale)


# ---- range guard: bounds that depend on the frozen weights alone -------------------------------------------------------------------------------------------
def ln_bound(gamma, beta):
    """|LN(x)_j gamma_j + beta_j| <= sqrt(D) |gamma_j| + |beta_j|   (|xhat_j| <= sqrt(D - 1) for any row)"""
    g, b = np.abs(np.asarray(gamma, dtype=np.float64)), np.abs(np.asarray(beta, dtype=np.float64))
    return math.sqrt(g.shape[0]) * g + b


def l1_bound(w, bias, u):
    """|sum_j W[n,j] x_j + b_n| <= sum_j |W[n,j]| u_j + |b_n|  for |x_j| <= u_j"""
    out = np.abs(np.asarray(w, dtype=np.float64)) @ np.asarray(u, dtype=np.float64)
    return out + (np.abs(np.asarray(bias, dtype=np.float64)) if bias is not None else 0.0)


def block_bounds(n1w, n1b, wqkv, bqkv, n2w, n2b, w1, b1):
    """bounds on the A operand of (qkv, proj, fc1, fc2): LN1 output; attention output <= max |V| (convex combination, V rows of the qkv Linear applied to
    LN1 outputs -- tokens and prompts alike); LN2 output; |GELU(x)| <= |x| of the fc1 pre-activation"""
    D = np.asarray(n1w).shape[0]
    u1, u2 = ln_bound(n1w, n1b), ln_bound(n2w, n2b)
    v = l1_bound(np.asarray(wqkv)[2 * D:], None if bqkv is None else np.asarray(bqkv)[2 * D:], u1)
    return [float(u1.max()), float(v.max()), float(u2.max()), float(l1_bound(w1, b1, u2).max())]
