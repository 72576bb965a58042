"""Plain numpy references (float64 / int64) of the row kernels in csrc/norm.hip -- LayerNorm forward and backward, the column sums, cross-entropy,
mse / smooth-l1, the cosine loss, the row gate, the add and the prompt rows -- the launch arithmetic of its entry points, and the inputs that
tests/test_gpu_norm_rows_edges.py feeds them.  tests/test_norm_rows_host.py checks every function here against torch.nn.functional / autograd in
float64, so the references are verified without a GPU.  No GPU code and no import of act_amd.  Inputs are generated once per process and handed out
read-only."""
import functools

import numpy as np

LN_EPS = 1e-5
COS_EPS = 1e-8                                               # CosineLossFn's eps (F.cosine_similarity's default)
GRID_CAP = 8192 * 256                                        # threads of the largest grid of the grid-stride kernels

# (D, M) of the far-mean lattice rows: |M| D + 4 D <= 2^21 keeps every float32 partial sum of a row exact (units of 1/8 below 2^24)
FAR_MEAN = [(4, 1024.0), (260, 1024.0), (384, 4096.0), (768, -2048.0), (2048, 512.0)]
FAR_T = 9                                                    # rows per case: three workgroups of the forward, the last with one live wave

LN_D = [4, 260, 512, 516, 1024, 1028, 2048]                  # one float4; one live lane in chunk 2; either side of both MAXV switches; the widest row
LN_FWD_T = [1, 5, 33]
LN_BWD_T = [1, 15, 16, 17, 33]
LN_BWD_BIG = (16411, 64)                                     # rows_per_block grows to 20; the last workgroup holds 11 rows

# T of the exact dgamma / dbeta cases -> nblk (16 rows per workgroup): every stride tail of colsum_stage2_pair
#   1: one row-lane; 2: two row-lanes; 5: the 8-stride loop once; 33: the 32-stride loop once plus the 4-stride tail; 820: all three
LN_EXACT_T = {11: 1, 20: 2, 70: 5, 520: 33, 13110: 820}
LN_EXACT_D = 68                                              # two column blocks of colsum_stage2_pair, the second of one float4

# (R, C) of act_colsum_f32 -> (parts, rows_per_block, nparts launched, rows of the last part)
#   (0, 8)       no rows: one part of zeros
#   (1, 1)       one element
#   (3, 5)       one part, a row-lane idle
#   (33, 70)     two parts, a second column block of six columns
#   (100, 64)    four parts: the tail loop only
#   (1000, 130)  32 parts of 32 rows, the last of 8: the unrolled loop once without a tail
#   (32768, 8)   1,024 parts launched
#   (32800, 8)   the 1,024-part cap binds (1,025 without it); rounding rows_per_block to 4 leaves 912 parts of 36 rows: unrolled loop plus tail
COLSUM = {(0, 8): (1, 4, 1, 0), (1, 1): (1, 4, 1, 1), (3, 5): (1, 4, 1, 3), (33, 70): (2, 20, 2, 13), (100, 64): (4, 28, 4, 16),
          (1000, 130): (32, 32, 32, 8), (32768, 8): (1024, 32, 1024, 32), (32800, 8): (1024, 36, 912, 4)}
COLSUM_SHAPES = list(COLSUM)

XENT_SHAPES = [(1, 1), (1, 3), (5, 63), (7, 64), (9, 65), (1025, 10), (2500, 40)]          # the last two: mean_kernel with per = 2 and 3
REG_SHAPES = [(1, 1), (5, 63), (1025, 65), (2100, 1000)]                                   # the last: n > GRID_CAP
COS_SHAPES = [(1, 4), (5, 63), (204, 384), (1025, 65)]
# d = s - t at and beside the knee of smooth-l1 (beta = 1); t = 0 so that d is exactly s
KNEE = [1.0, -1.0, 1.0 - 2.0 ** -23, -(1.0 - 2.0 ** -23), 1.0 + 2.0 ** -22, -(1.0 + 2.0 ** -22), 0.0, 3.0, -3.0]
SCALE_ROWS = [(7, 4, 3), (64, 260, 64), (4100, 2052, 41)]                                  # (T, D, rows_per_scale); the last: T D / 4 > GRID_CAP
ADD_N = [0, 4, 4 * (GRID_CAP + 37)]
PROMPT = (17624, 7, 68)                                      # (B, P, D): B P D / 4 = 2,097,256 > GRID_CAP; P no power of two, 17 float4 per row


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- launch arithmetic -------------------------------------------------------------------------------------------------------------------------
def ln_bwd_blocks(T, rpb_env=0):
    """ln_rows_per_block / nblk of act_layernorm_bwd_f32 -> (rows_per_block, nblk, rows of the last workgroup).  rpb_env: ACT_LN_BWD_RPB"""
    floor = (rpb_env + 3) // 4 * 4 if rpb_env >= 4 else 16
    r = ((T + 1023) // 1024 + 3) // 4 * 4
    rpb = max(r, floor)
    nblk = (T + rpb - 1) // rpb
    return rpb, nblk, T - (nblk - 1) * rpb


def ln_bwd_workspace_floats(T, D, rpb_env=0):
    """act_layernorm_bwd_workspace in floats: one partial row of dgamma and one of dbeta per workgroup"""
    return ln_bwd_blocks(T, rpb_env)[1] * D * 2


def colsum_parts(R, C):
    """act_colsum_f32 -> (parts the workspace is sized for, rows_per_block, nparts launched, rows of the last part)"""
    cb = (C + 63) // 64
    parts = max(1, min((2048 + cb - 1) // cb, (R + 31) // 32, 1024))
    rpb = max(4, ((R + parts - 1) // parts + 3) // 4 * 4)
    nparts = max(1, (R + rpb - 1) // rpb)
    return parts, rpb, nparts, R - (nparts - 1) * rpb


def colsum_workspace_floats(R, C):
    return colsum_parts(R, C)[0] * C


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps=LN_EPS):
    """-> y, mean, rstd (two passes, biased variance)"""
    x = _f64(x)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / np.sqrt(var + eps)
    return (x - mean[:, None]) * rstd[:, None] * _f64(gamma) + _f64(beta), mean, rstd


def layernorm_bwd(dy, xin, gamma, mean, rstd, dres=None):
    """-> dx = dres + rstd (dy g - mean(dy g) - xhat mean(dy g xhat)), dgamma = sum_r dy xhat, dbeta = sum_r dy; mean / rstd are inputs"""
    dy, xin = _f64(dy), _f64(xin)
    xh = (xin - _f64(mean)[:, None]) * _f64(rstd)[:, None]
    w = dy * _f64(gamma)
    dx = _f64(rstd)[:, None] * (w - w.mean(1, keepdims=True) - xh * (w * xh).mean(1, keepdims=True))
    if dres is not None:
        dx = dx + _f64(dres)
    return dx, (dy * xh).sum(0), dy.sum(0)


def layernorm_y32(x, gamma, beta, eps, single_pass):
    """LayerNorm in float32 numpy: two passes (mean, then the centred second moment) or one (E[x^2] - mean^2).  What the far-mean lattice tells
    apart; a negative variance of the one-pass form comes out as NaN"""
    x = np.asarray(x, np.float32)
    D = np.float32(x.shape[1])
    mean = x.sum(1, dtype=np.float32) / D
    if single_pass:
        var = (x * x).sum(1, dtype=np.float32) / D - mean * mean
    else:
        c = x - mean[:, None]
        var = (c * c).sum(1, dtype=np.float32) / D
    with np.errstate(invalid="ignore"):
        rstd = (np.float32(1) / np.sqrt(var + np.float32(eps))).astype(np.float32)
    return (x - mean[:, None]) * rstd[:, None] * np.asarray(gamma, np.float32) + np.asarray(beta, np.float32)


def rel(a, ref):
    """max|a - ref| / max(1, max|ref|): the _rel of tests/test_gpu_dense.py on arrays (NaN -> inf)"""
    a, ref = _f64(a), _f64(ref)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if a.size == 0:
        return 0.0
    e = np.abs(a - ref).max() / max(1.0, np.abs(ref).max())
    return float("inf") if np.isnan(e) else float(e)


@functools.lru_cache(maxsize=None)
def ln_params(D):
    r = np.random.default_rng(7919 * D + 1)
    return _frozen((1 + 0.1 * r.standard_normal(D)).astype(np.float32), (0.1 * r.standard_normal(D)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def ln_real(T, D):
    """Gaussian rows -> x, pos, dy, dres (float32)"""
    r = np.random.default_rng(100003 * T + D)
    return _frozen(*(s * r.standard_normal((T, D)).astype(np.float32) for s in (np.float32(1), np.float32(0.3), np.float32(1), np.float32(1))))


@functools.lru_cache(maxsize=None)
def far_mean_rows(T, D, M):
    """x [T,D] = M + k / 8, k integer in [-32, 32], every row of k summing to zero: the row mean is M exactly, the spread is O(1)"""
    r = np.random.default_rng(int(abs(M)) * 31 + D)
    half = r.integers(-32, 33, (T, D // 2))
    k = np.concatenate([half, -half], axis=1)
    k = np.take_along_axis(k, np.argsort(r.random((T, D)), axis=1), axis=1)
    assert (k.sum(1) == 0).all()
    return _frozen((M + k / 8.0).astype(np.float32))[0]


@functools.lru_cache(maxsize=None)
def ln_bwd_lattice(T, D):
    """-> xin = mean + {-4..4}, dy in {-2..2}, mean [T] in {-4..4}, rstd = 0.5, gamma (float32 holding integers but for rstd).  xhat and dy xhat
    are multiples of 1/2, so dgamma / dbeta are sums of multiples of 1/2 below 2^24: exact in float32 in any order"""
    r = np.random.default_rng(1000003 * T + D)
    mean = r.integers(-4, 5, T)
    xin = mean[:, None] + r.integers(-4, 5, (T, D))
    dy = r.integers(-2, 3, (T, D))
    gamma = r.integers(1, 4, D)
    return _frozen(xin.astype(np.float32), dy.astype(np.float32), mean.astype(np.float32), np.full(T, 0.5, np.float32), gamma.astype(np.float32))


def ln_bwd_lattice_sums(T, D):
    """dgamma, dbeta on ln_bwd_lattice(T, D), from int64 sums: dgamma = (sum dy (xin - mean)) / 2"""
    xin, dy, mean, _, _ = (a.astype(np.int64) for a in ln_bwd_lattice(T, D))
    return (dy * (xin - mean[:, None])).sum(0) / 2.0, dy.sum(0).astype(np.float64)


# ---- column sums -------------------------------------------------------------------------------------------------------------------------------
def colsum(x):
    return _f64(x).sum(0)


@functools.lru_cache(maxsize=None)
def colsum_lattice(R, C):
    """integers in [-8, 8] as float32 [R,C]: column sums below 2^24, exact in any order"""
    return _frozen(np.random.default_rng(31 * R + C).integers(-8, 9, (R, C)).astype(np.float32))[0]


# ---- cross-entropy -----------------------------------------------------------------------------------------------------------------------------
def xent(z, lab, g=1.0):
    """nn.CrossEntropyLoss (mean) -> loss, lse [R], top-1 fraction (lowest index among ties), dz = g / R (softmax - onehot).  -inf logits are
    classes that do not exist (probability 0); -inf on the label gives loss +inf"""
    z = _f64(z)
    lab = np.asarray(lab, np.int64)
    R = z.shape[0]
    m = z.max(1)
    e = np.exp(z - m[:, None])
    lse = m + np.log(e.sum(1))
    rows = np.arange(R)
    loss = (lse - z[rows, lab]).mean()
    p = e / e.sum(1, keepdims=True)
    p[rows, lab] -= 1.0
    return loss, lse, float((z.argmax(1) == lab).sum()) / R, g * p / R


@functools.lru_cache(maxsize=None)
def xent_input(R, C):
    r = np.random.default_rng(7 * R + C)
    return _frozen((3 * r.standard_normal((R, C))).astype(np.float32), r.integers(0, C, R))


# ---- regression losses -------------------------------------------------------------------------------------------------------------------------
def regression(s, t, kind, g=1.0):
    """kind 0: nn.MSELoss (mean); kind 1: nn.SmoothL1Loss (mean, beta = 1) -> loss, ds"""
    d = _f64(s) - _f64(t)
    if kind == 0:
        return (d * d).mean(), g * 2 * d / d.size
    a = np.abs(d)
    return np.where(a < 1, 0.5 * d * d, a - 0.5).mean(), g * np.clip(d, -1, 1) / d.size


# ---- cosine loss -------------------------------------------------------------------------------------------------------------------------------
def cosine(s, t, eps=COS_EPS, g=1.0):
    """mean_r (1 - cos_r), cos = s.t / (max(|s|, eps) max(|t|, eps)): F.cosine_similarity of the installed torch, every norm clamped on its own
    -> loss, row loss [R], ds.  The backward is autograd's: torch clamps the two norms in place under no_grad, so a clamped |s| still passes its
    gradient s / |s| on (0 at s = 0):   ds_r = -g / R (t / (ns nt) - cos s / (ns |s|)),   ns = max(|s|, eps), nt = max(|t|, eps).
    Where |s| > eps that is the derivative of cos, t / (|s| nt) - cos s / |s|^2; a zero student row gets -g / R t / (eps nt)"""
    s, t = _f64(s), _f64(t)
    R = s.shape[0]
    ss, tt, dot = (s * s).sum(1), (t * t).sum(1), (s * t).sum(1)
    n1 = np.sqrt(ss)
    ns, nt = np.maximum(n1, eps), np.maximum(np.sqrt(tt), eps)
    cos = dot / (ns * nt)
    second = np.where(n1 > 0, cos / (ns * np.where(n1 > 0, n1, 1.0)), 0.0)
    ds = -(g / R) * (t / (ns * nt)[:, None] - s * second[:, None])
    return (1 - cos).mean(), 1 - cos, ds


def cosine_product_clamp(s, t, eps=COS_EPS):
    """the definition the kernels had before: s.t / max(|s| |t|, eps) -> row cos.  Kept to show where the two part"""
    s, t = _f64(s), _f64(t)
    return (s * t).sum(1) / np.maximum(np.sqrt((s * s).sum(1) * (t * t).sum(1)), eps)


@functools.lru_cache(maxsize=None)
def cos_input(R, D):
    r = np.random.default_rng(13 * R + D)
    return _frozen(r.standard_normal((R, D)).astype(np.float32), r.standard_normal((R, D)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def cos_clamp_input(D=63):
    """-> s, t [6, D] float32 and the row names.  Every norm is 0 or a factor of 100 or more away from eps = 1e-8, so float32 and float64 take the
    same side of each clamp"""
    s, t = (a.copy() for a in cos_input(6, D))
    names = ["ordinary", "zero student", "zero teacher", "both zero", "student of norm 1e-10", "teacher of norm 1e-10"]
    s[1] = 0; t[2] = 0; s[3] = 0; t[3] = 0
    s[4] = (s[4].astype(np.float64) * (1e-10 / np.linalg.norm(s[4].astype(np.float64)))).astype(np.float32)
    t[5] = (t[5].astype(np.float64) * (1e-10 / np.linalg.norm(t[5].astype(np.float64)))).astype(np.float32)
    return _frozen(s, t) + (names,)


# ---- row gate, add, prompt rows ----------------------------------------------------------------------------------------------------------------
def scale_rows(x, gate, rows_per_scale):
    """x[r,:] * gate[r // rows_per_scale] in float32: one multiplication per element, so the device result is this one bit for bit"""
    x = np.asarray(x, np.float32)
    return x * np.asarray(gate, np.float32)[np.arange(x.shape[0]) // rows_per_scale, None]


def add(a, b):
    return np.asarray(a, np.float32) + np.asarray(b, np.float32)


def prompt_rows_fwd(tok, ppos, mask, B, inv_keep):
    """y[b P + p, :] = tok[p, :] mask[b P + p, :] inv_keep + ppos[p, :]  (float64)"""
    P, D = tok.shape
    return (_f64(tok)[None] * _f64(mask).reshape(B, P, D) * inv_keep + _f64(ppos)[None]).reshape(B * P, D)


def prompt_rows_bwd(dy, mask, B, P, inv_keep):
    """-> dtok[p, :] = sum_b dy mask inv_keep, dppos[p, :] = sum_b dy; int64 where dy holds integers"""
    dy, mask = np.asarray(dy), np.asarray(mask)
    D = dy.shape[1]
    if np.array_equal(dy, np.rint(dy)) and inv_keep == int(inv_keep):
        dy, mask, inv_keep = dy.astype(np.int64), mask.astype(np.int64), int(inv_keep)
    else:
        dy, mask = _f64(dy), _f64(mask)
    dy, mask = dy.reshape(B, P, D), mask.reshape(B, P, D)
    return (dy * mask * inv_keep).sum(0), dy.sum(0)
