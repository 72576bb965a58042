"""Plain numpy references (float64 / int64) of the row kernels in csrc/pointnet.hip, the shapes at which tests/test_gpu_pointnet_rows_edges.py runs
them and the inputs it feeds them.  tests/test_pointnet_rows_host.py checks every function here against torch float64 autograd and torch.max on
every shape, so the references are verified without a GPU.  Inputs are generated once per process and handed out read-only."""
import functools

import numpy as np

EPS32 = 2.0 ** -24                                           # half an ulp of a float32 in [1, 2)
BN_EPS = 1e-5

# (R, C) for statistics, apply and backward.  The launch arithmetic is stats_parts() of pointnet.hip (restated in launch() below):
#   parts = min(ceil(2048 / ceil(C / 64)), ceil(R / 64), 1024), rows_per_block = ceil(R / parts) rounded up to a multiple of 4.
# (R, C)          parts x rows_per_block, rows of the last part      reaches
# (2, 4)          1 x 4, 2       smallest train-mode BatchNorm; two row-lanes idle; one float4 quad
# (3, 68)         1 x 4, 3       second column block of one quad
# (5, 3)          1 x 8, 5       scalar forms, C < 4 (C ABI only: act_affine_act_f32 rejects C & 3)
# (17, 256)       1 x 20, 17     the classification head's BatchNorm on a ragged last batch
# (63, 64)        1 x 64, 63     just under the first split
# (65, 64)        2 x 36, 29     just over it; the part boundary (row 36) is not a multiple of 16
# (67, 130)       2 x 36, 31     C % 4 = 2: scalar backward; third column block of two columns
# (193, 132)      4 x 52, 37     exactly four parts through the four part-lanes of fold_partials
# (257, 132)      5 x 52, 49     five parts: one part-lane takes two
# (33000, 66)     516 x 64, 40   scalar apply past the grid cap (2,178,000 > 2,097,152 elements)
# (200003, 64)    1021 x 196, 83 the 1,024-part cap; three unrolled iterations plus a tail per row-lane in both stage-1 forms; bn_bwd_apply4 and
#                                affine_act past the grid cap (3.2 M float4)
LAUNCH = {(2, 4): (1, 4, 2), (3, 68): (1, 4, 3), (5, 3): (1, 8, 5), (17, 256): (1, 20, 17), (63, 64): (1, 64, 63), (65, 64): (2, 36, 29),
          (67, 130): (2, 36, 31), (193, 132): (4, 52, 37), (257, 132): (5, 52, 49), (33000, 66): (516, 64, 40), (200003, 64): (1021, 196, 83)}
SHAPES = list(LAUNCH)
VEC_SHAPES = [s for s in SHAPES if s[1] % 4 == 0]
SCALAR_SHAPES = [s for s in SHAPES if s[1] % 4 != 0]
GRID_CAP = 8192 * 256                                        # grid_for(): threads of the largest grid

# (G, n, C) for the live-group backward: R = 65, the part boundary at row 36 falls inside group 2; the scalar forms
LIVE_SHAPES = [(5, 13, 68), (3, 67, 130)]
# (tiles, rows_per_tile, C): one tile; a second workgroup of four columns; 63 / 64 / 65 tiles through 64 tile-lanes; M2 = 0 everywhere; the model's
TILE_SHAPES = [(1, 128, 16), (3, 32, 20), (63, 128, 16), (64, 128, 48), (65, 128, 20), (130, 1, 16), (2048, 128, 64)]
EVAL_C = [1, 255, 256, 257]
# (G, n, C) for the group kernels; the last has 2,132,000 outputs and 4,264,000 inputs, both past the grid cap
GROUP_SHAPES = [(1, 1, 1), (3, 1, 5), (7, 13, 3), (5, 32, 68), (9, 7, 130), (8200, 2, 260)]
SUM_N = [1, 3, 4, 5, 7, 13]                                  # group_sum: tail only, one unrolled step, an unrolled step plus tail
# (R, A): row 0 of x = 1.5 N(0,1) + 0.7 set to A, C = 64
PIVOT_CASES = [(4096, 30.0), (4096, 100.0), (4096, 1000.0), (65536, 30.0), (65536, 100.0)]
PIVOT_C = 64
# the first-row requirement at ragged shapes: an outlier OUTLIER in row 0 of every third column of the lattice.  dm^2 / var cannot exceed R - 1, so
# only R >= 27 can take the far-pivot branch of column_mean_var; these do, with one part of 63 rows (lanes of 16, 16, 16, 15), two to five parts
# through four part-lanes, a shorter last part, a partial column block, and far and near columns side by side in one workgroup
FAR_SHAPES = [(63, 64), (65, 64), (67, 130), (193, 132), (257, 132), (33000, 66), (200003, 64)]
OUTLIER, FAR_PIVOT = 64.0, 25.0                              # FAR_PIVOT: the switch of column_mean_var, dm^2 > 25 var
# either side of the switch at the row count of the Stage-II patch embedding: row 0 this many standard deviations from the mean in the even / odd columns
EDGE_R, EDGE_SIGMAS = 262144, (4.8, 5.3)
KINK_MARGIN = 1e-5                                           # 100 x the float32 rounding of an output near zero


def launch(R, C):
    """-> (parts, rows_per_block, rows of the last part) as the entry points of pointnet.hip compute them"""
    cb = (C + 63) // 64
    parts = max(1, min((2048 + cb - 1) // cb, (R + 63) // 64, 1024))
    rpb = ((R + parts - 1) // parts + 3) // 4 * 4
    nparts = (R + rpb - 1) // rpb
    return nparts, rpb, R - (nparts - 1) * rpb


def workspace_floats(R, C):
    """act_colstats_workspace in floats: four rows of C per part (two pairs of sums in the statistics pass)"""
    cb = (C + 63) // 64
    return max(1, min((2048 + cb - 1) // cb, (R + 63) // 64, 1024)) * 4 * C


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice(R, C):
    """-> x [R,C] in {-4..4}, dy [R,C] in {-2..2} (about a third zeros), mean [C] in {-4..4}, k [C] in {-3..3}, float32 holding integers.
    With rstd = 0.5, scale = 1 and shift = k + 0.5 every product and sum of the backward is a multiple of 1/2 below 2^24: exact in any order."""
    r = np.random.default_rng(1000003 * R + 1009 * C)
    x = r.integers(-4, 5, (R, C))
    dy = r.choice(np.array([-2, -1, 1, 2]), (R, C))
    dy[r.random((R, C)) < 1.0 / 3.0] = 0
    mean, k = r.integers(-4, 5, C), r.integers(-3, 4, C)
    return _frozen(*(a.astype(np.float32) for a in (x, dy, mean, k)))


def lattice_affine(R, C):
    """the per-column operands of the backward on the lattice -> scale, shift, mean, rstd (float32)"""
    _, _, mean, k = lattice(R, C)
    return np.ones(C, np.float32), (k + np.float32(0.5)).astype(np.float32), mean, np.full(C, 0.5, np.float32)


@functools.lru_cache(maxsize=None)
def pivot_input(R, A):
    """x = 1.5 N(0,1) + 0.7 with row 0 set to A, and the same rows with row 0 swapped into row R / 2 (the same multiset per column)"""
    r = np.random.default_rng(977 * R + int(A))
    x = (1.5 * r.standard_normal((R, PIVOT_C)) + 0.7).astype(np.float32)
    x[0] = A
    y = x.copy()
    y[[0, R // 2]] = y[[R // 2, 0]]
    return _frozen(x, y)


@functools.lru_cache(maxsize=None)
def outlier_lattice(R, C):
    """lattice(R, C)'s x with row 0 of every third column set to OUTLIER, and the same rows with row 0 swapped into row R / 2"""
    x = lattice(R, C)[0].copy()
    x[0, ::3] = OUTLIER
    y = x.copy()
    y[[0, R // 2]] = y[[R // 2, 0]]
    return _frozen(x, y)


def pivot_ratio(x):
    """dm^2 / var per column in float64, dm = x[0] - mean: what column_mean_var compares with FAR_PIVOT"""
    mean, var = mean_var(x)
    return (np.asarray(x[0], np.float64) - mean) ** 2 / var


@functools.lru_cache(maxsize=None)
def edge_input():
    """x = 1.5 N(0,1) + 0.7 [EDGE_R, PIVOT_C] with row 0 placed EDGE_SIGMAS standard deviations above each column's mean (even / odd columns)"""
    r = np.random.default_rng(262144)
    x = (1.5 * r.standard_normal((EDGE_R, PIVOT_C)) + 0.7).astype(np.float32)
    for _ in range(3):                                        # (the row itself moves mean and spread a little)
        mean, var = mean_var(x)
        k = np.where(np.arange(PIVOT_C) % 2 == 0, EDGE_SIGMAS[0], EDGE_SIGMAS[1])
        x[0] = (mean + k * np.sqrt(var)).astype(np.float32)
    return _frozen(x)[0]


def part_stats(x, R, C):
    """(mean, M2) of every stage-1 part of x in float64 -> [nparts, C] each, and the parts' row counts"""
    nparts, rpb, _ = launch(R, C)
    xd = np.asarray(x, np.float64)
    ms, qs, ns = [], [], []
    for p in range(nparts):
        blk = xd[p * rpb:(p + 1) * rpb]
        ms.append(blk.mean(0)); qs.append(((blk - blk.mean(0)) ** 2).sum(0)); ns.append(blk.shape[0])
    return np.stack(ms), np.stack(qs), np.array(ns)


def kink_free(x, gamma, beta, margin=KINK_MARGIN, step=0.05, eps=BN_EPS):
    """x (float32) with the few elements whose train-mode BatchNorm output lies within ``margin`` of 0 moved by ``step``, until none is left: the
    derivative of the ReLU behind it is then the same in float32 and in float64, so one reference gradient exists"""
    x = np.array(x, dtype=np.float32)
    for _ in range(20):
        _, _, _, scale, shift = bn_train(x, gamma, beta, eps)
        near = np.abs(x.astype(np.float64) * scale + shift) < margin
        if not near.any():
            return x
        x[near] += np.float32(step)
    raise AssertionError("kink_free did not settle")


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------------------------------
def exact_mean_var(x):
    """mean and biased variance of integer-valued columns as exact rationals: int64 sums, divided in float64"""
    xi = np.asarray(x).astype(np.int64)
    assert np.array_equal(xi, np.asarray(x))
    R = xi.shape[0]
    s, q = xi.sum(0), (xi * xi).sum(0)
    return s / float(R), (R * q - s * s) / float(R) ** 2


def mean_var(x):
    """mean and biased variance of the columns in float64 (two passes)"""
    xd = np.asarray(x, dtype=np.float64)
    m = xd.mean(0)
    return m, ((xd - m) ** 2).mean(0)


def bn_train(x, gamma, beta, eps=BN_EPS):
    """-> mean, var (biased), rstd, scale = gamma rstd, shift = beta - mean scale"""
    mean, var = mean_var(x)
    rstd = 1.0 / np.sqrt(var + eps)
    scale = np.asarray(gamma, np.float64) * rstd
    return mean, var, rstd, scale, np.asarray(beta, np.float64) - mean * scale


def running(before, mean, var, R, momentum):
    """nn.BatchNorm1d's update of (running_mean, running_var): the unbiased variance, R / (R - 1)"""
    rm, rv = (np.asarray(a, np.float64) for a in before)
    unb = var * (R / (R - 1.0)) if R > 1 else var
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * unb


def affine_act(x, scale, shift, relu):
    y = np.asarray(x, np.float64) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    return np.maximum(y, 0.0) if relu else y


def _dyh(x, dy, scale, shift, relu):
    d = np.asarray(dy, np.float64)
    return d * (affine_act(x, scale, shift, False) > 0) if relu else d


def bwd_sums(x, dy, scale, shift, mean, rstd, relu):
    """-> sum_r dyh, sum_r dyh xhat      (dyh = relu ? dy (x scale + shift > 0) : dy, xhat = (x - mean) rstd)"""
    d = _dyh(x, dy, scale, shift, relu)
    xh = (np.asarray(x, np.float64) - np.asarray(mean, np.float64)) * np.asarray(rstd, np.float64)
    return d.sum(0), (d * xh).sum(0)


def bwd_sums_int(R, C, relu, rows=slice(None)):
    """the two sums on lattice(R, C) in int64: sum dyh and 2 sum dyh xhat  (rstd = 0.5), over ``rows``"""
    x, dy, mean, k = (a.astype(np.int64) for a in lattice(R, C))
    x, dy = x[rows], dy[rows]
    d = dy * (2 * (x + k) + 1 > 0) if relu else dy
    return d.sum(0), (d * (x - mean)).sum(0)


def bwd_apply(x, dy, scale, shift, mean, rstd, sum_dy, sum_dy_xhat, count, relu):
    """dx = scale (dyh - sum_dy / count - xhat sum_dy_xhat / count)"""
    d = _dyh(x, dy, scale, shift, relu)
    xh = (np.asarray(x, np.float64) - np.asarray(mean, np.float64)) * np.asarray(rstd, np.float64)
    return np.asarray(scale, np.float64) * (d - np.asarray(sum_dy, np.float64) / count - xh * np.asarray(sum_dy_xhat, np.float64) / count)


def bn_bwd(x, dy, scale, shift, mean, rstd, relu):
    """-> dx, dgamma, dbeta of BatchNorm(+ReLU) in train mode"""
    s1, s2 = bwd_sums(x, dy, scale, shift, mean, rstd, relu)
    return bwd_apply(x, dy, scale, shift, mean, rstd, s1, s2, float(np.asarray(x).shape[0]), relu), s2, s1


def eval_affine(gamma, beta, rm, rv, eps=BN_EPS):
    scale = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(rv, np.float64) + eps)
    return scale, np.asarray(beta, np.float64) - np.asarray(rm, np.float64) * scale


# ---- tile statistics ---------------------------------------------------------------------------------------------------------------------------
def tile_stats(X, tiles, rows_per_tile):
    """per-tile column (mean, M2) of X [tiles * rows_per_tile, C] in float64, rounded to float32 -> [tiles, 2, C]"""
    T = np.asarray(X, np.float64).reshape(tiles, rows_per_tile, -1)
    m = T.mean(1)
    return np.stack([m, ((T - m[:, None, :]) ** 2).sum(1)], axis=1).astype(np.float32)


def chan(ts, rows_per_tile):
    """Chan's combination of equal-count (mean, M2) partials [tiles, 2, C] in float64 -> mean, biased var"""
    ts = np.asarray(ts, np.float64)
    mean = ts[:, 0].mean(0)
    m2 = (ts[:, 1] + rows_per_tile * (ts[:, 0] - mean) ** 2).sum(0)
    return mean, m2 / (ts.shape[0] * rows_per_tile)


# ---- group kernels -----------------------------------------------------------------------------------------------------------------------------
def group_max(x, n):
    """x [G n, C] -> out [G, C] (x's dtype), arg int32 [G, C] = the first row of the group attaining it"""
    x = np.asarray(x)
    g = x.reshape(-1, n, x.shape[1])
    arg = g.argmax(1)
    return np.take_along_axis(g, arg[:, None, :], 1)[:, 0, :], arg.astype(np.int32)


def group_max_bwd(dout, arg, n):
    """din [G n, C] = dout[g, c] where arg[g, c] == row, else 0  (dout's dtype)"""
    dout = np.asarray(dout)
    G, C = dout.shape
    din = np.zeros((G, n, C), dout.dtype)
    np.put_along_axis(din, np.asarray(arg, np.int64)[:, None, :], dout[:, None, :], 1)
    return din.reshape(G * n, C)


def group_sum(x, n, dtype=np.float64):
    x = np.asarray(x)
    return x.reshape(-1, n, x.shape[1]).astype(dtype).sum(1)


@functools.lru_cache(maxsize=None)
def group_input(G, n, C):
    """x [G n, C] float32 for the max-pool with the planted cases that fit the shape -> x, {name: (group, column)}.  Column 0 of group 0: an exact tie
    of rows 0 and n - 1; column 1 % C of the last group: +0.0 in row 0 against -0.0 elsewhere ... every planted column is listed so that the test
    can say what it reached."""
    r = np.random.default_rng(31 * G + 7 * n + C)
    x = r.standard_normal((G * n, C)).astype(np.float32)
    v = x.reshape(G, n, C)
    planted = {}
    cols = list(range(min(C, 5)))
    if n > 1 and cols:
        c = cols.pop(0); v[0, :, c] = -1.0; v[0, 0, c] = 2.5; v[0, n - 1, c] = 2.5; planted["tie"] = (0, c)
    if n > 1 and cols:
        c = cols.pop(0); v[G - 1, :, c] = -0.0; v[G - 1, 0, c] = 0.0; planted["+0/-0 tie (+0 first)"] = (G - 1, c)
    if n > 1 and cols:
        c = cols.pop(0); v[G // 2, :, c] = 0.0; v[G // 2, 0, c] = -0.0; planted["-0/+0 tie (-0 first)"] = (G // 2, c)
    if cols:
        c = cols.pop(0); v[G - 1, :, c] = -np.inf; planted["all -inf"] = (G - 1, c)
    if cols:
        c = cols.pop(0); v[0, :, c] = np.arange(n, dtype=np.float32); planted["maximum in the last row"] = (0, c)
    return x, planted
