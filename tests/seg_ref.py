"""numpy references for the dense-prediction kernels (csrc/seg.hip and the three-NN feature propagation of csrc/sa.hip; not a test itself).
``three_nn_f32`` restates the three-NN kernel and its inverse adjacency operation for operation in float32, so every output is expected bit
for bit (tests/fp_ref.py restates the same kernel independently; tests/test_fp_host.py holds the two to each other).  The other functions are float64 references of
the float32 inputs the device gets; each also returns the componentwise sum of absolute values of the terms it adds, which is what a rounding
bound of a float32 summation is proportional to.  Rows whose target lies outside [0, C) are ignored."""
import numpy as np

U = 2.0 ** -24                      # unit roundoff of float32


# ---- three nearest centres, float32, bit for bit -----------------------------------------------------------------------------------------
def sqdist_f32(xyz, ctr):
    """float32 [N, G]: (dx*dx + dy*dy) + dz*dz, one rounding per operation (common.h, sqdist3)"""
    xyz = np.asarray(xyz, dtype=np.float32)
    ctr = np.asarray(ctr, dtype=np.float32)
    dx = xyz[:, None, 0] - ctr[None, :, 0]
    dy = xyz[:, None, 1] - ctr[None, :, 1]
    dz = xyz[:, None, 2] - ctr[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def adjacency(idx, G):
    """idx int [B, N, 3] -> (off int32 [B, G+1], ent int32 [B, 3N]): per cloud and centre the entries e = 3n+k that chose it, increasing e"""
    B, N, _ = idx.shape
    off = np.zeros((B, G + 1), np.int32)
    ent = np.zeros((B, 3 * N), np.int32)
    for b in range(B):
        flat = idx[b].ravel()
        pos = 0
        for g in range(G):
            e = np.where(flat == g)[0]
            ent[b, pos:pos + e.size] = e
            pos += e.size
            off[b, g + 1] = pos
        assert pos == 3 * N
    return off, ent


def three_nn_f32(xyz, ctr):
    """xyz float32 [B, N, 3], ctr float32 [B, G, 3] -> (idx int32 [B,N,3], w float32 [B,N,3], off int32 [B,G+1], ent int32 [B,3N], d float32
    [B,N,3]).  Selection: the first three of a stable argsort over increasing centre index (the kernel's strict '<' insertion keeps the lower
    index among equal distances).  Weights: r = 1 / (d + 1e-8f), s = (r0 + r1) + r2, w = r / s, every operation rounded to float32.
    G < 3: the kernel's registers of the slots that never fill stay at idx 0 and d = +inf, so r = 1 / inf = 0 and w = 0 exactly."""
    xyz = np.asarray(xyz, dtype=np.float32)
    ctr = np.asarray(ctr, dtype=np.float32)
    B, N, _ = xyz.shape
    G = ctr.shape[1]
    idx = np.zeros((B, N, 3), np.int32)
    d3 = np.full((B, N, 3), np.inf, np.float32)
    for b in range(B):
        d = sqdist_f32(xyz[b], ctr[b])
        o = np.argsort(d, axis=-1, kind="stable")[:, :3]
        idx[b, :, :o.shape[1]] = o
        d3[b, :, :o.shape[1]] = np.take_along_axis(d, o, -1)
    one, eps = np.float32(1.0), np.float32(1e-8)
    r = one / (d3 + eps)
    s = (r[..., 0] + r[..., 1]) + r[..., 2]
    w = r / s[..., None]
    assert r.dtype == np.float32 and w.dtype == np.float32
    off, ent = adjacency(idx, G)
    return idx, w, off, ent, d3


def three_nn_order_f64(xyz, ctr):
    """float64 distances of the float32 inputs -> (stable ascending order [B,N,G], d [B,N,G])"""
    d = ((np.asarray(xyz)[:, :, None, :].astype(np.float64) - np.asarray(ctr)[:, None, :, :].astype(np.float64)) ** 2).sum(-1)
    return np.argsort(d, axis=-1, kind="stable"), d


def near_tie_clouds(B, n, m, seed):
    """points + centres on a coarse lattice (coordinates k / 64) with {0, 1, 2} * 2^-22 perturbations: many exactly equal and
    last-bit-different distances (the recipe of _near_tie_clouds in test_gpu_point_ops.py)"""
    rs = np.random.RandomState(seed)
    x = (rs.randint(-40, 41, (B, n, 3)) / 64.0).astype(np.float32) + (rs.randint(0, 3, (B, n, 3)) * 2.0 ** -22).astype(np.float32)
    y = (rs.randint(-40, 41, (B, m, 3)) / 64.0).astype(np.float32) + (rs.randint(0, 3, (B, m, 3)) * 2.0 ** -22).astype(np.float32)
    return x, y


# (B, N, G, seed) of the near-tie three-NN cases: a lattice of 81^3 positions needs on the order of a hundred centres before equal distances
# among the four nearest are common (three or five centres give none), so the ragged sizes here are those of the larger G
NEAR_TIE_CASES = [(2, 1000, 127, 13), (1, 683, 512, 14), (2, 700, 511, 15), (3, 257, 130, 16)]


def rows_with_ties(xyz, ctr):
    """bool [B, N]: the four smallest float32 distances of the row hold two equal values"""
    out = np.zeros(xyz.shape[:2], bool)
    for b in range(xyz.shape[0]):
        d = np.sort(sqdist_f32(xyz[b], ctr[b]), axis=-1)[:, :4]
        out[b] = (np.diff(d, axis=-1) == 0).any(-1)
    return out


# ---- row interpolation ---------------------------------------------------------------------------------------------------------------------
def _rows(idx, B, N, G):
    return (np.asarray(idx).astype(np.int64) + (np.arange(B, dtype=np.int64) * G)[:, None, None]).reshape(B * N, 3)


def interp_fwd_f64(P, idx, w, B, N, G, xyz=None, wxyz=None, bias=None):
    """Y[b*N+n] = sum_k w[n,k] P[b*G + idx[n,k]] (+ xyz[n] . wxyz^T + bias) -> (Y [B*N,C], A [B*N,C]) with
    A = sum_k |w_k P_k| + sum_j |xyz_j wxyz_cj| + |bias_c|"""
    P = np.asarray(P, dtype=np.float64)
    rows = _rows(idx, B, N, G)
    w = np.asarray(w, dtype=np.float64).reshape(B * N, 3)
    Y = np.zeros((B * N, P.shape[1]))
    A = np.zeros_like(Y)
    for k in range(3):
        t = w[:, k, None] * P[rows[:, k]]
        Y += t
        A += np.abs(t)
    if wxyz is not None:
        xyz = np.asarray(xyz, dtype=np.float64).reshape(B * N, 3)
        wxyz = np.asarray(wxyz, dtype=np.float64)
        Y += xyz @ wxyz.T
        A += np.abs(xyz) @ np.abs(wxyz).T
    if bias is not None:
        bias = np.asarray(bias, dtype=np.float64)
        Y += bias
        A += np.abs(bias)
    return Y, A


def interp_bwd_f64(dY, idx, w, B, N, G):
    """dP[b*G+g] = sum over the entries e = 3n+k with idx[b,n,k] == g of w[e] dY[b*N+n] -> (dP [B*G,C], A [B*G,C], L [B*G]) with
    A = sum_e |w_e dY_e| and L the number of entries of the centre"""
    dY = np.asarray(dY, dtype=np.float64)
    rows = _rows(idx, B, N, G)
    w = np.asarray(w, dtype=np.float64).reshape(B * N, 3)
    dP = np.zeros((B * G, dY.shape[1]))
    A = np.zeros_like(dP)
    for k in range(3):
        t = w[:, k, None] * dY
        np.add.at(dP, rows[:, k], t)
        np.add.at(A, rows[:, k], np.abs(t))
    L = np.bincount(rows.ravel(), minlength=B * G)
    return dP, A, L


def xyz_grad_f64(dY, xyz):
    """-> (dw [C,3] = dY^T xyz, db [C] = column sums of dY, Aw [C,3] = |dY|^T |xyz|, Ab [C] = column sums of |dY|)"""
    dY = np.asarray(dY, dtype=np.float64)
    xyz = np.asarray(xyz, dtype=np.float64)
    return dY.T @ xyz, dY.sum(0), np.abs(dY).T @ np.abs(xyz), np.abs(dY).sum(0)


# ---- log-softmax ---------------------------------------------------------------------------------------------------------------------------
def log_softmax_f64(z):
    """z [R, C] (entries may be -inf, not a whole row) -> (out [R,C], lse [R])"""
    z = np.asarray(z, dtype=np.float64)
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1))
    return z - lse[:, None], lse


def log_softmax_fwd_bound(out, lse, C):
    """U (|out| + |lse| + C + 16) per element: one rounding each of m + log s and z - lse, C + 2 for the sum of exps, slack for two-ulp
    expf / logf.  Infinite where out is -inf (those elements are compared exactly instead)."""
    return U * (np.abs(out) + np.abs(lse)[:, None] + C + 16)


def log_softmax_bwd_f64(logp, g):
    """dz = g - exp(logp) sum_c g of the float32 log-probabilities the backward kernel is given -> (dz [R,C], p [R,C], sum_c |g| [R])"""
    logp = np.asarray(logp, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    p = np.exp(logp)
    return g - p * g.sum(1, keepdims=True), p, np.abs(g).sum(1)


def log_softmax_bwd_bound(g, p, sabs, C):
    """U (|g_c| + (C + 4) p_c sum|g|): C - 1 roundings of the row sum, two ulps of expf, the product and the subtraction"""
    return U * (np.abs(np.asarray(g, dtype=np.float64)) + (C + 4) * p * sabs[:, None])


# ---- weighted-mean NLL, confusion matrix -----------------------------------------------------------------------------------------------------
def valid_rows(tgt, C):
    tgt = np.asarray(tgt)
    return (tgt >= 0) & (tgt < C)


def nll_f64(logp, tgt, weight, C):
    """-> dict(num, den, Anum, Aden, loss, correct, valid): num = sum_r w[t_r] (-logp[r, t_r]) and den = sum_r w[t_r] over the rows with a
    target in [0, C); A* the same sums over absolute values; correct = number of valid rows whose first arg-max equals the target"""
    logp = np.asarray(logp)
    tgt = np.asarray(tgt).astype(np.int64)
    v = valid_rows(tgt, C)
    t = tgt[v]
    lp = logp[v][np.arange(t.size), t].astype(np.float64)
    wt = np.ones(t.size) if weight is None else np.asarray(weight, dtype=np.float64)[t]
    num, den = float((-wt * lp).sum()), float(wt.sum())
    correct = int((logp[v].argmax(1) == t).sum()) if t.size else 0
    return dict(num=num, den=den, Anum=float(np.abs(wt * lp).sum()), Aden=float(np.abs(wt).sum()), loss=num / den if t.size else float("nan"),
                correct=correct, valid=v)


def nll_terms(R):
    """number of float32 roundings on the longest path of the kernel's fixed map: the per-lane stride loop, the eight-level tree of a block,
    the ordered pass over the nb <= 512 block partials"""
    nb = min(512, (R + 255) // 256)
    return -(-R // (nb * 256)) + 8 + nb


def nll_bwd_f64(tgt, weight, wsum, g, R, C):
    """dlogp[r, c] = -g w[t_r] / wsum at c == t_r of the valid rows, zero elsewhere (wsum: the float32 denominator the kernel is given)"""
    tgt = np.asarray(tgt).astype(np.int64)
    v = valid_rows(tgt, C)
    out = np.zeros((R, C))
    t = tgt[v]
    wt = np.ones(t.size) if weight is None else np.asarray(weight, dtype=np.float64)[t]
    out[np.where(v)[0], t] = -(float(g) * wt) / float(wsum)
    return out


def confusion_ref(pred, tgt, C):
    """int64 [C, C]: counts of (target, first arg-max of the row) over the rows with a target in [0, C)"""
    pred = np.asarray(pred)
    tgt = np.asarray(tgt).astype(np.int64)
    v = valid_rows(tgt, C)
    cm = np.zeros((C, C), np.int64)
    np.add.at(cm, (tgt[v], pred[v].argmax(1)), 1)
    return cm


def mixed_targets(rs, R, C, frac=0.3):
    """int64 [R]: targets in [0, C) with about ``frac`` of the rows replaced by one of {-100, -1, C, 255} (all outside [0, C), C <= 64)"""
    t = rs.randint(0, C, size=R).astype(np.int64)
    ign = rs.rand(R) < frac
    t[ign] = np.array([-100, -1, C, 255], np.int64)[rs.randint(0, 4, size=int(ign.sum()))]
    return t


# ---- inputs shared by the host and the GPU tests ---------------------------------------------------------------------------------------------
def softmax_inputs(kind, R, C, seed):
    """the value classes of the GPU test (float32 [R, C])"""
    rs = np.random.RandomState(seed)
    z = (3 * rs.standard_normal((R, C))).astype(np.float32)
    if kind == "large":
        z = (z * np.float32(1e4 / 3)).astype(np.float32)
    elif kind == "constant":
        z = np.repeat((1e3 * rs.standard_normal((R, 1))).astype(np.float32), C, axis=1)
    elif kind == "dominant":
        z[np.arange(R), rs.randint(0, C, size=R)] += np.float32(150.0)      # gap > 104: every other exp underflows to zero in float32
    elif kind == "neginf":
        if C > 1:
            m = rs.rand(R, C) < 0.3
            m[np.arange(R), rs.randint(0, C, size=R)] = False               # never a whole row
            z[m] = -np.inf
    else:
        assert kind == "randn"
    return z


KINDS = ["randn", "large", "constant", "dominant", "neginf"]
