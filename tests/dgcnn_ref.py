"""numpy float64 references of csrc/dgcnn.hip: the edge-conv tail (gather + GroupNorm + LeakyReLU + max over the neighbours) and its backward,
the k = 1 head, the tokenizer kernels (hard gumbel arg-max + codebook row, soft gumbel-softmax, KL to uniform), plain restatements of the two host
dispatch rules, and the input builders that tests/test_gpu_dgcnn_edges.py and tests/test_dgcnn_host.py share.  No torch anywhere in this file.

Layout (that of the kernels): yz [B*G, ldy] with Y in columns [0, C) and Z in [zoff, zoff + C) (zoff < 0: no Z), idx int64 [B, k, G] (None: the
k = 1 head), pre[b, j, g, c] = Y[b, idx[b, j, g], c] + Z[b, g, c], GroupNorm statistics per (sample, group) over (k, G, C / groups)."""
import numpy as np

EPS, SLOPE = 1e-5, 0.2
GN_SPLIT, FAR_PIVOT = 8, 25.0


# ---------------------------------------------------------------------------------------------------------------- edge tail
def _pre(yz, zoff, idx, B, G, k, C):
    yz = np.asarray(yz, np.float64)
    Y = yz[:, :C].reshape(B, G, C)
    if idx is None:
        assert k == 1
        pre = Y[:, None]
    else:
        assert idx.shape == (B, k, G)
        pre = Y[np.arange(B)[:, None, None], idx]                   # [B, k, G, C]
    if zoff >= 0:
        pre = pre + yz[:, zoff:zoff + C].reshape(B, 1, G, C)
    return pre


def _stats(pre, groups, eps):
    B, k, G, C = pre.shape
    p5 = pre.reshape(B, k, G, groups, C // groups)
    mean = p5.mean(axis=(1, 2, 4))
    var = ((p5 - mean[:, None, None, :, None]) ** 2).mean(axis=(1, 2, 4))       # two passes: nothing cancels
    return mean, 1.0 / np.sqrt(var + eps)


def _per_channel(stat, C):
    """[B, groups] -> [B, 1, 1, C]"""
    return np.repeat(stat, C // stat.shape[1], axis=1)[:, None, None, :]


def edge_tail(yz, zoff, idx, B, G, k, C, groups, gamma, beta, eps=EPS, slope=SLOPE):
    """-> out [B*G, C], mean [B, groups], rstd [B, groups]: the reference formulation, max over j taken last"""
    pre = _pre(yz, zoff, idx, B, G, k, C)
    mean, rstd = _stats(pre, groups, eps)
    y = (pre - _per_channel(mean, C)) * _per_channel(rstd, C) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    act = np.where(y > 0, y, y * slope)
    return act.max(axis=1).reshape(B * G, C), mean, rstd


def _select(yz, idx, B, G, k, C, gamma):
    """edge_select: j* [B, G, C] = the first maximum of Y[b, idx[b, j, g], c] over j where gamma * rstd >= 0 (rstd > 0), else the first minimum"""
    if idx is None:
        return np.zeros((B, G, C), np.int64)
    Y = np.asarray(yz, np.float64)[:, :C].reshape(B, G, C)
    v = Y[np.arange(B)[:, None, None], idx]                         # [B, k, G, C]
    return np.where(np.asarray(gamma) >= 0, v.argmax(axis=1), v.argmin(axis=1))          # numpy returns the first extremum


def edge_tail_bwd(yz, zoff, idx, B, G, k, C, groups, gamma, beta, dout, eps=EPS, slope=SLOPE):
    """-> dyz [B*G, ldy] (columns outside Y and Z are 0), dgamma [C], dbeta [C] for the loss sum(out * dout)"""
    gamma, beta, dout = (np.asarray(a, np.float64) for a in (gamma, beta, dout))
    pre = _pre(yz, zoff, idx, B, G, k, C)
    mean, rstd = _stats(pre, groups, eps)
    rs = _per_channel(rstd, C)
    xhat = (pre - _per_channel(mean, C)) * rs                       # [B, k, G, C]
    js = _select(yz, idx, B, G, k, C, gamma)
    xs = np.take_along_axis(xhat, js[:, None], axis=1)[:, 0]        # [B, G, C]
    ysel = xs * gamma + beta
    da = dout.reshape(B, G, C) * np.where(ysel > 0, 1.0, slope)
    dgamma, dbeta = (da * xs).sum(axis=(0, 1)), da.sum(axis=(0, 1))
    cpg = C // groups
    n = float(cpg * G * k)
    gda = gamma * da
    m1 = gda.reshape(B, G, groups, cpg).sum(axis=(1, 3)) / n
    m2 = (gda * xs).reshape(B, G, groups, cpg).sum(axis=(1, 3)) / n
    onehot = np.arange(k)[None, :, None, None] == js[:, None]
    dpre = rs * (gda[:, None] * onehot - _per_channel(m1, C) - xhat * _per_channel(m2, C))
    dyz = np.zeros(np.asarray(yz).shape, np.float64)
    if zoff >= 0:
        dyz[:, zoff:zoff + C] = dpre.sum(axis=1).reshape(B * G, C)
    dY = np.zeros((B, G, C), np.float64)
    if idx is None:
        dY += dpre[:, 0]
    else:
        np.add.at(dY, (np.arange(B)[:, None, None], idx), dpre)
    dyz[:, :C] += dY.reshape(B * G, C)
    return dyz, dgamma, dbeta


def margins(yz, zoff, idx, B, G, k, C, groups, gamma, beta, eps=EPS, slope=SLOPE):
    """-> (the smallest |y| over the selected pre-activations, y = xhat * gamma + beta;
           the smallest gap between the best and the second-best neighbour value of a DIFFERENT source row, over (b, g, c); inf without one)"""
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    pre = _pre(yz, zoff, idx, B, G, k, C)
    mean, rstd = _stats(pre, groups, eps)
    xhat = (pre - _per_channel(mean, C)) * _per_channel(rstd, C)
    js = _select(yz, idx, B, G, k, C, gamma)
    xs = np.take_along_axis(xhat, js[:, None], axis=1)[:, 0]
    ymin = np.abs(xs * gamma + beta).min()
    if idx is None or k == 1:
        return ymin, np.inf
    Y = np.asarray(yz, np.float64)[:, :C].reshape(B, G, C)
    v = Y[np.arange(B)[:, None, None], idx] * np.where(gamma >= 0, 1.0, -1.0)            # the selection maximises this
    best = np.take_along_axis(v, js[:, None], axis=1)
    src = np.broadcast_to(idx[..., None], v.shape)
    other = src != np.take_along_axis(src, js[:, None], axis=1)
    gap = np.where(other, best - v, np.inf)
    return ymin, gap.min()


# --------------------------------------------------------------------------------------------------------- dispatch rules
def forward_path(G, k, C, groups, ldy, zoff, has_idx):
    """act_edge_gn_lrelu_max_f32, csrc/dgcnn.hip: the single-kernel condition (`if (fuse && idx && zoff >= 0 && (cpg & 3) == 0 && ...` with
    `smem = (2 G cpg + k G) * sizeof(float)`, yz itself 16-byte aligned as every torch allocation is), then the slab condition
    (`if (slab && idx && zoff >= 0 && k == 4 && (cpg % SW) == 0 && cpg / SW <= GN_SPLIT && smem <= 72 * 1024)` with SW = 32 and
    `smem = (G SW + 4 G) * sizeof(float)`), else the three generic kernels -- "head" where they run without a graph."""
    cpg = C // groups
    if has_idx and zoff >= 0 and cpg % 4 == 0 and ldy % 4 == 0 and zoff % 4 == 0 and (2 * G * cpg + k * G) * 4 <= 140 * 1024:
        return "fused"
    if has_idx and zoff >= 0 and k == 4 and cpg % 32 == 0 and cpg // 32 <= GN_SPLIT and (G * 32 + 4 * G) * 4 <= 72 * 1024:
        return "slab"
    return "generic" if has_idx else "head"


def backward_path(G, k, has_idx, lds=True):
    """act_edge_gn_lrelu_max_bwd_f32, csrc/dgcnn.hip: `use_lds = idx && G <= 128 && k == 4 && <switch on>` with `if (G <= 64) APPLY_LDS(.., 16) else
    APPLY_LDS(.., 32)`, then `else if (!idx)` (the head), then `if (G > 512) return ACT_E_BADARG` and
    `GL = G <= 128 ? 4 : (G <= 256 ? 2 : 1)` lane images.  lds: the state of act_edge_bwd_lds (on unless a test turns it off)."""
    if has_idx and G <= 128 and k == 4 and lds:
        return "lds16" if G <= 64 else "lds32"
    if not has_idx:
        return "head"
    if G > 512:
        return "refused"
    return "gl4" if G <= 128 else ("gl2" if G <= 256 else "gl1")


# ---------------------------------------------------------------------------------------------------------- input builders
def graph(rng, B, G, k):
    """a k-NN-like graph: neighbour 0 is the point itself, the others are any rows"""
    idx = rng.integers(0, G, size=(B, k, G), dtype=np.int64)
    idx[:, 0] = np.arange(G)
    return idx


def gammas(rng, C, groups, zero=True):
    """unit-normal gammas with, in every group, the first entry negative and (zero=True) the second exactly 0.0 where the group has two channels"""
    g = rng.standard_normal(C)
    g[np.abs(g) < 0.05] = 0.5
    cpg = C // groups
    for gi in range(groups):
        g[gi * cpg] = -abs(g[gi * cpg])
        if zero and cpg > 1:
            g[gi * cpg + 1] = 0.0
        elif zero and gi == 1:
            g[gi * cpg] = 0.0                                        # one channel per group: alternate between the two
    return g.astype(np.float32)


def forward_inputs(case):
    """case = dict(B, G, k, C, groups, ldy, zoff, idx (bool), seed) -> yz float32 [B*G, ldy], idx or None, gamma, beta (float32)"""
    B, G, k, C, groups = (case[n] for n in ("B", "G", "k", "C", "groups"))
    rng = np.random.default_rng(case["seed"])
    yz = rng.standard_normal((B * G, case["ldy"])).astype(np.float32)
    idx = graph(rng, B, G, k) if case["idx"] else None
    return yz, idx, gammas(rng, C, groups), (0.1 * rng.standard_normal(C)).astype(np.float32)


def separated(rng, B, G, C):
    """real-valued Y [B*G, C] whose rows differ by at least 1.5 / G in every column (a jittered permutation of a grid over [-1.5, 1.5]):
    no two different source rows are ever within 1e-4 of each other, whatever the graph"""
    out = np.empty((B, G, C))
    for b in range(B):
        order = np.argsort(rng.random((G, C)), axis=0)
        out[b] = (order + rng.uniform(0.25, 0.75, size=(G, C))) * (3.0 / G) - 1.5
    return out.reshape(B * G, C)


def clear_betas(yz, zoff, idx, B, G, k, C, groups, gamma, eps=EPS):
    """a beta per channel that keeps every selected y = xhat * gamma + beta away from 0: minus the midpoint of the widest gap that the channel's
    selected xhat * gamma leave inside [-0.3, 0.3] (0.1 if they leave that window empty).  beta moves neither the statistics nor the selection."""
    gamma = np.asarray(gamma, np.float64)
    pre = _pre(yz, zoff, idx, B, G, k, C)
    mean, rstd = _stats(pre, groups, eps)
    xhat = (pre - _per_channel(mean, C)) * _per_channel(rstd, C)
    js = _select(yz, idx, B, G, k, C, gamma)
    u = (np.take_along_axis(xhat, js[:, None], axis=1)[:, 0] * gamma).reshape(B * G, C)
    beta = np.empty(C)
    for c in range(C):
        s = np.sort(np.concatenate((u[:, c][np.abs(u[:, c]) < 0.3], [-0.3, 0.3])))
        i = np.argmax(np.diff(s))
        beta[c] = -0.5 * (s[i] + s[i + 1])
    return beta.astype(np.float32)


def backward_inputs(case):
    """case = dict(B, G, k, C, groups, idx (bool), seed, graph=None | "hub" | "same" | "k1", plant=None | d) -> yz [B*G, 2C] (C for the head), idx,
    gamma, beta, dout (float32).  Real-valued data built so that margins() is wide: separated() rows in Y, clear_betas() for beta."""
    B, G, k, C, groups = (case[n] for n in ("B", "G", "k", "C", "groups"))
    rng = np.random.default_rng(case["seed"])
    has_idx = case["idx"]
    Y = separated(rng, B, G, C)
    yz = np.concatenate((Y, rng.standard_normal((B * G, C))), axis=1) if has_idx else Y * (1 + rng.random(C)) + 0.3
    yz = yz.astype(np.float32)
    idx = graph(rng, B, G, k) if has_idx else None
    kind = case.get("graph")
    if kind == "hub":                                              # row 3 of sample 0 collects (k - 1) G + 1 edges; rows that lose their last edge get dY = 0
        idx[0, 1:] = 3
        idx[0, 0, 5:9] = 5                                         # (rows 6, 7, 8 are named by no edge; row 3 keeps its self edge)
    elif kind == "same":                                           # row 2's k neighbours are all row 7
        idx[:, :, 2] = 7
    zoff = C if has_idx else -1
    gamma = gammas(rng, C, groups, zero=False)
    if case.get("plant"):
        yz = plant(yz, zoff, idx, B, G, k, C, groups, case["plant"], "first")
    beta = clear_betas(yz, zoff, idx, B, G, k, C, groups, gamma)
    return yz, idx, gamma, beta, rng.standard_normal((B * G, C)).astype(np.float32)


def unnamed_rows(idx, G):
    """[B, G] bool: rows that no edge of their sample names"""
    return np.stack([~np.isin(np.arange(G), idx[b]) for b in range(idx.shape[0])])


def tie_inputs(case):
    """Y on the 1/8 lattice in [-1, 1] (equal values at different source rows are common), Z and dout integers, gamma in {+-1, +-2},
    beta in {+-0.5, +-1.5}"""
    B, G, k, C, groups = (case[n] for n in ("B", "G", "k", "C", "groups"))
    rng = np.random.default_rng(case["seed"])
    Y = rng.integers(-8, 9, size=(B * G, C)) / 8.0
    Z = rng.integers(-3, 4, size=(B * G, C)).astype(np.float64)
    gamma = rng.choice([-2.0, -1.0, 1.0, 2.0], size=C)
    gamma[0] = -1.0
    beta = rng.choice([-1.5, -0.5, 0.5, 1.5], size=C)
    dout = rng.integers(-2, 3, size=(B * G, C)).astype(np.float64)
    f = np.float32
    return np.concatenate((Y, Z), axis=1).astype(f), graph(rng, B, G, k), gamma.astype(f), beta.astype(f), dout.astype(f)


def plant(yz, zoff, idx, B, G, k, C, groups, d, where, column=False):
    """the far-pivot plantings, d in standard deviations of the untouched group.  column=False: ONE element of every (sample, group) is set so
    that its pre-activation lies d deviations above the group's mean -- where="first": Z[b, 0, c0] (h[b, 0, c0] without a graph), the element every
    statistics kernel takes as its pivot; where="last": Z[b, G - 1, c0 + cpg - 1], the same inputs met in the reverse order.
    column=True: d deviations are ADDED to the whole channel c0 (c0 + cpg - 1 for "last") of Z (of h)."""
    yz = np.array(yz, np.float32)
    pre = _pre(yz, zoff, idx, B, G, k, C)
    mean, rstd = _stats(pre, groups, 0.0)
    cpg = C // groups
    off = max(zoff, 0)
    for b in range(B):
        for gi in range(groups):
            sd = 1.0 / rstd[b, gi]
            c = gi * cpg + (0 if where == "first" else cpg - 1)
            if column:
                yz[b * G:(b + 1) * G, off + c] += np.float32(d * sd)
            else:
                g = 0 if where == "first" else G - 1
                src = g if idx is None else idx[b, 0, g]
                rest = float(yz[b * G + src, c]) if zoff >= 0 else 0.0
                yz[b * G + g, off + c] = np.float32(mean[b, gi] + d * sd - rest)
    return yz


def pivot_ratio(yz, zoff, idx, B, G, k, C, groups):
    """dm^2 / var per (sample, group) in float64, dm = mean - pivot: the quantity the kernels compare with FAR_PIVOT"""
    pre = _pre(yz, zoff, idx, B, G, k, C)
    mean, rstd = _stats(pre, groups, 0.0)
    cpg = C // groups
    pv = pre[:, 0, 0, ::cpg]
    return (mean - pv) ** 2 * rstd ** 2


# ------------------------------------------------------------------------------------------------------------- tokenizer
def gumbel_argmax_gather(h, B, G, C, groups, gamma, beta, noise, tau, codebook, eps=EPS, slope=SLOPE):
    """-> logits [B*G, C] = LeakyReLU(GroupNorm(h)), index [B*G] = first arg-max of (logits + noise) / tau, codes = codebook[index],
    gap [B*G] between the two largest scores of a row, mean, rstd"""
    logits, mean, rstd = edge_tail(h, -1, None, B, G, 1, C, groups, gamma, beta, eps, slope)
    score = (logits + np.asarray(noise, np.float64).reshape(B * G, C)) / tau
    index = score.argmax(axis=1)
    top = np.sort(score, axis=1)[:, -2:] if C > 1 else np.concatenate((score - np.inf, score), axis=1)
    return logits, index, np.asarray(codebook)[index], top[:, 1] - top[:, 0], mean, rstd


def gumbel_softmax(logits, noise, tau):
    t = (np.asarray(logits, np.float64) + np.asarray(noise, np.float64)) / tau
    e = np.exp(t - t.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def gumbel_softmax_bwd(y, dy, tau):
    y, dy = np.asarray(y, np.float64), np.asarray(dy, np.float64)
    return y * (dy - (y * dy).sum(axis=-1, keepdims=True)) / tau


def _softmax_rows(logits):
    z = np.asarray(logits, np.float64)
    m = z.max(axis=-1, keepdims=True)
    lse = m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True))
    return np.exp(z - lse)


def kl_uniform(logits):
    """logits [B, G, C] -> KL(mean_g softmax || uniform), 'batchmean'"""
    B, G, C = logits.shape
    qbar = _softmax_rows(logits).mean(axis=1)
    u = 1.0 / C
    return (u * (np.log(u) - np.log(qbar))).sum() / B


def kl_uniform_bwd(logits, gout=1.0):
    B, G, C = logits.shape
    p = _softmax_rows(logits)
    w = gout * (-(1.0 / C) / (B * p.mean(axis=1, keepdims=True))) / G        # d klv / d p[b, g, c]
    return p * (w - (p * w).sum(axis=-1, keepdims=True))
