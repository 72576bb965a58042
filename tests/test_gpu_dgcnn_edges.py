"""GPU: csrc/dgcnn.hip where tests/test_gpu_dense.py does not reach it.  Forward: every form that act_edge_gn_lrelu_max_f32 dispatches to by shape
(single kernel, slab, the three generic kernels with a graph, the k = 1 head) on both sides of the 140 KB and G = 512 bounds, at one, two and eight
slabs per group, with empty statistics splits and past one trip of the grid-stride loops; a first element (the statistics' pivot) or a first
channel 5 - 1000 deviations away from its group, the same inputs met in the reverse order, and either side of the FAR_PIVOT switch.  Backward: both
LDS instantiations and the three scatter-image widths one past each boundary, hubs, rows without edges, repeated neighbours, k = 1 with a graph,
exact ties between different source rows under both forms, the refusal at G > 512.  Tokenizer: the soft gumbel-softmax, the KL term and the
arg-max at their stride and refusal boundaries.  Every argument check of the seven entry points.

Bars are those of test_dgcnn_edge_tail_* (2e-5 forward, 5e-5 backward), taken ELEMENTWISE as |got - ref| / max(1, |ref|): a planted outlier makes
the tensor's largest entry about 1000, and dividing by it would hide every other element.  References: tests/dgcnn_ref.py (numpy float64, checked
on the CPU by tests/test_dgcnn_host.py, which also proves that the tables below reach every path and that the backward inputs keep every
LeakyReLU side and every arg-max at least 1e-4 clear, so nothing is excluded from any comparison).  No environment switch is set: the paths are
chosen by shape.  Every test prints what it measured before it asserts."""

import numpy as np
import pytest
import torch

from tests import dgcnn_ref as R

pytestmark = pytest.mark.gpu

ACT_E_BADARG, ACT_E_NULLPTR = -1, -2
FWD, BWD = 2e-5, 5e-5                                           # the bars of test_dgcnn_edge_tail_and_head / _backward
MEAN, RSTD = 1e-6, 2e-5                                         # saved statistics against float64
SENT, GUARD = 7.0, 64                                           # sentinel value around the output / behind the statistics workspace
FAR_D = (5, 30, 300, 1000)


def _fwd(path, G, k, C, B=2, groups=4, odd_ldy=False, idx=True):
    """odd_ldy: yz has 2C + 1 columns, which keeps a shape off the single-kernel form"""
    ldy = (2 * C + 1 if odd_ldy else 2 * C) if idx else C
    return dict(path=path, B=B, G=G, k=k, C=C, groups=groups, ldy=ldy, zoff=C if idx else -1, idx=idx, seed=1000 + G * 7 + C + k)


FORWARD = [
    _fwd("fused", 1, 1, 16, B=3),
    _fwd("fused", 5, 3, 16, B=3),
    _fwd("fused", 300, 4, 64),                                   # k G = 1200 > 1024: a second trip of the index staging; G cpg / 4 = 1200 is no multiple of 1024
    _fwd("fused", 271, 4, 256),                                  # 143,088 B: the last shape under the 140 KB rule
    _fwd("slab", 272, 4, 256),                                   # the first shape over it, G % 8 == 0
    _fwd("slab", 273, 4, 256),                                   # G % 8 != 0
    _fwd("slab", 512, 4, 1024, B=1),                             # eight slabs per group: every GN_SPLIT slot is written; 72 KB of LDS exactly
    _fwd("slab", 64, 4, 128, odd_ldy=True),                      # cpg = 32: one slab per group, slab 0 zeroes seven slots
    _fwd("generic", 513, 4, 256),                                # one past the slab bound
    _fwd("generic", 600, 3, 256),                                # k != 4, too large for the single kernel
    _fwd("generic", 64, 4, 288, groups=1),                       # nine slabs > GN_SPLIT (148,480 B: too large for the single kernel)
    _fwd("generic", 20, 4, 24),                                  # cpg = 6
    _fwd("generic", 7, 2, 12, groups=3, odd_ldy=True),           # G k cpg = 56 < 256: seven of the eight statistics splits are empty (cpg = 4 with an even
                                                                 # row stride would take the single kernel)
    _fwd("generic", 513, 4, 1024, B=5),                          # B G C > 8192 x 256: second grid-stride trip of the apply kernel; yz is 21 MB
    _fwd("head", 1, 1, 8, B=3, idx=False),
    _fwd("head", 33, 1, 24, B=3, idx=False),
    _fwd("head", 64, 1, 8192, idx=False),                        # the tokenizer's width
    _fwd("head", 513, 1, 1024, B=5, idx=False),                  # second grid-stride trip
]
# far pivots: one representative of each forward form at cpg = 64 and, where the form allows it, at cpg = 4
FAR = [
    _fwd("fused", 5, 3, 16), _fwd("fused", 271, 4, 256, B=1),
    _fwd("slab", 272, 4, 256, B=1),
    _fwd("generic", 7, 2, 12, groups=3, odd_ldy=True), _fwd("generic", 513, 4, 256, B=1),
    _fwd("head", 33, 1, 16, idx=False), _fwd("head", 33, 1, 256, idx=False),
    _fwd("token", 16, 1, 16, idx=False), _fwd("token", 16, 1, 256, idx=False),
]
PLANTINGS = [("element", "first"), ("element", "last"), ("column", "first"), ("column", "last")]
SWITCH = [c for c in FAR if c["C"] == 256]                       # either side of FAR_PIVOT, every form
SWITCH_D = (4.8, 5.2)


def _bwd(path, G, k, C, B=2, groups=4, idx=True, graph=None, plant=None):
    return dict(path=path, B=B, G=G, k=k, C=C, groups=groups, idx=idx, graph=graph, plant=plant, seed=2000 + G * 5 + C + k)


BACKWARD = [
    _bwd("lds16", 64, 4, 96),                                    # the last 64-channel block is half full
    _bwd("lds32", 65, 4, 64),
    _bwd("lds32", 128, 4, 24),                                   # cpg = 6
    _bwd("gl4", 64, 3, 64),
    _bwd("gl4", 128, 5, 64),
    _bwd("gl2", 129, 4, 64),
    _bwd("gl2", 256, 4, 64),
    _bwd("gl1", 257, 4, 64),
    _bwd("gl1", 512, 3, 64, B=1),
    _bwd("head", 33, 1, 24, idx=False),
    _bwd("head", 64, 1, 8192, B=1, idx=False),
    _bwd("lds16", 64, 4, 96, graph="hub"),                       # a row with (k - 1) G + 1 edges, three rows with none
    _bwd("gl4", 64, 3, 64, graph="hub"),
    _bwd("lds32", 65, 4, 64, graph="same"),                      # a row whose k neighbours are one source
    _bwd("gl2", 129, 4, 64, graph="same"),
    _bwd("gl4", 64, 1, 64),                                      # k = 1 with a graph
    _bwd("lds16", 64, 4, 96, plant=300),                         # the backward consumes the saved statistics of a far pivot
    _bwd("gl2", 129, 4, 64, plant=300),
]
REFUSED = _bwd("refused", 513, 4, 64, B=1)
TIES = [_bwd("lds16", 64, 4, 64), _bwd("lds32", 128, 4, 64), _bwd("gl2", 129, 4, 64)]
TOKEN_SEED = 77


def _id(c):
    tag = "".join(f"-{n}{c[n]}" for n in ("graph", "plant") if c.get(n))
    return f"{c['path']}-{c['B']}x{c['G']}x{c['k']}x{c['C']}g{c['groups']}{tag}"


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available()
    import act_amd.kernels as K
    return K


def _st():
    return torch.cuda.current_stream().cuda_stream


def _d(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _n(t):
    return t.detach().double().cpu().numpy()


def _p(t):
    return None if t is None else t.data_ptr()


def _err(got, ref):
    """the largest elementwise |got - ref| / max(1, |ref|)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()) if ref.size else 0.0


def _geom(c):
    return c["B"], c["G"], c["k"], c["C"], c["groups"]


def _forward(K, c, yz, idx, gamma, beta):
    """act_edge_gn_lrelu_max_f32 into a wider buffer at a non-zero column offset -> out [B*G, C], mean, rstd [B, groups] (numpy float64)"""
    B, G, k, C, groups = _geom(c)
    ooff = 1 if c["path"] == "generic" else 40
    buf = torch.full((B * G, ooff + C + 3), SENT, device="cuda")
    stats = torch.full((18 * B * groups + GUARD,), SENT, device="cuda")
    t = [_d(yz), _d(idx, torch.int64), _d(gamma), _d(beta)]
    rc = K.lib.act_edge_gn_lrelu_max_f32(_p(t[0]), c["ldy"], c["zoff"], _p(t[1]), B, G, k, C, groups, _p(t[2]), _p(t[3]), R.EPS, R.SLOPE,
                                         stats.data_ptr(), buf.data_ptr(), buf.stride(0), ooff, _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert (buf[:, :ooff] == SENT).all() and (buf[:, ooff + C:] == SENT).all(), "columns beside the output were written"
    assert (stats[18 * B * groups:] == SENT).all(), "the kernels wrote past 18 B groups floats of statistics workspace"
    st = _n(stats)
    return _n(buf[:, ooff:ooff + C]), st[:B * groups].reshape(B, groups), st[B * groups:2 * B * groups].reshape(B, groups)


def _tokenizer(K, B, G, C, groups, h, gamma, beta, noise, tau, codebook):
    """act_gn_gumbel_argmax_gather_f32 with injected noise -> codes, index, logits, mean, rstd"""
    D = codebook.shape[1]
    stats = torch.full((18 * B * groups + GUARD,), SENT, device="cuda")
    index = torch.full((B * G,), -1, dtype=torch.int64, device="cuda")
    out = torch.full((B * G, D), SENT, device="cuda"); logits = torch.full((B * G, C), SENT, device="cuda")
    t = [_d(h), _d(gamma), _d(beta), _d(noise), _d(codebook)]
    rc = K.lib.act_gn_gumbel_argmax_gather_f32(_p(t[0]), B, G, C, groups, _p(t[1]), _p(t[2]), R.EPS, R.SLOPE, _p(t[3]), 0, None, tau, _p(t[4]), D,
                                               stats.data_ptr(), index.data_ptr(), out.data_ptr(), logits.data_ptr(), _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert (stats[18 * B * groups:] == SENT).all()
    st = _n(stats)
    return _n(out), index.cpu().numpy(), _n(logits), st[:B * groups].reshape(B, groups), st[B * groups:2 * B * groups].reshape(B, groups)


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("c", FORWARD, ids=_id)
def test_forward_on_every_dispatch_path(K, c):
    B, G, k, C, groups = _geom(c)
    assert R.forward_path(G, k, C, groups, c["ldy"], c["zoff"], c["idx"]) == c["path"]
    yz, idx, gamma, beta = R.forward_inputs(c)
    cpg = C // groups
    assert all((gamma[g * cpg:(g + 1) * cpg] < 0).any() for g in range(groups)) and (gamma == 0).sum() >= (groups if cpg > 1 else 1)
    ref, mean, rstd = R.edge_tail(yz, c["zoff"], idx, B, G, k, C, groups, gamma, beta)
    out, m, r = _forward(K, c, yz, idx, gamma, beta)
    e = _err(out, ref), _err(m, mean), float((np.abs(r - rstd) / rstd).max())
    print(f"[dgcnn fwd] {_id(c)}: out {e[0]:.2e} (bar {FWD:.0e})  mean {e[1]:.2e} (bar {MEAN:.0e})  rstd {e[2]:.2e} (bar {RSTD:.0e})")
    assert e[0] <= FWD and e[1] <= MEAN and e[2] <= RSTD


def _far_inputs(c, kind, where, d):
    """-> yz (h), idx, gamma, beta of a FAR case with one planting at distance d"""
    B, G, k, C, groups = _geom(c)
    yz, idx, gamma, beta = R.forward_inputs(c)
    return R.plant(yz, c["zoff"], idx, B, G, k, C, groups, d, where, column=kind == "column"), idx, gamma, beta


def token_noise_and_codebook(c):
    rng = np.random.default_rng(TOKEN_SEED + c["C"])
    u = rng.random((c["B"] * c["G"], c["C"]))
    return (-np.log(-np.log(u * (1 - 2e-7) + 1e-7))).astype(np.float32), rng.standard_normal((c["C"], 12)).astype(np.float32)


def _far_bar(ref, mean, rstd, gamma, B, G, C):
    """2e-5 elementwise plus the rounding of the stored float32 mean, 2^-23 |mean| rstd |gamma[c]|, which no float32 kernel can avoid"""
    per = lambda s: np.repeat(np.repeat(s, C // s.shape[1], axis=1), G, axis=0)                  # [B, groups] -> [B*G, C]
    return FWD * np.maximum(1.0, np.abs(ref)) + 2.0 ** -23 * np.abs(per(mean)) * per(rstd) * np.abs(gamma)


def _far_run(K, c, yz, idx, gamma, beta):
    """-> worst (error / bar) of the output over the elements, relative error of rstd, left-out fraction of the tokenizer's rows (else 0)"""
    B, G, k, C, groups = _geom(c)
    if c["path"] == "token":
        noise, cb = token_noise_and_codebook(c)
        ref, rindex, rcodes, gap, mean, rstd = R.gumbel_argmax_gather(yz, B, G, C, groups, gamma, beta, noise, 1.0, cb)
        codes, index, out, m, r = _tokenizer(K, B, G, C, groups, yz, gamma, beta, noise, 1.0, cb)
        sure = gap > 1e-4
        assert np.array_equal(index[sure], rindex[sure]) and np.array_equal(codes[sure], rcodes[sure].astype(np.float64))
        left = 1.0 - sure.mean()
    else:
        ref, mean, rstd = R.edge_tail(yz, c["zoff"], idx, B, G, k, C, groups, gamma, beta)
        out, m, r = _forward(K, c, yz, idx, gamma, beta)
        left = 0.0
    return float((np.abs(out - ref) / _far_bar(ref, mean, rstd, gamma, B, G, C)).max()), float((np.abs(r - rstd) / rstd).max()), left


@pytest.mark.parametrize("kind,where", PLANTINGS, ids=[f"{a}-{b}" for a, b in PLANTINGS])
@pytest.mark.parametrize("c", FAR, ids=_id)
def test_far_pivot(K, c, kind, where):
    """(a) one element of every group, (b) one whole channel, 5 - 1000 deviations away; "first": it is the statistics' pivot, "last": the same inputs
    met in the reverse order"""
    bad = []
    for d in FAR_D:
        worst, rs, left = _far_run(K, c, *_far_inputs(c, kind, where, d))
        print(f"[dgcnn far pivot] {_id(c)} {kind} {where} d={d}: out {worst:.3f} of its bar (2e-5 + mean rounding)  rstd {rs:.2e} (bar {RSTD:.0e})"
              f"  rows left out {left:.4f}")
        if not (worst <= 1.0 and rs <= RSTD and left <= 0.01):
            bad.append((d, worst, rs, left))
    assert not bad, bad


@pytest.mark.parametrize("c", SWITCH, ids=_id)
def test_either_side_of_the_far_pivot_switch(K, c):
    """a first element 4.8 deviations out keeps the single-pass arithmetic (dm^2 < 25 var), one 5.2 out takes the second pass: the same bars hold on
    both sides, and the error just short of the switch is printed"""
    B, G, k, C, groups = _geom(c)
    for d, past in zip(SWITCH_D, (False, True)):
        yz, idx, gamma, beta = _far_inputs(c, "element", "first", d)
        ratio = R.pivot_ratio(yz, c["zoff"], idx, B, G, k, C, groups)
        assert (ratio > R.FAR_PIVOT * 1.02).all() if past else (ratio < R.FAR_PIVOT * 0.98).all(), ratio
        worst, rs, _ = _far_run(K, c, yz, idx, gamma, beta)
        print(f"[dgcnn switch] {_id(c)} d={d} (dm^2/var {ratio.min():.1f} - {ratio.max():.1f}, {'past' if past else 'short of'} the switch):"
              f" out {worst:.3f} of its bar  rstd {rs:.2e} (bar {RSTD:.0e})")
        assert worst <= 1.0 and rs <= RSTD


# ----------------------------------------------------------------------------------------------------------------- backward
def _backward(K, c, yz, idx, gamma, beta, dout):
    """EdgeGnLreluMaxFn forward + backward -> out, dyz, dgamma, dbeta (device tensors)"""
    B, G, k, C, groups = _geom(c)
    yg = _d(yz).requires_grad_(True); gm = _d(gamma).requires_grad_(True); bt = _d(beta).requires_grad_(True)
    out = K.EdgeGnLreluMaxFn.apply(yg, gm, bt, _d(idx, torch.int64), C if c["idx"] else -1, B, G, k, C, groups, R.EPS, R.SLOPE)
    (out * _d(dout)).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), yg.grad, gm.grad, bt.grad


def _check_backward(K, c, inputs, tag, lds=True):
    B, G, k, C, groups = _geom(c)
    yz, idx, gamma, beta, dout = inputs
    zoff = C if c["idx"] else -1
    assert R.backward_path(G, k, c["idx"]) == c["path"] and (lds or R.backward_path(G, k, c["idx"], lds=False) == "gl4")
    ref = R.edge_tail(yz, zoff, idx, B, G, k, C, groups, gamma, beta)[0]
    dyz, dg, db = R.edge_tail_bwd(yz, zoff, idx, B, G, k, C, groups, gamma, beta, dout)
    got = _backward(K, c, *inputs)
    again = _backward(K, c, *inputs)
    e = _err(_n(got[0]), ref), _err(_n(got[1]), dyz), _err(_n(got[2]), dg), _err(_n(got[3]), db)
    same = all(torch.equal(a, b) for a, b in zip(got, again))
    print(f"[dgcnn bwd] {tag} {_id(c)}: out {e[0]:.2e} (bar {FWD:.0e})  dyz {e[1]:.2e}  dgamma {e[2]:.2e}  dbeta {e[3]:.2e} (bar {BWD:.0e})"
          f"  two runs bit-identical: {same}")
    assert e[0] <= FWD and max(e[1:]) <= BWD and same
    return got


@pytest.mark.parametrize("c", BACKWARD, ids=_id)
def test_backward_on_every_dispatch_path(K, c):
    inputs = R.backward_inputs(c)
    got = _check_backward(K, c, inputs, "real")
    if c["graph"] == "hub":
        lone = R.unnamed_rows(inputs[1], c["G"])
        assert lone[0].sum() >= 3 and (inputs[1][0] == 3).sum() == (c["k"] - 1) * c["G"] + 1
        dY = got[1][:, :c["C"]].reshape(c["B"], c["G"], c["C"])
        assert (dY[torch.from_numpy(lone).cuda()] == 0).all(), "a row that no edge names received a gradient"


def test_backward_refuses_more_than_512_rows(K):
    c = REFUSED
    B, G, k, C, groups = _geom(c)
    assert R.backward_path(G, k, True) == "refused"
    yz, idx, gamma, beta, dout = R.backward_inputs(c)
    yg = _d(yz).requires_grad_(True); gm = _d(gamma).requires_grad_(True); bt = _d(beta).requires_grad_(True)
    out = K.EdgeGnLreluMaxFn.apply(yg, gm, bt, _d(idx, torch.int64), C, B, G, k, C, groups, R.EPS, R.SLOPE)
    with pytest.raises(Exception, match="act_edge_gn_lrelu_max_bwd_f32") as info:
        (out * _d(dout)).sum().backward()
    torch.cuda.synchronize()
    print(f"[dgcnn bwd] refused G = {G}: {info.value}")
    assert yg.grad is None and gm.grad is None and bt.grad is None


@pytest.mark.parametrize("c", TIES, ids=_id)
def test_backward_ties_between_different_sources(K, c):
    """Y on the 1/8 lattice: equal neighbour values at different rows are common, and the first extremum has to win in every form"""
    B, G, k, C, groups = _geom(c)
    inputs = R.tie_inputs(c)
    yz, idx = inputs[0], inputs[1]
    v = yz[:, :C].reshape(B, G, C)[np.arange(B)[:, None, None], idx]                             # [B, k, G, C]
    s = np.sort(v, axis=1)
    tied = ((s[:, -1] == s[:, -2]) | (s[:, 0] == s[:, 1])).mean()
    print(f"[dgcnn ties] {_id(c)}: {tied:.1%} of the (g, c) have a tied extremum")
    assert tied > 0.05
    if c["G"] > 128:
        _check_backward(K, c, inputs, "ties")
        return
    prev = K.lib.act_edge_bwd_lds(-1)
    res = []
    try:
        for on in (0, 1):
            K.lib.act_edge_bwd_lds(on)
            res.append(_check_backward(K, c, inputs, f"ties lds={on}", lds=bool(on)))
    finally:
        K.lib.act_edge_bwd_lds(prev)
    z = _err(_n(res[1][1][:, C:]), _n(res[0][1][:, C:])), _err(_n(res[1][1][:, :C]), _n(res[0][1][:, :C]))
    print(f"[dgcnn ties] {_id(c)}: LDS form against the scatter-image form: dZ {z[0]:.2e}  dY {z[1]:.2e} (bar 2e-6: one moved selection is a whole term)"
          f"  bit-identical: {torch.equal(res[0][1], res[1][1])}")
    assert max(z) <= 2e-6


# ---------------------------------------------------------------------------------------------------------------- tokenizer
@pytest.mark.parametrize("C", [4, 252, 1028, 16384])
def test_soft_gumbel_softmax_at_the_stride_and_size_bounds(K, C):
    """one float4, one past a 1,024-wide trip, the refusal bound"""
    rows, tau = 6, 0.7
    rng = np.random.default_rng(C)
    logits = (2 * rng.standard_normal((rows, C))).astype(np.float32); dy = rng.standard_normal((rows, C)).astype(np.float32)
    noise = (-np.log(rng.exponential(size=(rows, C)))).astype(np.float32)
    yr = R.gumbel_softmax(logits, noise, tau)
    lg = _d(logits).requires_grad_(True)
    y = K.gumbel_softmax(lg, tau, noise=_d(noise))
    (y * _d(dy)).sum().backward()
    e = _err(_n(y), yr), _err(_n(lg.grad), R.gumbel_softmax_bwd(yr, dy, tau))
    print(f"[soft gumbel] C={C}: y {e[0]:.2e} (bar {FWD:.0e})  dlogits {e[1]:.2e} (bar {BWD:.0e})")
    assert e[0] <= FWD and e[1] <= BWD


def test_soft_gumbel_softmax_wide_range_and_refusals(K):
    C = 1028
    rng = np.random.default_rng(5)
    logits = rng.uniform(-80, 80, size=(4, C)).astype(np.float32)
    logits[:, 0] = -80; logits[:, C - 1] = 80; logits[1, 7] = 80                              # row 1: two equal maxima
    y = _n(K.gumbel_softmax(_d(logits), 1.0, noise=_d(np.zeros((4, C), np.float32))))
    e = _err(y, R.gumbel_softmax(logits, np.zeros((4, C)), 1.0))
    print(f"[soft gumbel] (logits + g) / tau over +-80: row sums - 1 = {np.abs(y.sum(-1) - 1).max():.2e}, y {e:.2e}")
    assert np.isfinite(y).all() and np.abs(y.sum(-1) - 1).max() <= 1e-4 and e <= FWD
    for bad in (16388, 6):
        with pytest.raises(Exception, match="act_gumbel_softmax_fwd_f32"):
            K.gumbel_softmax(torch.zeros(2, bad, device="cuda"), 1.0, noise=torch.zeros(2, bad, device="cuda"))


@pytest.mark.parametrize("B,G,C", [(2, 1, 1), (2, 5, 1), (2, 5, 255), (17, 1, 255), (2, 1, 257), (15, 5, 257), (16, 5, 257), (2, 5, 4100), (1, 1, 4100)])
def test_kl_to_uniform_around_the_unrolled_loop(K, B, G, C):
    """kl_uniform_kernel walks B C values four at a time across 1,024 threads: B C below 4,096 (tail loop only), just past it, and two trips"""
    rng = np.random.default_rng(B * 100 + C)
    logits = (2 * rng.standard_normal((B, G, C))).astype(np.float32)
    ref, dref = R.kl_uniform(logits), R.kl_uniform_bwd(logits, 1.7)
    lg = _d(logits).requires_grad_(True)
    kl = K.kl_to_uniform(lg)
    (kl * 1.7).backward()
    e = abs(kl.item() - ref) / max(1.0, abs(ref)), _err(_n(lg.grad), dref)
    print(f"[kl uniform] B={B} G={G} C={C} (B C = {B * C}): kl {e[0]:.2e} (bar {FWD:.0e})  dlogits {e[1]:.2e} (bar {BWD:.0e})")
    assert e[0] <= FWD and e[1] <= BWD


@pytest.mark.parametrize("C,c1,c2", [(8192, 800, 1064), (24, 5, 17)], ids=["float4-branch", "elementwise-branch"])
def test_gumbel_argmax_ties_and_planted_maxima(K, C, c1, c2):
    """equal scores: the lowest index wins, inside a thread, across the lanes of a wave and across waves (C = 8192: c1 = 800 belongs to thread 200 in
    wave 3, c2 = 1064 to thread 10 in wave 0, second trip); C = 24 with four groups is cpg = 6, the element-wise branch"""
    B, G, groups = 2, 3, 4
    rng = np.random.default_rng(C)
    gamma = rng.standard_normal(C).astype(np.float32); beta = np.full(C, 0.1, np.float32)
    cb = rng.standard_normal((C, 5)).astype(np.float32)
    h = np.full((B * G, C), 0.75, np.float32)                                                  # equal activations: every logit is lrelu(beta)
    zero = np.zeros((B * G, C), np.float32)
    for what, noise, want in (("all equal", zero, 0), ("maximum at C - 1", None, C - 1), ("two equal maxima", None, c1)):
        if noise is None:
            noise = zero.copy()
            noise[:, [C - 1] if want == C - 1 else [c1, c2]] = 5.0
        codes, index, logits, _, _ = _tokenizer(K, B, G, C, groups, h, gamma, beta, noise, 1.0, cb)
        print(f"[gumbel argmax] C={C} {what}: index {sorted(set(index.tolist()))}, expected {want}")
        assert (index == want).all() and np.array_equal(codes, np.tile(cb[want].astype(np.float64), (B * G, 1)))
        assert _err(logits, np.full((B * G, C), 0.1)) <= FWD


# ---------------------------------------------------------------------------------------------------------- argument checks
def _arg_checks(fn, valid, checks):
    """valid: the argument list of a call that succeeds; checks: (position, value, expected return code)"""
    assert fn(*valid) == 0
    torch.cuda.synchronize()
    for pos, value, want in checks:
        args = list(valid)
        args[pos] = value
        got = fn(*args)
        assert got == want, (fn.__name__, pos, value, got, want)
    torch.cuda.synchronize()
    return len(checks)


def test_argument_checks(K):
    B, G, k, C, groups, D = 2, 8, 2, 16, 4, 3
    f = lambda *s: torch.ones(*s, device="cuda")
    yz, gamma, beta, stats, out, dout, dyz = f(B * G, 2 * C), f(C), f(C), f(18 * B * groups), f(B * G, C), f(B * G, C), f(B * G, 2 * C)
    part, mstat, h, cb, logits, y = f(2, B, C), f(2 * B * groups), f(B * G, C), f(C, D), f(B * G, C), f(B * G, C)
    idx = torch.zeros(B, k, G, dtype=torch.int64, device="cuda"); index = torch.zeros(B * G, dtype=torch.int64, device="cuda")
    codes, lse, qbar, one = f(B * G, D), f(B * G), f(B, C), f(1)
    p, st = (lambda t: t.data_ptr()), _st()
    bad_dims = lambda pos: [(q, v, ACT_E_BADARG) for q in pos for v in (0, -1)]
    null = lambda pos: [(q, None, ACT_E_NULLPTR) for q in pos]
    n = 0
    # yz ldy zoff idx B G k C groups gamma beta eps slope stats out ldo ooff stream
    n += _arg_checks(K.lib.act_edge_gn_lrelu_max_f32, [p(yz), 2 * C, C, p(idx), B, G, k, C, groups, p(gamma), p(beta), 1e-5, 0.2, p(stats), p(out), C, 0, st],
                     null([0, 9, 10, 13, 14]) + bad_dims([4, 5, 6, 7, 8]) + [(8, 3, ACT_E_BADARG)])
    # yz ldy zoff idx B G k C groups gamma beta stats slope dout ldd dyz part mstat stream
    valid = [p(yz), 2 * C, C, p(idx), B, G, k, C, groups, p(gamma), p(beta), p(stats), 0.2, p(dout), C, p(dyz), p(part), p(mstat), st]
    n += _arg_checks(K.lib.act_edge_gn_lrelu_max_bwd_f32, valid, null([0, 9, 10, 11, 13, 15, 16, 17]) + bad_dims([4, 5, 6, 7, 8]) + [(8, 3, ACT_E_BADARG)])
    head = list(valid); head[2] = -1; head[3] = None; head[6] = 1; head[1] = C
    n += _arg_checks(K.lib.act_edge_gn_lrelu_max_bwd_f32, [p(h)] + head[1:], [(6, 2, ACT_E_BADARG), (2, 0, ACT_E_BADARG)])     # no graph: k = 1 and no Z only
    # h B G C groups gamma beta eps slope noise seed seed_dev tau codebook D stats index out logits stream
    n += _arg_checks(K.lib.act_gn_gumbel_argmax_gather_f32,
                     [p(h), B, G, C, groups, p(gamma), p(beta), 1e-5, 0.2, p(logits), 0, None, 1.0, p(cb), D, p(stats), p(index), p(codes), p(y), st],
                     null([0, 5, 6, 13, 15, 17]) + bad_dims([1, 2, 3, 4, 14]) + [(4, 3, ACT_E_BADARG), (12, 0.0, ACT_E_BADARG), (12, -1.0, ACT_E_BADARG)])
    n += _arg_checks(K.lib.act_gn_gumbel_argmax_gather_f32,                                      # C % 4 != 0 (18 columns, groups = 3)
                     [p(h), B, G, 12, 3, p(gamma), p(beta), 1e-5, 0.2, None, 0, None, 1.0, p(cb), D, p(stats), None, p(codes), None, st],
                     [(3, 18, ACT_E_BADARG)])
    # logits R C noise seed tau y stream
    n += _arg_checks(K.lib.act_gumbel_softmax_fwd_f32, [p(logits), B * G, C, None, 0, 1.0, p(y), st],
                     null([0, 6]) + bad_dims([1, 2]) + [(2, 6, ACT_E_BADARG), (2, 16388, ACT_E_BADARG), (5, 0.0, ACT_E_BADARG)])
    # y dy R C tau dlogits stream
    n += _arg_checks(K.lib.act_gumbel_softmax_bwd_f32, [p(y), p(dout), B * G, C, 1.0, p(out), st], null([0, 1, 5]) + bad_dims([2, 3]) + [(4, 0.0, ACT_E_BADARG)])
    # logits B G C lse qbar klv stream
    n += _arg_checks(K.lib.act_kl_uniform_fwd_f32, [p(logits), B, G, C, p(lse), p(qbar), p(one), st], null([0, 4, 5, 6]) + bad_dims([1, 2, 3]))
    # logits lse qbar grad B G C dlogits stream
    n += _arg_checks(K.lib.act_kl_uniform_bwd_f32, [p(logits), p(lse), p(qbar), p(one), B, G, C, p(out), st], null([0, 1, 2, 3, 7]) + bad_dims([4, 5, 6]))
    too_many = torch.zeros(1, k, 513, dtype=torch.int64, device="cuda")
    yz5, dout5, dyz5 = f(513, 2 * C), f(513, C), f(513, 2 * C)
    big = [p(yz5), 2 * C, C, p(too_many), 1, 513, k, C, groups, p(gamma), p(beta), p(stats), 0.2, p(dout5), C, p(dyz5), p(part), p(mstat), st]
    assert K.lib.act_edge_gn_lrelu_max_bwd_f32(*big) == ACT_E_BADARG
    torch.cuda.synchronize()
    print(f"[dgcnn args] {n + 1} refused calls, each with the documented code")
