"""GPU: the kernels of the Transformer segmentation head (csrc/seg.hip and the three-NN feature propagation of csrc/sa.hip) at the sizes where
their index arithmetic changes (ragged tiles, one past a block or a chunk, grid-stride loops, the limits of G and C) and on ignored labels.
Every comparison is bit-exact (three-NN against its float32 restatement, integer-valued data whose float32 partial sums are exact, counts)
or against a rounding bound computed in float64 from the inputs (tests/seg_ref.py); the one
exception is interp_conv, which goes through the GEMM and reuses the project's relative bar.  Each test prints its largest error / bound ratio
(pytest -s) so that the tightness of the bounds stays visible."""
import functools

import numpy as np
import pytest
import torch

from tests import seg_ref as SR
from tests.test_gpu_dense import TOL, _rel

pytestmark = pytest.mark.gpu

U = SR.U


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _d(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _ratio(name, err, bound):
    """largest err / bound over the elements with a non-zero bound (err must be 0 where the bound is 0)"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.all(err[bound == 0] == 0), name
    nz = bound > 0
    r = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    print("[seg_edges] %s: max err/bound = %.3f" % (name, r))
    return r


# ---- three-NN and adjacency ----------------------------------------------------------------------------------------------------------------
def _cloud(B, N, G, seed):
    rs = np.random.RandomState(seed)
    xyz = rs.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    if N < G:
        return xyz, rs.uniform(-1, 1, size=(B, G, 3)).astype(np.float32)
    return xyz, np.stack([xyz[b, rs.choice(N, G, replace=False)] for b in range(B)])        # centres are cloud points (as FPS picks them)


def _check_three_nn(dev, xyz, ctr):
    from act_amd import kernels as K
    G = ctr.shape[1]
    ref = SR.three_nn_f32(xyz, ctr)
    got = [t.cpu().numpy() for t in K.three_nn(_d(xyz, dev), _d(ctr, dev))]
    for name, g, r in zip(("idx", "w", "off", "ent"), got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape, name
        assert np.array_equal(_bits(g), _bits(r)), (name, int((_bits(g) != _bits(r)).sum()))
    idx2, w2, off2, ent2 = K.three_nn(_d(xyz, dev), _d(ctr, dev), want_adj=False)
    assert off2 is None and ent2 is None
    assert np.array_equal(idx2.cpu().numpy(), ref[0]) and np.array_equal(_bits(w2.cpu().numpy()), _bits(ref[1]))
    assert got[2][:, 0].tolist() == [0] * xyz.shape[0] and got[2][:, G].tolist() == [3 * xyz.shape[1]] * xyz.shape[0]
    return ref


NN_CASES = [(1, 1, 3), (2, 255, 3), (3, 257, 5), (2, 1000, 127), (1, 683, 512), (2, 700, 511), (1, 683, 256), (2, 300, 257)]


@pytest.mark.parametrize("B,N,G", NN_CASES)
def test_three_nn_bit_exact_on_all_rows(dev, B, N, G):
    """idx, w, off and ent equal the float32 restatement on every row (not only off near-ties); E = 3N = 2049 is one entry past a chunk of the
    one-launch adjacency kernel at N = 683 and G = 256, its largest G (257 and above go to the three-launch builder); G = 3 / 511 / 512 were the
    limits of the centre loop and of the scan of the former kernel"""
    xyz, ctr = _cloud(B, N, G, 1000 + N + G)
    _check_three_nn(dev, xyz, ctr)


@pytest.mark.parametrize("B,N,G,seed", SR.NEAR_TIE_CASES)
def test_three_nn_bit_exact_on_near_tie_clouds(dev, B, N, G, seed):
    """lattice clouds: equal and last-bit-different distances, where the float32 expression and the index decide the order"""
    xyz, ctr = SR.near_tie_clouds(B, N, G, seed)
    assert SR.rows_with_ties(xyz, ctr).any()
    _check_three_nn(dev, xyz, ctr)


@pytest.mark.parametrize("B,N,G", [(2, 257, 5), (1, 683, 40), (2, 300, 512)])
def test_three_nn_bit_exact_on_a_coarse_lattice(dev, B, N, G):
    """integer coordinates in [-3, 3]: a third of the rows at G = 5 and nearly all at G >= 40 have exact ties among their four nearest, many
    of them with duplicated centres"""
    rs = np.random.RandomState(N + G)
    xyz = rs.randint(-3, 4, size=(B, N, 3)).astype(np.float32)
    ctr = rs.randint(-3, 4, size=(B, G, 3)).astype(np.float32)
    assert SR.rows_with_ties(xyz, ctr).mean() > (0.25 if G == 5 else 0.75)
    _check_three_nn(dev, xyz, ctr)


@pytest.mark.parametrize("G", [3, 64, 512])
def test_three_nn_degenerate_adjacency(dev, G):
    """every point within 0.01 of centres 0, 1, 2, the other centres far away: lists 0..2 hold N entries each, every other list is empty"""
    B, N = 2, 700
    rs = np.random.RandomState(G)
    ctr = np.zeros((B, G, 3), np.float32)
    ctr[:, 1, 0] = 0.004
    ctr[:, 2, 1] = 0.004
    ctr[:, 3:] = 100.0 + rs.uniform(0, 1, size=(B, G - 3, 3)).astype(np.float32)
    xyz = rs.uniform(-0.002, 0.002, size=(B, N, 3)).astype(np.float32)
    idx, w, off, ent, _ = _check_three_nn(dev, xyz, ctr)
    assert np.array_equal(np.sort(idx, axis=-1), np.broadcast_to(np.arange(3, dtype=np.int32), (B, N, 3)))
    want_off = np.minimum(np.arange(G + 1), 3) * N
    assert np.array_equal(off, np.broadcast_to(want_off.astype(np.int32), (B, G + 1)))


@pytest.mark.parametrize("G", [1, 2, 513])
def test_three_nn_outside_the_former_3_512_limit(dev, G):
    """G < 3: the slots that never fill carry idx 0 and weight exactly 0, the others are normalised over what exists; G = 513 is one past the
    former limit.  Bit for bit, as at every other size"""
    xyz, ctr = _cloud(2, 300, G, 2000 + G)
    idx, w, _, _, d = _check_three_nn(dev, xyz, ctr)
    if G < 3:
        assert (idx[..., G:] == 0).all() and np.isinf(d[..., G:]).all() and (w[..., G:] == 0).all()
    if G == 1:
        assert (w[..., 0] == 1).all()


# ---- row interpolation: index coverage in exact arithmetic -----------------------------------------------------------------------------------
# weights in quarters, |P|, |dY| <= 8: every term is a multiple of 1/4 and every partial sum of a list of up to 262148 entries (a point names a
# centre at most once) stays below 2^24 quarters, so each float32 operation is exact and the result does not depend on the order of the sum
_TRIPLES = np.array([(0.5, 0.25, 0.25), (0.25, 0.5, 0.25), (0.25, 0.25, 0.5), (0.5, 0.5, 0.0), (0.75, 0.25, 0.0), (1.0, 0.0, 0.0),
                     (0.0, 0.25, 0.75)], np.float32)


@functools.lru_cache(maxsize=None)
def _exact_case(B, N, G, C):
    rs = np.random.RandomState(B + N + G + C)
    xyz, ctr = _cloud(B, N, G, 7 * N + G)
    idx, _, off, ent, _ = SR.three_nn_f32(xyz, ctr)
    w = _TRIPLES[rs.randint(0, len(_TRIPLES), size=(B, N))]
    P = rs.randint(-8, 9, size=(B * G, C)).astype(np.float32)
    dY = rs.randint(-8, 9, size=(B * N, C)).astype(np.float32)
    pts = (rs.randint(-8, 9, size=(B * N, 3)) / 4.0).astype(np.float32)
    wx = rs.randint(-8, 9, size=(C, 3)).astype(np.float32)
    bias = rs.randint(-8, 9, size=C).astype(np.float32)
    Y = SR.interp_fwd_f64(P, idx, w, B, N, G)[0]
    Y2 = SR.interp_fwd_f64(P, idx, w, B, N, G, xyz=pts, wxyz=wx, bias=bias)[0]
    dP = SR.interp_bwd_f64(dY, idx, w, B, N, G)[0]
    return dict(xyz=xyz, ctr=ctr, idx=idx, off=off, ent=ent, w=w, P=P, dY=dY, pts=pts, wx=wx, bias=bias, Y=Y, Y2=Y2, dP=dP)


INTERP_CASES = [(1, 1, 3, 4), (3, 5, 3, 4), (2, 257, 7, 260), (1, 1000, 512, 12), (1, 262148, 3, 4), (2, 5, 3, 1), (2, 37, 7, 3), (1, 257, 7, 130)]


@pytest.mark.parametrize("B,N,G,C", INTERP_CASES)
def test_interp_rows_exact(dev, B, N, G, C):
    """forward (with and without the xyz / bias epilogue) and backward equal float64 element for element: R = 15 is no multiple of the 4 rows of
    a block, C / 4 = 65 is one past a 64-lane block, G = 512 is a long centre table, and B * N = 262148 needs 65537
    row blocks; C = 1, 3 and 130 are no multiple of 4 (one float per lane; 130 is two past two 64-lane blocks)"""
    from act_amd import kernels as K
    c = _exact_case(B, N, G, C)
    idx, w, off, ent = _d(c["idx"], dev), _d(c["w"], dev), _d(c["off"], dev), _d(c["ent"], dev)
    Y = K.interp_rows_fwd(_d(c["P"], dev), idx, w, B, N, G)
    assert np.array_equal(Y.cpu().numpy().astype(np.float64), c["Y"])
    Y2 = K.interp_rows_fwd(_d(c["P"], dev), idx, w, B, N, G, xyz=_d(c["pts"], dev), wxyz=_d(c["wx"], dev), bias=_d(c["bias"], dev))
    assert np.array_equal(Y2.cpu().numpy().astype(np.float64), c["Y2"])
    dP = K.interp_rows_bwd(_d(c["dY"], dev), off, ent, w, B, N, G)
    assert np.array_equal(dP.cpu().numpy().astype(np.float64), c["dP"])


def test_three_nn_at_65537_row_blocks(dev):
    """the cloud of the largest interpolation case through three_nn itself: E = 786444 = 384 chunks + 12 entries"""
    c = _exact_case(1, 262148, 3, 4)
    _check_three_nn(dev, c["xyz"], c["ctr"])


# ---- row interpolation: rounding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,G,C", [(2, 257, 7, 260), (2, 1024, 128, 1536)])
def test_interp_rows_rounding_bounds(dev, B, N, G, C):
    """real-valued data.  forward: 8 U (sum_k |w_k P_k| + sum_j |xyz_j wxyz_cj| + |bias_c|), a chain of three + three FMAs and two additions;
    backward: (L + 2) U sum_e |w_e dY_e| with L the length of the centre's list.  Componentwise, from the inputs, not tuned."""
    from act_amd import kernels as K
    rs = np.random.RandomState(C)
    xyz, ctr = _cloud(B, N, G, C + 1)
    idx, w, off, ent, _ = SR.three_nn_f32(xyz, ctr)
    P = rs.standard_normal((B * G, C)).astype(np.float32)
    dY = rs.standard_normal((B * N, C)).astype(np.float32)
    wx = rs.standard_normal((C, 3)).astype(np.float32)
    bias = rs.standard_normal(C).astype(np.float32)
    di, dw = _d(idx, dev), _d(w, dev)
    Y, A = SR.interp_fwd_f64(P, idx, w, B, N, G)
    got = K.interp_rows_fwd(_d(P, dev), di, dw, B, N, G).cpu().numpy().astype(np.float64)
    assert _ratio("interp_fwd %s" % ((B, N, G, C),), np.abs(got - Y), 8 * U * A) <= 1
    Y2, A2 = SR.interp_fwd_f64(P, idx, w, B, N, G, xyz=xyz.reshape(-1, 3), wxyz=wx, bias=bias)
    got = K.interp_rows_fwd(_d(P, dev), di, dw, B, N, G, xyz=_d(xyz.reshape(-1, 3), dev), wxyz=_d(wx, dev), bias=_d(bias, dev))
    assert _ratio("interp_fwd+xyz+bias %s" % ((B, N, G, C),), np.abs(got.cpu().numpy().astype(np.float64) - Y2), 8 * U * A2) <= 1
    dP, Ab, L = SR.interp_bwd_f64(dY, idx, w, B, N, G)
    got = K.interp_rows_bwd(_d(dY, dev), _d(off, dev), _d(ent, dev), dw, B, N, G).cpu().numpy().astype(np.float64)
    assert _ratio("interp_bwd %s" % ((B, N, G, C),), np.abs(got - dP), (L[:, None] + 2) * U * Ab) <= 1


def _check_interp_conv(dev, B, N, G, C, Kf, want_adj):
    from act_amd import kernels as K
    rs = np.random.RandomState(Kf)
    xyz, ctr = _cloud(B, N, G, Kf + 1)
    idx, w, _, _, _ = SR.three_nn_f32(xyz, ctr)
    x = torch.from_numpy(rs.standard_normal((B * G, Kf)).astype(np.float32))
    W = torch.from_numpy((rs.standard_normal((C, 3 + Kf)) / 8).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(C).astype(np.float32))
    dY = torch.from_numpy(rs.standard_normal((B * N, C)).astype(np.float32))
    pts = torch.from_numpy(xyz).reshape(B * N, 3)
    x64, W64, b64 = (t.double().requires_grad_(True) for t in (x, W, b))
    rows = torch.from_numpy(SR._rows(idx, B, N, G))
    feat = (x64[rows] * torch.from_numpy(w).double().reshape(B * N, 3, 1)).sum(1)
    ref = torch.cat((pts.double(), feat), dim=1) @ W64.t() + b64
    ref.backward(dY.double())
    nn3 = K.three_nn(_d(xyz, dev), _d(ctr, dev), want_adj=want_adj)
    assert (nn3[2] is None) == (not want_adj)
    assert np.array_equal(nn3[0].cpu().numpy(), idx) and np.array_equal(_bits(nn3[1].cpu().numpy()), _bits(w))
    xd, Wd, bd = (t.to(dev).requires_grad_(True) for t in (x, W, b))
    y = K.interp_conv(xd, Wd, bd, pts.to(dev), nn3, B, N, G)
    y.backward(dY.to(dev))
    assert _rel(y, ref) <= TOL
    assert _rel(xd.grad, x64.grad) <= TOL and _rel(Wd.grad, W64.grad) <= TOL and _rel(bd.grad, b64.grad) <= TOL


def test_interp_conv_forward_backward(dev):
    """the per-group form (GEMM once per centre, then interpolation + xyz columns + bias in one kernel) against the plain form
    W . cat(xyz, sum_k w_k x[idx_k]) + b in float64 autograd, at a ragged shape"""
    _check_interp_conv(dev, 2, 257, 7, 260, 64, True)


def test_interp_conv_builds_the_adjacency_its_search_left_out(dev):
    """nn3 from a search without the adjacency (want_adj=False): the backward builds it.  G = 2 leaves every third slot at weight 0, and C = 6 /
    Kf = 5 are no multiples of 4"""
    _check_interp_conv(dev, 2, 37, 2, 6, 5, False)


def test_interp_rows_skip_a_slot_of_weight_zero(dev):
    """the third slot of every point has weight exactly 0 (a search over two centres) and is aimed at a row of inf in P: it is neither read nor
    added, so the forward with the xyz / bias epilogue stays finite and equals the unpoisoned result bit for bit, and the backward leaves that
    row's gradient 0"""
    from act_amd import kernels as K
    B, N, G, C = 2, 37, 3, 6
    rs = np.random.RandomState(37)
    xyz, ctr = _cloud(B, N, 2, 38)
    idx, w, _, _, _ = SR.three_nn_f32(xyz, ctr)
    assert (w[..., 2] == 0).all() and (idx[..., 2] == 0).all() and (w[..., :2] > 0).all()
    P = rs.standard_normal((B * G, C)).astype(np.float32)
    wx, bias = rs.standard_normal((C, 3)).astype(np.float32), rs.standard_normal(C).astype(np.float32)
    dY = rs.standard_normal((B * N, C)).astype(np.float32)
    epi = dict(xyz=_d(xyz, dev), wxyz=_d(wx, dev), bias=_d(bias, dev))
    base = K.interp_rows_fwd(_d(P, dev), _d(idx, dev), _d(w, dev), B, N, G, **epi)
    poisoned = P.copy()
    poisoned.reshape(B, G, C)[:, 2] = np.inf
    aimed = idx.copy()
    aimed[..., 2] = 2
    Y = K.interp_rows_fwd(_d(poisoned, dev), _d(aimed, dev), _d(w, dev), B, N, G, **epi)
    assert torch.isfinite(Y).all() and np.array_equal(_bits(Y.cpu().numpy()), _bits(base.cpu().numpy()))
    want, A = SR.interp_fwd_f64(P, idx, w, B, N, G, xyz=xyz.reshape(-1, 3), wxyz=wx, bias=bias)
    assert _ratio("interp_fwd skipped slot", np.abs(Y.cpu().numpy().astype(np.float64) - want), 8 * U * A) <= 1
    off, ent = SR.adjacency(aimed, G)
    dP = K.interp_rows_bwd(_d(dY, dev), _d(off, dev), _d(ent, dev), _d(w, dev), B, N, G).cpu().numpy()
    assert np.isfinite(dP).all() and (dP.reshape(B, G, C)[:, 2] == 0).all() and (dP.reshape(B, G, C)[:, :2] != 0).any()
    off2, ent2 = K.three_adjacency(_d(aimed, dev), G)
    assert np.array_equal(off2.cpu().numpy(), off) and np.array_equal(ent2.cpu().numpy(), ent)


# ---- xyz / bias gradient -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C", [(1, 1), (511, 3), (513, 257), (1025, 260)])
def test_interp_xyz_grad_exact(dev, R, C):
    """integers |v| <= 8: products <= 64, sums <= 64 * 1025, every float32 partial sum exact.  R = 513 / 1025 leave a one-row last block of
    rows, C = 257 / 260 a ragged last block of columns.  want_w only and want_b only write nothing else and the same values."""
    from act_amd import kernels as K
    rs = np.random.RandomState(R + C)
    dY = rs.randint(-8, 9, size=(R, C)).astype(np.float32)
    xyz = rs.randint(-8, 9, size=(R, 3)).astype(np.float32)
    dw, db, _, _ = SR.xyz_grad_f64(dY, xyz)
    gw, gb = K.interp_xyz_grad(_d(dY, dev), _d(xyz, dev))
    assert gw.shape == (C, 3) and gb.shape == (C,)
    assert np.array_equal(gw.cpu().numpy().astype(np.float64), dw) and np.array_equal(gb.cpu().numpy().astype(np.float64), db)
    gw2, none = K.interp_xyz_grad(_d(dY, dev), _d(xyz, dev), want_b=False)
    assert none is None and torch.equal(gw2, gw)
    none, gb2 = K.interp_xyz_grad(_d(dY, dev), _d(xyz, dev), want_w=False)
    assert none is None and torch.equal(gb2, gb)


# ---- log-softmax -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SR.KINDS)
@pytest.mark.parametrize("C", [1, 2, 13, 50, 64])
def test_log_softmax_bounds(dev, C, kind):
    """forward within U (|out| + |lse| + C + 16) of float64, -inf exactly where the input is -inf, exactly 0 at C = 1; backward within
    U (|g_c| + (C + 4) p_c sum|g|) of g - exp(logp) sum g evaluated in float64 on the float32 log-probabilities the backward kernel reads
    (tests/test_seg_ref_host.py holds torch's float32 CPU kernels to the same two bounds)"""
    from act_amd import kernels as K
    worst_f = worst_b = 0.0
    for R in (1, 255, 257):
        z = SR.softmax_inputs(kind, R, C, 100 * C + R)
        g = np.random.RandomState(C + R).standard_normal((R, C)).astype(np.float32)
        out, lse = SR.log_softmax_f64(z)
        zd = _d(z, dev).requires_grad_(True)
        lp = K.log_softmax(zd)
        lp.backward(_d(g, dev))
        got = lp.detach().cpu().numpy()
        fin = ~np.isneginf(z)
        assert np.all(np.isneginf(got[~fin])) and np.all(np.isfinite(got[fin]))
        if C == 1:
            assert np.all(got == 0)
        err = np.abs(got.astype(np.float64) - np.where(fin, out, 0.0))[fin]
        worst_f = max(worst_f, _ratio("log_softmax_fwd C=%d R=%d %s" % (C, R, kind), err, SR.log_softmax_fwd_bound(out, lse, C)[fin]))
        dz, p, sabs = SR.log_softmax_bwd_f64(got, g)
        gz = zd.grad.cpu().numpy()
        assert np.all(np.isfinite(gz))
        worst_b = max(worst_b, _ratio("log_softmax_bwd C=%d R=%d %s" % (C, R, kind), np.abs(gz.astype(np.float64) - dz),
                                      SR.log_softmax_bwd_bound(g, p, sabs, C)))
    assert worst_f <= 1 and worst_b <= 1


def test_log_softmax_rejects_more_than_64_classes(dev):
    from act_amd import kernels as K, _C
    with pytest.raises(_C.ActHipError):
        K.log_softmax(torch.zeros(4, 65, device=dev))


# ---- weighted-mean NLL -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _logp_base(C):
    """float32 [131073, C] log-probabilities (float64 log-softmax of 3 * randn, rounded once), shared by all row counts of one C; in one row
    of eight the maximum is planted a second time at another column, so that the arg-max has an exact tie"""
    rs = np.random.RandomState(C)
    R = 131073
    lp = SR.log_softmax_f64((3 * rs.standard_normal((R, C))).astype(np.float32))[0].astype(np.float32)
    if C > 1:
        r = np.arange(0, R, 8)
        col = rs.randint(0, C, size=r.size)
        lp[r, col] = lp[r].max(1)
    lp.setflags(write=False)
    return lp


def _nll_targets(R, C, mode, seed):
    rs = np.random.RandomState(seed)
    lp = _logp_base(C)[:R]
    if mode == "all_valid":
        t = rs.randint(0, C, size=R).astype(np.int64)
    elif mode == "one_valid":
        t = np.array([-100, -1, C, 255], np.int64)[rs.randint(0, 4, size=R)]
        t[R // 2] = C - 1
    else:
        t = SR.mixed_targets(rs, R, C)
    # on the rows with a planted tie, aim a third of the valid targets at the first and a third at the second maximum
    tie = np.where((lp == lp.max(1, keepdims=True)).sum(1) > 1)[0]
    for k, r in enumerate(tie):
        if 0 <= t[r] < C and mode != "one_valid" and k % 3:
            cols = np.where(lp[r] == lp[r].max())[0]
            t[r] = cols[0] if k % 3 == 1 else cols[1]
    return t


def _nll_raw(dev, lp, t, wt):
    """the C ABI directly: (loss, wsum, correct) -- the denominator is not part of the Python wrapper's result"""
    from act_amd import kernels as K
    R, C = lp.shape
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    wsum = torch.empty(1, dtype=torch.float32, device=dev)
    correct = torch.empty(1, dtype=torch.int64, device=dev)
    ws = K.workspace(dev, K.lib.act_nll_weighted_workspace(R))
    K.check(K.lib.act_nll_weighted_fwd_f32(K.ptr(lp), K.ptr(t), K.ptr(wt), R, C, K.ptr(loss), K.ptr(wsum), K.ptr(correct), K.ptr(ws),
                                           ws.numel() * 4, K.stream()), "act_nll_weighted_fwd_f32")
    return loss.cpu().numpy()[0], wsum.cpu().numpy()[0], int(correct.item())


def _check_nll(dev, R, C, weighted, mode):
    from act_amd import kernels as K
    lp = _logp_base(C)[:R]
    t = _nll_targets(R, C, mode, 3 * R + C)
    wt = (0.5 + np.random.RandomState(C).rand(C)).astype(np.float32) if weighted else None
    ref = SR.nll_f64(lp, t, wt, C)
    assert ref["valid"].any()
    lpd, td, wd = _d(lp, dev), _d(t, dev), (None if wt is None else _d(wt, dev))
    loss, wsum, correct = _nll_raw(dev, lpd, td, wd)
    assert correct == ref["correct"]                                      # first arg-max on ties, ignored rows never counted
    n = SR.nll_terms(R)
    tag = "R=%d C=%d w=%s %s" % (R, C, weighted, mode)
    _r = _ratio("nll den " + tag, abs(float(wsum) - ref["den"]), n * U * ref["Aden"])
    # numerator: loss = fl(num / den), so num = loss * den up to one more rounding of the quotient
    num = float(loss) * float(wsum)
    _r = max(_r, _ratio("nll num " + tag, abs(num - ref["num"]), n * U * ref["Anum"] + U * abs(num)))
    assert _r <= 1
    # the autograd wrapper: the same bits, twice; backward exactly zero on ignored rows, -g w_t / wsum to 2 ulp on the others
    g = np.float32(1.5)
    lpg = lpd.clone().requires_grad_(True)
    l1, c1 = K.nll_weighted(lpg, td, wd)
    (l1 * float(g)).backward()
    l2, c2 = K.nll_weighted(lpd, td, wd)
    assert _bits(l1.detach().cpu().numpy().reshape(1))[0] == _bits(np.array([loss]))[0] and torch.equal(l1.detach(), l2) and torch.equal(c1, c2)
    assert int(c1.item()) == ref["correct"]
    d = lpg.grad.cpu().numpy()
    want = SR.nll_bwd_f64(t, wt, wsum, g, R, C)
    assert np.all(d[~ref["valid"]] == 0) and np.count_nonzero(d) == int(ref["valid"].sum())
    assert np.all(np.abs(d.astype(np.float64) - want) <= 2 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) * (want != 0))
    lpg.grad = None
    l3, _ = K.nll_weighted(lpg, td, wd)
    (l3 * float(g)).backward()
    assert torch.equal(lpg.grad, _d(d, dev))


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("C", [1, 13, 50, 64])
@pytest.mark.parametrize("R", [1, 255, 257, 131072, 131073])
def test_nll_weighted_with_ignored_targets(dev, R, C, weighted):
    """about 30 % of the targets are one of {-100, -1, C, 255}.  Numerator and denominator each within n U sum|terms| of float64 over the valid
    rows, n = ceil(R / (nb 256)) + 8 + nb: R = 131072 fills the 512 blocks exactly once, 131073 sends one row round the stride loop."""
    if R == 1:
        lp = _logp_base(C)[:1]
        t = np.array([C - 1], np.int64)                                   # a single row must be a valid one: 0 / 0 otherwise
        ref = SR.nll_f64(lp, t, None, C)
        loss, wsum, correct = _nll_raw(dev, _d(lp, dev), _d(t, dev), None)
        assert wsum == 1 and correct == ref["correct"] and float(loss) == float(np.float32(ref["num"]))
    _check_nll(dev, R, C, weighted, "mixed" if R > 1 else "all_valid")


@pytest.mark.parametrize("mode", ["all_valid", "one_valid"])
@pytest.mark.parametrize("R,C", [(257, 13), (131073, 50)])
def test_nll_weighted_all_valid_and_all_but_one_ignored(dev, R, C, mode):
    _check_nll(dev, R, C, True, mode)
    _check_nll(dev, R, C, False, mode)


# ---- confusion matrix ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C", [(1, 1), (257, 13), (5000, 64), (262145, 2)])
def test_confusion_exact_with_ignored_targets(dev, R, C):
    """30 % ignored targets, many arg-max ties (values in 0..3), accumulation into a non-zero matrix; R = 262145 is one row past 1024 blocks"""
    from act_amd import kernels as K
    rs = np.random.RandomState(R + C)
    pred = rs.randint(0, 4, size=(R, C)).astype(np.float32)
    t = SR.mixed_targets(rs, R, C) if R > 1 else np.zeros(1, np.int64)
    ref = SR.confusion_ref(pred, t, C)
    cm = K.confusion(_d(pred, dev), _d(t, dev), C)
    assert cm.dtype == torch.int64 and np.array_equal(cm.cpu().numpy(), ref)
    start = rs.randint(0, 1000, size=(C, C)).astype(np.int64)
    out = _d(start, dev)
    assert K.confusion(_d(pred, dev), _d(t, dev), C, out=out) is out
    assert np.array_equal(out.cpu().numpy(), start + ref)
    if R > 1:                                                             # every row ignored: nothing is counted
        K.confusion(_d(pred, dev), _d(np.full(R, 255, np.int64), dev), C, out=out)
        assert np.array_equal(out.cpu().numpy(), start + ref)


# ---- wrappers: operands that are not contiguous float32 / int32 --------------------------------------------------------------------------------
def test_interp_wrappers_never_silently_misread_an_operand(dev):
    """a [:, :3] slice of an [R, 4] tensor and an int64 idx give the result of the contiguous / int32 operands (or raise); float64 raises"""
    from act_amd import kernels as K, _C
    B, N, G, C = 2, 257, 7, 260
    c = _exact_case(B, N, G, C)
    P, idx, w = _d(c["P"], dev), _d(c["idx"], dev), _d(c["w"], dev)
    pts, wx, bias, dY = _d(c["pts"], dev), _d(c["wx"], dev), _d(c["bias"], dev), _d(c["dY"], dev)
    want = K.interp_rows_fwd(P, idx, w, B, N, G, xyz=pts, wxyz=wx, bias=bias)
    assert np.array_equal(want.cpu().numpy().astype(np.float64), c["Y2"])
    pts4 = torch.cat((pts, torch.full((B * N, 1), 99.0, device=dev)), dim=1)[:, :3]
    wx4 = torch.cat((wx, torch.full((C, 1), 99.0, device=dev)), dim=1)[:, :3]
    w4 = torch.cat((w, torch.full((B, N, 1), 99.0, device=dev)), dim=2)[:, :, :3]
    idx4 = torch.cat((idx, torch.full((B, N, 1), 1, dtype=torch.int32, device=dev)), dim=2)[:, :, :3]
    assert not pts4.is_contiguous() and not wx4.is_contiguous() and not w4.is_contiguous() and not idx4.is_contiguous()
    variants = [dict(xyz=pts4), dict(wxyz=wx4), dict(w=w4), dict(idx=idx4), dict(idx=idx.long()), dict(idx=idx4.long()),
                dict(P=torch.cat((P, P), dim=1)[:, :C]), dict(bias=torch.stack((bias, bias), dim=1)[:, 0])]
    for v in variants:
        a = dict(P=P, idx=idx, w=w, xyz=pts, wxyz=wx, bias=bias)
        a.update(v)
        try:
            got = K.interp_rows_fwd(a["P"], a["idx"], a["w"], B, N, G, xyz=a["xyz"], wxyz=a["wxyz"], bias=a["bias"])
        except _C.ActHipError:
            continue
        assert torch.equal(got, want), sorted(v)
    for v in (dict(w=w.double()), dict(xyz=pts.double()), dict(wxyz=wx.double())):
        a = dict(P=P, idx=idx, w=w, xyz=pts, wxyz=wx, bias=bias)
        a.update(v)
        with pytest.raises(_C.ActHipError):
            K.interp_rows_fwd(a["P"], a["idx"], a["w"], B, N, G, xyz=a["xyz"], wxyz=a["wxyz"], bias=a["bias"])
    with pytest.raises(_C.ActHipError):                                   # an idx of another cloud size
        K.interp_rows_fwd(P, idx[:, :-1].contiguous(), w, B, N, G)
    # interp_xyz_grad
    gw, gb = K.interp_xyz_grad(dY, pts)
    dw, db, _, _ = SR.xyz_grad_f64(c["dY"], c["pts"])
    assert np.array_equal(gw.cpu().numpy().astype(np.float64), dw) and np.array_equal(gb.cpu().numpy().astype(np.float64), db)
    try:
        gw2, gb2 = K.interp_xyz_grad(dY, pts4)
        assert torch.equal(gw2, gw) and torch.equal(gb2, gb)
    except _C.ActHipError:
        pass
    with pytest.raises(_C.ActHipError):
        K.interp_xyz_grad(dY, pts.double())
    # interp_rows_bwd: int64 adjacency
    off, ent = _d(c["off"], dev), _d(c["ent"], dev)
    dP = K.interp_rows_bwd(dY, off, ent, w, B, N, G)
    assert np.array_equal(dP.cpu().numpy().astype(np.float64), c["dP"])
    try:
        assert torch.equal(K.interp_rows_bwd(dY, off.long(), ent.long(), w4, B, N, G), dP)
    except _C.ActHipError:
        pass
