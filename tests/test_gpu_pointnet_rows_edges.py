"""GPU: the row kernels of csrc/pointnet.hip (BatchNorm statistics / apply / backward, the SyncBatchNorm pieces, the tile and eval finalizers, the
group max / sum kernels) where tests/test_gpu_dense.py does not reach them: C % 4 != 0 (the scalar backward forms, which every SyncBatchNorm step
takes), a last column block of one float4 or of two columns, fewer stage-1 parts than part-lanes, a last part of 2 - 83 rows, a part boundary that
is no multiple of 16, the 1,024-part cap, three unrolled iterations plus a tail per row-lane, the second trip of every grid-stride loop,
relu = 0 in training, momentum = 1, running statistics left out, arg = NULL, accumulate = 1, n = 1, the argument checks -- and a first row that is
not a typical sample: on Gaussian data (test_batchnorm_statistics_do_not_depend_on_the_first_row), at the ragged shapes with far and near columns in
one workgroup (test_first_row_outlier_at_ragged_shapes), either side of the switch between the two forms (test_either_side_of_the_far_pivot_switch),
and the per-part (mean, M2) partials themselves at every shape (test_part_mean_and_m2_partials).

Sums are checked for EQUALITY on integer lattices (x in [-4, 4], dy in [-2, 2], mean an integer, rstd = 0.5, shift = k + 0.5): every partial sum is
a multiple of 1/2 below 2^24, so float32 adds them exactly in any order and the result is the int64 numpy sum, element for element.  On real values
the bars are those of tests/test_gpu_dense.py, unchanged: 2e-5 forward, 5e-5 backward, 1e-5 running statistics, relative to max(1, |ref|max).
The references are tests/pointnet_rows_ref.py (numpy float64 / int64, checked on the CPU by tests/test_pointnet_rows_host.py).  Every test prints
what it measured before it asserts."""
import functools

import numpy as np
import pytest
import torch

from tests import pointnet_rows_ref as P
from tests.golden.fill import fill_tensor
from tests.test_gpu_dense import _rel

pytestmark = pytest.mark.gpu

ACT_E_BADARG, ACT_E_NULLPTR = -1, -2
FWD, BWD, RUN = 2e-5, 5e-5, 1e-5                              # the bars of test_batchnorm_relu_fwd_bwd
GUARD = 64                                                   # sentinel floats behind a workspace / an output
_ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available()
    import act_amd.kernels as K
    return K


def _st():
    return torch.cuda.current_stream().cuda_stream


def _d(a, dtype=torch.float32):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.copy()).to(dtype).cuda()


def _n(t):
    return t.detach().cpu().numpy()


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _empty(*shape):
    return torch.full(shape, 7.0, device="cuda")


class _Workspace:
    """exactly act_colstats_workspace(R, C) bytes followed by sentinel floats that must survive the call"""

    def __init__(self, K, R, C):
        self.bytes = K.lib.act_colstats_workspace(R, C)
        assert self.bytes == 4 * P.workspace_floats(R, C)
        self.t = torch.full((self.bytes // 4 + GUARD,), 7.0, device="cuda")

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        assert (self.t[self.bytes // 4:] == 7.0).all(), "the kernel wrote past act_colstats_workspace"


def _params(C):
    return (1 + 0.2 * fill_tensor(f"pre.w{C}", (C,), "code")).numpy(), (0.1 * fill_tensor(f"pre.b{C}", (C,), "code")).numpy()


def _assert_exact(got, ref, what):
    """got (float32 from the device) == ref (int64 or float64) element for element; the message names the first element that differs"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere(~(got == ref))
    print(f"{what}: {len(bad)} of {ref.size} elements differ from the exact result")
    if len(bad):
        at = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{what}: {len(bad)} elements differ, the first at {at}: got {got[at]!r}, expected {ref[at]!r}")


def _bn_stats(K, x, R, C, gamma, beta, momentum, rm, rv):
    """-> mean, rstd, scale, shift of act_bn_stats_f32 (rm / rv updated in place, or None)"""
    out = [_empty(C) for _ in range(4)]
    ws = _Workspace(K, R, C)
    rc = K.lib.act_bn_stats_f32(x.data_ptr(), R, C, gamma.data_ptr(), beta.data_ptr(), P.BN_EPS, momentum, rm.data_ptr() if rm is not None else None,
                                rv.data_ptr() if rv is not None else None, *(o.data_ptr() for o in out), ws.ptr(), ws.bytes, _st())
    assert rc == 0
    ws.check()
    return out


def _col_mean_var(K, x, R, C):
    mean, var = _empty(C), _empty(C)
    ws = _Workspace(K, R, C)
    assert K.lib.act_col_mean_var_f32(x.data_ptr(), R, C, mean.data_ptr(), var.data_ptr(), ws.ptr(), ws.bytes, _st()) == 0
    ws.check()
    return mean, var


def _bn_bwd(K, x, dy, aff, relu, R, C, live=None, n=1):
    """act_bn_bwd_groups_f32 (act_bn_bwd_f32 when live is None and n == 1) -> dx, dgamma, dbeta"""
    dx, dg, db = _empty(R, C), _empty(C), _empty(C)
    ws = _Workspace(K, R, C)
    if live is None and n == 1:
        rc = K.lib.act_bn_bwd_f32(x.data_ptr(), dy.data_ptr(), *(a.data_ptr() for a in aff), relu, R, C, dx.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                  ws.ptr(), ws.bytes, _st())
    else:
        rc = K.lib.act_bn_bwd_groups_f32(x.data_ptr(), dy.data_ptr(), *(a.data_ptr() for a in aff), relu, R, C,
                                         live.data_ptr() if live is not None else None, n, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.ptr(),
                                         ws.bytes, _st())
    assert rc == 0
    ws.check()
    return dx, dg, db


def _bwd_sums(K, x, dy, aff, relu, R, C):
    s1, s2 = _empty(C), _empty(C)
    ws = _Workspace(K, R, C)
    assert K.lib.act_bn_bwd_sums_f32(x.data_ptr(), dy.data_ptr(), *(a.data_ptr() for a in aff), relu, R, C, s1.data_ptr(), s2.data_ptr(), ws.ptr(),
                                     ws.bytes, _st()) == 0
    ws.check()
    return s1, s2


def _bwd_apply(K, x, dy, aff, s1, s2, count, relu, R, C):
    dx = _empty(R, C)
    assert K.lib.act_bn_bwd_apply_f32(x.data_ptr(), dy.data_ptr(), *(a.data_ptr() for a in aff), s1.data_ptr(), s2.data_ptr(), float(count), relu, R, C,
                                      dx.data_ptr(), _st()) == 0
    return dx


@functools.lru_cache(maxsize=None)
def _lattice_dev(R, C):
    """the lattice on the device -> x, dy, (scale, shift, mean, rstd)"""
    x, dy, _, _ = P.lattice(R, C)
    return _d(x), _d(dy), tuple(_d(a) for a in P.lattice_affine(R, C))


# ---- 1. statistics -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C", P.SHAPES, ids=_ids(P.SHAPES))
def test_batchnorm_statistics_on_the_lattice(K, R, C):
    xl = P.lattice(R, C)[0]
    x = _lattice_dev(R, C)[0]
    gamma, beta = _params(C)
    g, b = _d(gamma), _d(beta)
    m_ref, v_ref = P.exact_mean_var(xl)
    amax = float(np.abs(xl).max())
    m_bound, v_bound = 4 * P.EPS32 * (2 * amax), 8 * P.EPS32 * (2 * amax) ** 2
    rstd_ref = 1.0 / np.sqrt(v_ref + P.BN_EPS)
    scale_ref = gamma.astype(np.float64) * rstd_ref
    shift_ref = beta.astype(np.float64) - m_ref * scale_ref
    r = np.random.default_rng(R)
    rm0, rv0 = r.standard_normal(C).astype(np.float32), (1 + r.random(C)).astype(np.float32)
    plain = _bn_stats(K, x, R, C, g, b, 0.1, None, None)
    mean, rstd, scale, shift = plain
    var_dev = 1.0 / _n(rstd).astype(np.float64) ** 2 - P.BN_EPS
    em, ev = np.abs(_n(mean) - m_ref).max(), np.abs(var_dev - v_ref).max()
    print(f"[{R}x{C}] parts x rows, last = {P.LAUNCH[(R, C)]}: |mean - exact| = {em:.2e} (bound {m_bound:.2e}), |var - exact| = {ev:.2e} (bound {v_bound:.2e})")
    errs = [_rel(scale, _t64(scale_ref)), _rel(shift, _t64(shift_ref))]
    print(f"[{R}x{C}] scale, shift rel err = {errs[0]:.2e}, {errs[1]:.2e}")
    assert em <= m_bound and ev <= v_bound
    assert max(errs) <= RUN
    for momentum in (0.1, 1.0):
        rm, rv = _d(rm0), _d(rv0)
        outs = _bn_stats(K, x, R, C, g, b, momentum, rm, rv)
        ref_rm, ref_rv = P.running((rm0, rv0), m_ref, v_ref, R, momentum)
        e = _rel(rm, _t64(ref_rm)), _rel(rv, _t64(ref_rv))
        print(f"[{R}x{C}] momentum {momentum}: running mean, var rel err = {e[0]:.2e}, {e[1]:.2e}")
        assert max(e) <= RUN
        for a, o in zip(plain, outs):                                                     # leaving the running statistics out changes no output bit
            assert torch.equal(_bits(a), _bits(o))
    cm, cv = _col_mean_var(K, x, R, C)
    ecv = np.abs(_n(cv).astype(np.float64) - v_ref).max()
    print(f"[{R}x{C}] act_col_mean_var_f32: |var - exact| = {ecv:.2e}")
    assert torch.equal(_bits(cm), _bits(mean)) and ecv <= v_bound


# ---- 2. apply ----------------------------------------------------------------------------------------------------------------------------------
def _ordered(a):
    """float32 -> int64 that increases with the value, +0.0 and -0.0 both 0: differences count ulps"""
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("R,C", P.VEC_SHAPES, ids=_ids(P.VEC_SHAPES))
def test_affine_act_is_the_rounded_float64_map(K, R, C, relu):
    x = fill_tensor(f"pre.ax{R}", (R, C), "code").numpy()
    scale, shift = (1 + 0.2 * fill_tensor(f"pre.as{C}", (C,), "code")).numpy(), fill_tensor(f"pre.ah{C}", (C,), "code").numpy()
    y = _empty(R, C)
    assert K.lib.act_affine_act_f32(_d(x).data_ptr(), _d(scale).data_ptr(), _d(shift).data_ptr(), relu, R, C, y.data_ptr(), _st()) == 0
    ref = P.affine_act(x, scale, shift, relu).astype(np.float32)
    ulps = np.abs(_ordered(_n(y)) - _ordered(ref))
    print(f"[{R}x{C} relu={relu}] max ulp distance to fl32(x scale + shift) = {ulps.max()} over {ulps.size} elements ({(ulps > 0).sum()} differ)")
    assert ulps.max() <= 2


# ---- 3. backward -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("R,C", P.SHAPES, ids=_ids(P.SHAPES))
def test_batchnorm_backward_on_the_lattice(K, R, C, relu):
    x, dy, aff = _lattice_dev(R, C)
    dx, dg, db = _bn_bwd(K, x, dy, aff, relu, R, C)
    i1, i2 = P.bwd_sums_int(R, C, relu)
    xl, dyl = P.lattice(R, C)[:2]
    ref_dx = P.bn_bwd(xl, dyl, *P.lattice_affine(R, C), relu)[0]
    e = _rel(dx, _t64(ref_dx))
    print(f"[{R}x{C} relu={relu}] {'16-byte' if C % 4 == 0 else 'scalar'} forms, dx rel err = {e:.2e} on {dx.numel()} elements")
    _assert_exact(_n(db), i1, f"[{R}x{C} relu={relu}] dbeta")
    _assert_exact(2 * _n(dg).astype(np.float64), i2, f"[{R}x{C} relu={relu}] 2 dgamma")
    assert e <= BWD


@functools.lru_cache(maxsize=None)
def _real_case(R, C):
    """real-valued x (kept clear of the ReLU's kink), dy, gamma, beta and the float64 statistics of x"""
    gamma, beta = _params(C)
    x = P.kink_free((fill_tensor(f"pre.x{R}", (R, C), "code") * 1.5 + 0.7).numpy(), gamma, beta)
    dy = fill_tensor(f"pre.dy{R}", (R, C), "code").numpy()
    x.setflags(write=False)
    return x, dy, gamma, beta, P.bn_train(x, gamma, beta)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("R,C", P.VEC_SHAPES, ids=_ids(P.VEC_SHAPES))
def test_batch_norm_act_wrapper_on_real_data(K, R, C, relu):
    """K.batch_norm_act in training mode with and without the ReLU against float64 (the references equal autograd: test_pointnet_rows_host.py)"""
    x, dy, gamma, beta, (mean, var, rstd, scale, shift) = _real_case(R, C)
    bn = torch.nn.BatchNorm1d(C).cuda()
    with torch.no_grad():
        bn.weight.copy_(_d(gamma)); bn.bias.copy_(_d(beta))
    ref_rm, ref_rv = P.running((np.zeros(C), np.ones(C)), mean, var, R, bn.momentum)
    ref_dx, ref_dg, ref_db = P.bn_bwd(x, dy, scale, shift, mean, rstd, relu)
    xg = _d(x).requires_grad_(True)
    y = K.batch_norm_act(xg, bn, True, relu=relu)
    (y * _d(dy)).sum().backward()
    e = dict(y=_rel(y, _t64(P.affine_act(x, scale, shift, relu))), dx=_rel(xg.grad, _t64(ref_dx)), dgamma=_rel(bn.weight.grad, _t64(ref_dg)),
             dbeta=_rel(bn.bias.grad, _t64(ref_db)), running_mean=_rel(bn.running_mean, _t64(ref_rm)), running_var=_rel(bn.running_var, _t64(ref_rv)))
    print(f"[{R}x{C} relu={relu}] " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["y"] <= FWD and max(e["dx"], e["dgamma"], e["dbeta"]) <= BWD and max(e["running_mean"], e["running_var"]) <= RUN
    assert int(bn.num_batches_tracked) == 1


# ---- 4. the SyncBatchNorm pieces ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("R,C", P.SHAPES, ids=_ids(P.SHAPES))
def test_backward_sums_then_apply(K, R, C, relu):
    x, dy, aff = _lattice_dev(R, C)
    s1, s2 = _bwd_sums(K, x, dy, aff, relu, R, C)
    dx = _bwd_apply(K, x, dy, aff, s1, s2, R, relu, R, C)
    i1, i2 = P.bwd_sums_int(R, C, relu)
    _assert_exact(_n(s1), i1, f"[{R}x{C} relu={relu}] sum_dy")
    _assert_exact(2 * _n(s2).astype(np.float64), i2, f"[{R}x{C} relu={relu}] 2 sum_dy_xhat")
    if C % 4:
        fdx, fdg, fdb = _bn_bwd(K, x, dy, aff, relu, R, C)
        same = [torch.equal(_bits(a), _bits(b)) for a, b in ((dx, fdx), (s2, fdg), (s1, fdb))]
        print(f"[{R}x{C} relu={relu}] bit-identical to act_bn_bwd_f32 (dx, dgamma, dbeta): {same}")
        assert all(same)
    else:
        xl, dyl = P.lattice(R, C)[:2]
        e = _rel(dx, _t64(P.bn_bwd(xl, dyl, *P.lattice_affine(R, C), relu)[0]))
        print(f"[{R}x{C} relu={relu}] dx rel err = {e:.2e}")
        assert e <= BWD


@pytest.mark.parametrize("relu", [0, 1])
def test_two_shards_add_up_to_the_full_backward(K, relu):
    """rows [0, 37) and [37, 65) of the (65, 68) lattice as two ranks would hold them, in one process: no process group"""
    R, C, cut = 65, 68, 37
    x, dy, aff = _lattice_dev(R, C)
    shards = [(x[:cut].contiguous(), dy[:cut].contiguous(), cut), (x[cut:].contiguous(), dy[cut:].contiguous(), R - cut)]
    sums = [_bwd_sums(K, xs, ds, aff, relu, n, C) for xs, ds, n in shards]
    full1, full2 = P.bwd_sums_int(R, C, relu)
    for (s1, s2), rows in zip(sums, (slice(0, cut), slice(cut, R))):
        i1, i2 = P.bwd_sums_int(R, C, relu, rows)
        _assert_exact(_n(s1), i1, f"[rows {rows.start}:{rows.stop} relu={relu}] sum_dy")
        _assert_exact(2 * _n(s2).astype(np.float64), i2, f"[rows {rows.start}:{rows.stop} relu={relu}] 2 sum_dy_xhat")
    t1, t2 = sums[0][0] + sums[1][0], sums[0][1] + sums[1][1]                              # what the all-reduce leaves on every rank
    _assert_exact(_n(t1), full1, f"[relu={relu}] shard sums of sum_dy"); _assert_exact(2 * _n(t2).astype(np.float64), full2, f"[relu={relu}] shard sums of 2 sum_dy_xhat")
    xl, dyl = P.lattice(R, C)[:2]
    ref = P.bn_bwd(xl, dyl, *P.lattice_affine(R, C), relu)[0]
    for (xs, ds, n), rows in zip(shards, (slice(0, cut), slice(cut, R))):
        e = _rel(_bwd_apply(K, xs, ds, aff, t1, t2, R, relu, n, C), _t64(ref[rows]))
        print(f"[rows {rows.start}:{rows.stop} relu={relu}] dx of the shard against the full backward: rel err = {e:.2e}")
        assert e <= BWD


# ---- 5. dead groups ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,n,C", P.LIVE_SHAPES, ids=_ids(P.LIVE_SHAPES))
def test_dead_groups_are_not_read_at_ragged_sizes(K, G, n, C):
    R = G * n
    dy = P.lattice(R, C)[1]
    x, _, aff = _lattice_dev(R, C)
    dead = [g for g in (1, 3) if g < G]
    live = np.ones(G, np.int32); live[dead] = 0
    rows_dead = np.repeat(live == 0, n)
    zero, garbage = dy.copy(), dy.copy()
    zero[rows_dead] = 0.0; garbage[rows_dead] = 7.0
    assert P.launch(R, C)[0] >= 2 and P.launch(R, C)[1] % n                               # a part boundary inside a group
    for relu in (0, 1):
        a = _bn_bwd(K, x, _d(zero), aff, relu, R, C)
        b = _bn_bwd(K, x, _d(garbage), aff, relu, R, C, _d(live, torch.int32), n)
        same = [torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b)]
        e = _rel(b[0], _t64(P.bn_bwd(P.lattice(R, C)[0], zero, *P.lattice_affine(R, C), relu)[0]))
        print(f"[{G}x{n}x{C} relu={relu}] dead groups {dead}: bit-identical (dx, dgamma, dbeta) = {same}, dx rel err = {e:.2e}")
        assert all(same) and e <= BWD


# ---- 6. argument checks (every call returns before a launch) -----------------------------------------------------------------------------------
def test_refused_calls_touch_nothing(K):
    lib = K.lib
    R, C = 8, 8
    x, dy = torch.ones(R * C + 4, device="cuda"), torch.ones(R, C, device="cuda")
    x0 = x[:R * C].view(R, C)
    aff = [torch.ones(C, device="cuda") for _ in range(4)]
    s1, s2 = torch.ones(C, device="cuda"), torch.ones(C, device="cuda")
    need = lib.act_colstats_workspace(R, C)
    ws = torch.full((need // 4 + GUARD,), 7.0, device="cuda")
    outs = dict(dx=_empty(R, C), a=_empty(C), b=_empty(C), c=_empty(C), d=_empty(C))
    p = lambda t: t.data_ptr()
    A = [p(a) for a in aff]
    dx, oa, ob, oc, od = (p(outs[k]) for k in ("dx", "a", "b", "c", "d"))
    live = torch.ones(3, dtype=torch.int32, device="cuda")
    st = _st()
    stats = lambda x_=p(x0), R_=R, wsb=need: lib.act_bn_stats_f32(x_, R_, C, A[0], A[1], P.BN_EPS, 0.1, None, None, oa, ob, oc, od, p(ws), wsb, st)
    meanvar = lambda x_=p(x0), R_=R, wsb=need: lib.act_col_mean_var_f32(x_, R_, C, oa, ob, p(ws), wsb, st)
    bwd = lambda x_=p(x0), R_=R, wsb=need: lib.act_bn_bwd_f32(x_, p(dy), *A, 1, R_, C, dx, oa, ob, p(ws), wsb, st)
    sums = lambda x_=p(x0), R_=R, wsb=need: lib.act_bn_bwd_sums_f32(x_, p(dy), *A, 1, R_, C, oa, ob, p(ws), wsb, st)
    apply = lambda x_=p(x0), R_=R, count=8.0: lib.act_bn_bwd_apply_f32(x_, p(dy), *A, p(s1), p(s2), count, 1, R_, C, dx, st)
    calls = {}
    for name, f in (("bn_stats", stats), ("col_mean_var", meanvar), ("bn_bwd", bwd), ("bn_bwd_sums", sums), ("bn_bwd_apply", apply)):
        calls[f"{name}: null x"] = (f(x_=None), ACT_E_NULLPTR)
        calls[f"{name}: R = 0"] = (f(R_=0), ACT_E_BADARG)
        if name != "bn_bwd_apply":
            calls[f"{name}: workspace one float short"] = (f(wsb=need - 4), ACT_E_BADARG)
    calls["bn_bwd_apply: count = 0"] = (apply(count=0.0), ACT_E_BADARG)
    calls["bn_bwd_groups: R % n != 0"] = (lib.act_bn_bwd_groups_f32(p(x0), p(dy), *A, 1, R, C, p(live), 3, dx, oa, ob, p(ws), need, st), ACT_E_BADARG)
    calls["bn_bwd: x one float past a 16-byte boundary at C = 8"] = (bwd(x_=p(x0) + 4), ACT_E_BADARG)
    calls["affine_act: C = 6"] = (lib.act_affine_act_f32(p(x0), A[0], A[1], 1, R, 6, dx, st), ACT_E_BADARG)
    calls["affine_act: null y"] = (lib.act_affine_act_f32(p(x0), A[0], A[1], 1, R, C, None, st), ACT_E_NULLPTR)
    calls["group_max: null out"] = (lib.act_group_max_f32(p(x0), 2, 4, C, None, None, st), ACT_E_NULLPTR)
    calls["group_max: n = 0"] = (lib.act_group_max_f32(p(x0), 2, 0, C, dx, None, st), ACT_E_BADARG)
    calls["group_max_bwd: null arg"] = (lib.act_group_max_bwd_f32(p(dy), None, 2, 4, C, 0, dx, st), ACT_E_NULLPTR)
    calls["group_sum: C = 0"] = (lib.act_group_sum_f32(p(x0), 2, 4, 0, dx, st), ACT_E_BADARG)
    calls["bn_tiles_finalize: tiles = 0"] = (lib.act_bn_tiles_finalize_f32(p(x0), 0, 4, C, A[0], A[1], P.BN_EPS, 0.1, None, None, oa, ob, oc, od, st), ACT_E_BADARG)
    calls["bn_eval_affine: null scale"] = (lib.act_bn_eval_affine_f32(A[0], A[1], A[2], A[3], P.BN_EPS, C, None, oa, st), ACT_E_NULLPTR)
    torch.cuda.synchronize()
    for name, (got, want) in calls.items():
        print(f"{name}: returned {got} (expected {want})")
    assert all(got == want for got, want in calls.values())
    assert all(bool((t == 7.0).all()) for t in outs.values()) and bool((ws == 7.0).all())


# ---- tile and eval finalizers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles,rpt,C", P.TILE_SHAPES, ids=_ids(P.TILE_SHAPES))
def test_tile_statistics_finalize(K, tiles, rpt, C):
    r = np.random.default_rng(tiles * 131 + C)
    X = (1.5 * r.standard_normal((tiles * rpt, C)) + 0.7).astype(np.float32)
    ts = P.tile_stats(X, tiles, rpt)
    gamma, beta = _params(C)
    mean_ref, var_ref = P.chan(ts, rpt)
    rstd_ref = 1.0 / np.sqrt(var_ref + P.BN_EPS)
    scale_ref = gamma * rstd_ref
    refs = [mean_ref, rstd_ref, scale_ref, beta - mean_ref * scale_ref]
    rm0, rv0 = r.standard_normal(C).astype(np.float32), (1 + r.random(C)).astype(np.float32)
    refs += list(P.running((rm0, rv0), mean_ref, var_ref, tiles * rpt, 0.1))
    rm, rv, g, b = _d(rm0), _d(rv0), _d(gamma), _d(beta)
    out = [_empty(C) for _ in range(4)]
    assert K.lib.act_bn_tiles_finalize_f32(_d(ts).data_ptr(), tiles, rpt, C, g.data_ptr(), b.data_ptr(), P.BN_EPS, 0.1, rm.data_ptr(), rv.data_ptr(),
                                           *(o.data_ptr() for o in out), _st()) == 0
    e = [_rel(a, _t64(ref)) for a, ref in zip(out + [rm, rv], refs)]
    direct = _bn_stats(K, _d(X), tiles * rpt, C, g, b, 0.1, None, None)
    e2 = [_rel(a, d_.double()) for a, d_ in zip(out, direct)]
    print(f"[{tiles}x{rpt}x{C}] mean, rstd, scale, shift, running mean, var against Chan in float64: " + ", ".join(f"{v:.2e}" for v in e))
    print(f"[{tiles}x{rpt}x{C}] mean, rstd, scale, shift against act_bn_stats_f32 on the matrix: " + ", ".join(f"{v:.2e}" for v in e2))
    if rpt == 1:
        assert not ts[:, 1].any()
    assert max(e) <= RUN and max(e2) <= FWD


@pytest.mark.parametrize("C", P.EVAL_C)
def test_eval_affine(K, C):
    r = np.random.default_rng(C)
    gamma, beta = _params(C)
    rm, rv = r.standard_normal(C).astype(np.float32), (0.5 + r.random(C)).astype(np.float32)
    scale, shift = torch.full((C + GUARD,), 7.0, device="cuda"), torch.full((C + GUARD,), 7.0, device="cuda")
    assert K.lib.act_bn_eval_affine_f32(_d(gamma).data_ptr(), _d(beta).data_ptr(), _d(rm).data_ptr(), _d(rv).data_ptr(), P.BN_EPS, C, scale.data_ptr(),
                                        shift.data_ptr(), _st()) == 0
    rs, rh = P.eval_affine(gamma, beta, rm, rv)
    e = _rel(scale[:C], _t64(rs)), _rel(shift[:C], _t64(rh))
    print(f"[C={C}] scale, shift rel err = {e[0]:.2e}, {e[1]:.2e}")
    assert max(e) <= 1e-6 and (scale[C:] == 7.0).all() and (shift[C:] == 7.0).all()


# ---- group kernels -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,n,C", P.GROUP_SHAPES, ids=_ids(P.GROUP_SHAPES))
def test_group_max_forward_and_backward(K, G, n, C):
    lib = K.lib
    xh, planted = P.group_input(G, n, C)
    ref_out, ref_arg = P.group_max(xh, n)
    x = _d(xh)
    out, arg = torch.full((G * C + GUARD,), 7.0, device="cuda"), torch.full((G * C + GUARD,), 7, dtype=torch.int32, device="cuda")
    assert lib.act_group_max_f32(x.data_ptr(), G, n, C, out.data_ptr(), arg.data_ptr(), _st()) == 0
    out2 = torch.full((G * C + GUARD,), 7.0, device="cuda")
    assert lib.act_group_max_f32(x.data_ptr(), G, n, C, out2.data_ptr(), None, _st()) == 0
    o, a = _n(out[:G * C]).reshape(G, C), _n(arg[:G * C]).reshape(G, C)
    print(f"[{G}x{n}x{C}] planted: " + ", ".join(f"{k} at (group, column) {v}: out {o[v]!r} arg {a[v]}" for k, v in planted.items()))
    nb, na = int((o.view(np.int32) != ref_out.view(np.int32)).sum()), int((a != ref_arg).sum())
    print(f"[{G}x{n}x{C}] {nb} of {G * C} maxima differ in bits from numpy, {na} arg differ from np.argmax")
    assert nb == 0 and na == 0
    assert torch.equal(_bits(out2), _bits(out)) and (out[G * C:] == 7.0).all() and (arg[G * C:] == 7).all()
    # backward: the scatter, then one add per element on a pre-filled din
    r = np.random.default_rng(G + n)
    dout = r.standard_normal((G, C)).astype(np.float32)
    pre = r.standard_normal((G * n, C)).astype(np.float32)
    scatter = P.group_max_bwd(dout, ref_arg, n)
    din = torch.full((G * n * C + GUARD,), 7.0, device="cuda")
    assert lib.act_group_max_bwd_f32(_d(dout).data_ptr(), arg.data_ptr(), G, n, C, 0, din.data_ptr(), _st()) == 0
    acc = torch.cat([_d(pre).flatten(), torch.full((GUARD,), 7.0, device="cuda")])
    assert lib.act_group_max_bwd_f32(_d(dout).data_ptr(), arg.data_ptr(), G, n, C, 1, acc.data_ptr(), _st()) == 0
    d0 = int((_n(din[:G * n * C]).view(np.int32) != scatter.ravel().view(np.int32)).sum())
    d1 = int((_n(acc[:G * n * C]).view(np.int32) != (pre + scatter).ravel().view(np.int32)).sum())
    print(f"[{G}x{n}x{C}] backward: {d0} (accumulate = 0), {d1} (accumulate = 1) of {G * n * C} elements differ in bits")
    assert d0 == 0 and d1 == 0 and (din[G * n * C:] == 7.0).all() and (acc[G * n * C:] == 7.0).all()


SUM_SHAPES = [(9, n, 130) for n in P.SUM_N] + [P.GROUP_SHAPES[-1]]


@pytest.mark.parametrize("G,n,C", SUM_SHAPES, ids=_ids(SUM_SHAPES))
def test_group_sum(K, G, n, C):
    r = np.random.default_rng(G * n + C)
    xi = r.integers(-4, 5, (G * n, C)).astype(np.float32)
    xr = r.standard_normal((G * n, C)).astype(np.float32)
    out = torch.full((G * C + GUARD,), 7.0, device="cuda")
    assert K.lib.act_group_sum_f32(_d(xi).data_ptr(), G, n, C, out.data_ptr(), _st()) == 0
    _assert_exact(_n(out[:G * C]).reshape(G, C), P.group_sum(xi, n, np.int64), f"[{G}x{n}x{C}] group_sum on the lattice")
    assert (out[G * C:] == 7.0).all()
    assert K.lib.act_group_sum_f32(_d(xr).data_ptr(), G, n, C, out.data_ptr(), _st()) == 0
    e = _rel(out[:G * C].view(G, C), _t64(P.group_sum(xr, n)))
    print(f"[{G}x{n}x{C}] group_sum on real data: rel err = {e:.2e}")
    assert e <= 1e-6


def test_linear_group_add_gradient_of_the_group_term(K):
    G, n, Cin, Cout = 7, 13, 64, 48
    x, w = fill_tensor("pre.lx", (G * n, Cin), "code"), fill_tensor("pre.lw", (Cout, Cin), "code") * 0.1
    g, d = fill_tensor("pre.lg", (G, Cout), "code"), fill_tensor("pre.ld", (G * n, Cout), "code")
    ts = [t.double().requires_grad_(True) for t in (x, w, g)]
    ref = (ts[0] @ ts[1].t()).view(G, n, Cout) + ts[2].unsqueeze(1)
    (ref.reshape(G * n, Cout) * d.double()).sum().backward()
    tg = [t.cuda().requires_grad_(True) for t in (x, w, g)]
    y = K.linear_group_add(tg[0], tg[1], tg[2], n)
    (y * d.cuda()).sum().backward()
    e = _rel(y, ref.reshape(G * n, Cout)), _rel(tg[2].grad, ts[2].grad), _rel(tg[2].grad, _t64(P.group_sum(d.numpy(), n)))
    print(f"[{G}x{n}] y rel err = {e[0]:.2e}, dg against autograd = {e[1]:.2e}, against the reference sum = {e[2]:.2e}")
    assert e[0] <= FWD and e[1] <= 1e-6 and e[2] <= 1e-6


# ---- the first row -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,A", P.PIVOT_CASES)
def test_batchnorm_statistics_do_not_depend_on_the_first_row(K, R, A):
    """x = 1.5 N(0,1) + 0.7 at C = 64 with one row set to A, as row 0 and as row R / 2: the same multiset, so the same statistics.  Sums pivoted on
    row 0 of the tensor cancel here (var = q / R - dm^2 with dm ~ A).  torch's own float32 CPU batch_norm handles every one of these inputs to
    2e-6 (asserted below; measured 1.2e-7 ... 4.0e-7), so they are inputs a float32 BatchNorm must handle.  The ReLU is left off: the
    statistics are the subject, and without it every output element is compared and no derivative hangs on the sign of an output within
    rounding of zero.  The statistics pass keeps lane-pivoted (mean, M2) partials next to its row-0 sums for these inputs (column_mean_var)."""
    C = P.PIVOT_C
    F = torch.nn.functional
    gamma, beta = _params(C)
    order = torch.arange(R); order[0], order[R // 2] = R // 2, 0                          # the swap of the two rows (its own inverse)
    dy0 = fill_tensor(f"pre.pdy{R}", (R, C), "code")
    res = []
    for tag, xh, dy in zip(("row 0 = A", "row R/2 = A"), P.pivot_input(R, A), (dy0, dy0[order])):   # the gradient follows its row
        xt = torch.from_numpy(xh.copy())
        xd = xt.double().requires_grad_(True)
        rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
        yr = F.batch_norm(xd, rm, rv, _t64(gamma), _t64(beta), True, 0.1, P.BN_EPS)
        (yr * dy.double()).sum().backward()
        cpu32 = F.batch_norm(xt, None, None, torch.from_numpy(gamma), torch.from_numpy(beta), True, 0.1, P.BN_EPS)
        pre = _rel(cpu32, yr)
        bn = torch.nn.BatchNorm1d(C).cuda()
        with torch.no_grad():
            bn.weight.copy_(_d(gamma)); bn.bias.copy_(_d(beta))
        xg = xt.cuda().requires_grad_(True)
        y = K.batch_norm_act(xg, bn, True, relu=False)
        (y * dy.cuda()).sum().backward()
        e = dict(y=_rel(y, yr), running_mean=_rel(bn.running_mean, rm), running_var=_rel(bn.running_var, rv), dx=_rel(xg.grad, xd.grad))
        print(f"[R={R} A={A:g}] {tag}: torch fp32 CPU {pre:.2e}; device " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
        res.append((pre, e, y.detach(), xg.grad, bn.running_var.clone()))
    swap = lambda t: t[order.to(t.device)]
    between = dict(y=_rel(swap(res[1][2]), res[0][2].double()), dx=_rel(swap(res[1][3]), res[0][3].double()), running_var=_rel(res[1][4], res[0][4].double()))
    print(f"[R={R} A={A:g}] the two row orders against each other: " + ", ".join(f"{k} {v:.2e}" for k, v in between.items()))
    for pre, e, *_ in res:
        assert pre <= 2e-6                                                                # the precondition: an input a float32 BatchNorm handles
        assert e["y"] <= FWD and e["running_var"] <= RUN and e["running_mean"] <= RUN and e["dx"] <= BWD
    assert between["y"] <= FWD and between["dx"] <= BWD and between["running_var"] <= RUN


# ---- the lane-pivoted partials and the far-pivot branch at ragged sizes --------------------------------------------------------------------------
@pytest.mark.parametrize("R,C", P.SHAPES, ids=_ids(P.SHAPES))
def test_part_mean_and_m2_partials(K, R, C):
    """rows 2 and 3 of the statistics pass's partials [nparts][4][C]: every part's (mean, M2) from the lane-pivoted sums, merged over row-lanes
    that hold unequal numbers of rows or none.  Bounds as for the whole column: a handful of float32 roundings of shifted values <= 2 max|x|,
    M2 being n_p times a variance."""
    xl = P.lattice(R, C)[0]
    nparts, rpb, last = P.LAUNCH[(R, C)]
    mean, var = _empty(C), _empty(C)
    ws = _Workspace(K, R, C)
    assert K.lib.act_col_mean_var_f32(_lattice_dev(R, C)[0].data_ptr(), R, C, mean.data_ptr(), var.data_ptr(), ws.ptr(), ws.bytes, _st()) == 0
    ws.check()
    got = _n(ws.t[:nparts * 4 * C]).reshape(nparts, 4, C).astype(np.float64)
    ms, qs, ns = P.part_stats(xl, R, C)
    assert ns[-1] == last and (ns[:-1] == rpb).all()
    amax = float(np.abs(xl).max())
    em = np.abs(got[:, 2] - ms).max() / (4 * P.EPS32 * 2 * amax)
    eq = (np.abs(got[:, 3] - qs) / (ns[:, None] * 8 * P.EPS32 * (2 * amax) ** 2)).max()
    print(f"[{R}x{C}] {nparts} parts of {rpb} rows, last {last} (rows per lane {[(last - l + 3) // 4 if last > l else 0 for l in range(4)]}): "
          f"part mean err / bound = {em:.3f}, part M2 err / bound = {eq:.3f}")
    assert em <= 1 and eq <= 1


@pytest.mark.parametrize("R,C", P.FAR_SHAPES, ids=_ids(P.FAR_SHAPES))
def test_first_row_outlier_at_ragged_shapes(K, R, C):
    """the lattice with 64.0 in row 0 of every third column: those columns take Chan's combination of the parts (shorter last part, fewer parts
    than part-lanes, a partial column block), their neighbours in the same workgroup keep the row-0 form.  scale, shift and the running statistics
    against the exact rational to the file's 1e-5, in both row orders and against each other; the near columns bit-identical to the plain lattice."""
    gamma, beta = _params(C)
    g, b = _d(gamma), _d(beta)
    far = np.arange(C) % 3 == 0
    r = np.random.default_rng(R)
    rm0, rv0 = r.standard_normal(C).astype(np.float32), (1 + r.random(C)).astype(np.float32)
    outs = []
    for tag, xh in zip(("outlier in row 0", "outlier in row R/2"), P.outlier_lattice(R, C)):
        m_ref, v_ref = P.exact_mean_var(xh)
        scale_ref = gamma.astype(np.float64) / np.sqrt(v_ref + P.BN_EPS)
        refs = [scale_ref, beta.astype(np.float64) - m_ref * scale_ref, *P.running((rm0, rv0), m_ref, v_ref, R, 0.1)]
        rm, rv = _d(rm0), _d(rv0)
        x = _d(xh)
        mean, rstd, scale, shift = _bn_stats(K, x, R, C, g, b, 0.1, rm, rv)
        cm, cv = _col_mean_var(K, x, R, C)
        e = [_rel(t, _t64(ref)) for t, ref in zip((scale, shift, rm, rv), refs)] + [_rel(cm, _t64(m_ref)), _rel(cv, _t64(v_ref))]
        print(f"[{R}x{C}] {tag}: scale, shift, running mean, running var, mean, var rel err = " + ", ".join(f"{v:.2e}" for v in e))
        assert max(e) <= RUN and torch.equal(_bits(cm), _bits(mean))
        outs.append((mean, rstd, scale, shift, rm, rv))
    between = [_rel(p, q.double()) for p, q in zip(*outs)]
    print(f"[{R}x{C}] the two row orders against each other: " + ", ".join(f"{v:.2e}" for v in between))
    assert max(between) <= RUN
    plain = _bn_stats(K, _lattice_dev(R, C)[0], R, C, g, b, 0.1, None, None)
    near = torch.from_numpy(~far).cuda()
    same = [torch.equal(_bits(p[near]), _bits(q[near])) for p, q in zip(plain, outs[0][:4])]
    print(f"[{R}x{C}] near columns of the outlier run bit-identical to the plain lattice (mean, rstd, scale, shift): {same}")
    assert all(same)


def test_either_side_of_the_far_pivot_switch(K):
    """R = 262,144 rows of 1.5 N(0,1) + 0.7 with row 0 placed 4.8 (even columns: row-0 form, dm^2 / var = 23) and 5.3 (odd columns: Chan's
    combination, 28) standard deviations from the mean: the row-0 form at its worst admissible pivot and the largest row count of the models"""
    x = P.edge_input()
    R, C = x.shape
    gamma, beta = _params(C)
    mean, var, rstd, scale, shift = P.bn_train(x, gamma, beta)
    ref_rm, ref_rv = P.running((np.zeros(C), np.ones(C)), mean, var, R, 0.1)
    bn = torch.nn.BatchNorm1d(C).cuda()
    with torch.no_grad():
        bn.weight.copy_(_d(gamma)); bn.bias.copy_(_d(beta))
    y = K.batch_norm_act(_d(x), bn, True, relu=False)
    ref = _t64(P.affine_act(x, scale, shift, False))
    for name, cols in (("row-0 form, 4.8 sigma", slice(0, None, 2)), ("Chan's combination, 5.3 sigma", slice(1, None, 2))):
        e = _rel(y[:, cols], ref[:, cols]), _rel(bn.running_mean[cols], _t64(ref_rm[cols])), _rel(bn.running_var[cols], _t64(ref_rv[cols]))
        print(f"[{R}x{C}] {name}: y {e[0]:.2e}, running mean {e[1]:.2e}, running var {e[2]:.2e}")
        assert e[0] <= FWD and max(e[1:]) <= RUN
