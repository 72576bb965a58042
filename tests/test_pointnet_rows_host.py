"""CPU: the numpy references of tests/pointnet_rows_ref.py against torch float64 autograd, F.batch_norm and torch.max on every shape at which
tests/test_gpu_pointnet_rows_edges.py uses them, the launch table those shapes were chosen from, and the exactness of the lattice inputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pointnet_rows_ref as P

_ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]
T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _close(a, ref, tol=1e-12):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() <= tol * max(1.0, np.abs(ref).max())


def _params(C, seed):
    r = np.random.default_rng(seed)
    return 1 + 0.2 * r.standard_normal(C), 0.1 * r.standard_normal(C)


def test_launch_table_is_the_arithmetic_of_stats_parts():
    for (R, C), row in P.LAUNCH.items():
        assert P.launch(R, C) == row, (R, C)
        assert P.workspace_floats(R, C) >= row[0] * 4 * C
    assert P.launch(200003, 64)[0] < 1024 == min(2048, (200003 + 63) // 64, 1024)        # the cap binds; rounding rows_per_block to 4 leaves 1,021
    assert 33000 * 66 > P.GRID_CAP and 200003 * 64 // 4 > P.GRID_CAP
    G, n, C = P.GROUP_SHAPES[-1]
    assert G * C > P.GRID_CAP and G * n * C > P.GRID_CAP
    # rows per row-lane: the unrolled loop of stage 1 (four rows of a lane = 16 rows) and of the 16-byte form (64 rows) each run three times, then the tail
    rpb = P.LAUNCH[(200003, 64)][1]
    assert rpb // 16 >= 3 and rpb % 16 and rpb // 64 == 3 and rpb % 64


@pytest.mark.parametrize("R,C", P.SHAPES, ids=_ids(P.SHAPES))
def test_lattice_sums_are_exact_in_float32(R, C):
    """every sum the lattice tests compare for equality stays below 2^24 in the unit it is a multiple of, so float32 adds it exactly in any order"""
    x, dy, mean, k = (a.astype(np.int64) for a in P.lattice(R, C))
    assert np.abs(x).max() <= 4 and np.abs(dy).max() <= 2 and (0.25 < (dy == 0).mean() < 0.42 or R * C < 100)
    assert (np.abs(dy).sum(0)).max() < 2 ** 24                                            # sum dyh, units of 1
    assert (np.abs(dy * (x - mean))).sum(0).max() < 2 ** 24                               # sum dyh xhat, units of 1/2
    assert ((np.abs(x) + 4) ** 2).sum(0).max() < 2 ** 24                                  # sum (x - pivot)^2 for any pivot on the lattice
    for relu in (0, 1):
        scale, shift, mu, rstd = P.lattice_affine(R, C)
        s1, s2 = P.bwd_sums(*P.lattice(R, C)[:2], scale, shift, mu, rstd, relu)
        i1, i2 = P.bwd_sums_int(R, C, relu)
        assert np.array_equal(s1, i1) and np.array_equal(2 * s2, i2)
    m, v = P.exact_mean_var(P.lattice(R, C)[0])
    m2, v2 = P.mean_var(P.lattice(R, C)[0])
    assert _close(m, m2, 1e-10) and _close(v, v2, 1e-10)       # (numpy adds a column's 200,003 float64 terms one after the other)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("R,C", P.SHAPES, ids=_ids(P.SHAPES))
def test_batchnorm_references_against_autograd(R, C, relu):
    r = np.random.default_rng(R + C)
    gamma, beta = _params(C, C)
    x = P.kink_free((1.5 * r.standard_normal((R, C)) + 0.7).astype(np.float32), gamma, beta)
    dy = r.standard_normal((R, C))
    mean, var, rstd, scale, shift = P.bn_train(x, gamma, beta)
    xt = T(x).requires_grad_(True); g, b = T(gamma).requires_grad_(True), T(beta).requires_grad_(True)
    for momentum in (0.1, 1.0):
        rm0, rv0 = r.standard_normal(C), 1 + r.random(C)
        rm, rv = T(rm0).clone(), T(rv0).clone()
        y = F.batch_norm(xt, rm, rv, g, b, True, momentum, P.BN_EPS)
        ref_rm, ref_rv = P.running((rm0, rv0), mean, var, R, momentum)
        if R > 1:
            assert _close(ref_rm, rm.numpy()) and _close(ref_rv, rv.numpy())
    y = torch.relu(y) if relu else y
    assert _close(P.affine_act(x, scale, shift, relu), y.detach().numpy())
    assert np.abs(P.affine_act(x, scale, shift, False)).min() >= P.KINK_MARGIN            # kink_free: the ReLU's derivative is unambiguous
    y.backward(T(dy))
    dx, dgamma, dbeta = P.bn_bwd(x, dy, scale, shift, mean, rstd, relu)
    assert _close(dx, xt.grad.numpy(), 1e-10) and _close(dgamma, g.grad.numpy(), 1e-10) and _close(dbeta, b.grad.numpy(), 1e-10)
    # two shards: the sums add up, and apply with the full count gives the rows of the full backward
    cut = max(1, R * 37 // 65)
    parts = [P.bwd_sums(x[s], dy[s], scale, shift, mean, rstd, relu) for s in (slice(0, cut), slice(cut, R))]
    s1, s2 = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    assert _close(s1, dbeta) and _close(s2, dgamma)
    assert _close(P.bwd_apply(x[:cut], dy[:cut], scale, shift, mean, rstd, s1, s2, float(R), relu), dx[:cut])


@pytest.mark.parametrize("tiles,rpt,C", P.TILE_SHAPES, ids=_ids(P.TILE_SHAPES))
def test_chan_combination_of_tile_statistics(tiles, rpt, C):
    r = np.random.default_rng(tiles + C)
    X = 1.5 * r.standard_normal((tiles * rpt, C)) + 0.7
    T64 = X.reshape(tiles, rpt, C)
    exact = np.stack([T64.mean(1), ((T64 - T64.mean(1, keepdims=True)) ** 2).sum(1)], axis=1)
    mean, var = P.chan(exact, rpt)
    m2, v2 = P.mean_var(X)
    assert _close(mean, m2) and _close(var, v2)
    ts = P.tile_stats(X, tiles, rpt)
    assert ts.dtype == np.float32 and ts.shape == (tiles, 2, C) and np.abs(ts - exact).max() <= 2 * P.EPS32 * np.abs(exact).max()
    if rpt == 1:
        assert not ts[:, 1].any()


@pytest.mark.parametrize("C", P.EVAL_C)
def test_eval_affine_is_batch_norm_in_eval_mode(C):
    r = np.random.default_rng(C)
    gamma, beta = _params(C, C)
    rm, rv = r.standard_normal(C), 0.5 + r.random(C)
    x = r.standard_normal((3, C))
    scale, shift = P.eval_affine(gamma, beta, rm, rv)
    assert _close(P.affine_act(x, scale, shift, False), F.batch_norm(T(x), T(rm), T(rv), T(gamma), T(beta), False, 0.1, P.BN_EPS).numpy())


@pytest.mark.parametrize("G,n,C", P.GROUP_SHAPES, ids=_ids(P.GROUP_SHAPES))
def test_group_references_against_torch_max_and_autograd(G, n, C):
    x, planted = P.group_input(G, n, C)
    out, arg = P.group_max(x, n)
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    tout, targ = xt.view(G, n, C).max(dim=1)
    assert np.array_equal(out.view(np.int32), tout.detach().numpy().view(np.int32))       # bits: the sign of a zero included
    for name, (g, c) in planted.items():
        want = {"tie": 0, "+0/-0 tie (+0 first)": 0, "-0/+0 tie (-0 first)": 0, "all -inf": 0, "maximum in the last row": n - 1}[name]
        assert arg[g, c] == want, name
    # torch.max leaves the index of a tie to the implementation; away from the planted ties the maximum is unique
    tied = np.zeros((G, C), bool)
    for name, (g, c) in planted.items():
        tied[g, c] = "tie" in name or "inf" in name
    assert np.array_equal(arg[~tied], targ.numpy()[~tied])
    dout = np.random.default_rng(G).standard_normal((G, C)).astype(np.float32)
    if not tied.any() or n == 1:
        tout.backward(torch.from_numpy(dout))
        assert np.array_equal(P.group_max_bwd(dout, arg, n), xt.grad.numpy())
    din = P.group_max_bwd(dout, arg, n).reshape(G, n, C)
    assert np.array_equal(din.sum(1), dout) and (din != 0).sum() <= G * C
    assert np.array_equal(np.take_along_axis(din, arg.astype(np.int64)[:, None, :], 1)[:, 0], dout)


@pytest.mark.parametrize("n", P.SUM_N)
def test_group_sum_reference(n):
    r = np.random.default_rng(n)
    x = r.standard_normal((7 * n, 5))
    assert _close(P.group_sum(x, n), T(x).view(7, n, 5).sum(1).numpy())
    xi = r.integers(-4, 5, (7 * n, 5)).astype(np.float32)
    assert np.array_equal(P.group_sum(xi, n, np.int64), xi.reshape(7, n, 5).sum(1).astype(np.int64))


@pytest.mark.parametrize("R,A", P.PIVOT_CASES)
def test_pivot_inputs_are_ones_a_float32_batchnorm_handles(R, A):
    """the precondition of test_batchnorm_statistics_do_not_depend_on_the_first_row, on the CPU: torch's own fp32 F.batch_norm is within 2e-6"""
    for x in P.pivot_input(R, A):
        ref = F.batch_norm(torch.from_numpy(x.copy()).double(), None, None, None, None, True, 0.0, P.BN_EPS)
        got = F.batch_norm(torch.from_numpy(x.copy()), None, None, None, None, True, 0.0, P.BN_EPS)
        err = ((got.double() - ref).abs().max() / max(1.0, ref.abs().max())).item()
        print(f"R={R} A={A:g}: torch fp32 CPU batch_norm err {err:.2e}")
        assert err <= 2e-6
    a, b = P.pivot_input(R, A)
    assert np.array_equal(np.sort(a, 0), np.sort(b, 0)) and (b[R // 2] == A).all() and (a[0] == A).all()


@pytest.mark.parametrize("R,C", P.FAR_SHAPES, ids=_ids(P.FAR_SHAPES))
def test_outlier_lattice_decides_the_branch_by_construction(R, C):
    """with the outlier first its columns are well past the switch and the others well short of it; moved to row R / 2 no column is past it"""
    a, b = P.outlier_lattice(R, C)
    ra, rb = P.pivot_ratio(a), P.pivot_ratio(b)
    far = np.arange(C) % 3 == 0
    print(f"{R}x{C}: dm^2/var {ra[far].min():.1f} .. {ra[far].max():.1f} (outlier first), at most {ra[~far].max():.1f} elsewhere, {rb.max():.1f} swapped")
    assert ra[far].min() > 1.5 * P.FAR_PIVOT and ra[~far].max() < P.FAR_PIVOT / 1.5 and rb.max() < P.FAR_PIVOT / 1.5
    assert np.array_equal(np.sort(a, 0), np.sort(b, 0))
    ms, qs, ns = P.part_stats(a, R, C)
    mean, var = P.exact_mean_var(a)
    assert ns.sum() == R and len(ns) == P.LAUNCH.get((R, C), P.launch(R, C))[0]
    assert _close((ns[:, None] * ms).sum(0) / R, mean, 1e-10)
    assert _close((qs + ns[:, None] * (ms - mean) ** 2).sum(0) / R, var, 1e-10)


def test_edge_input_sits_either_side_of_the_switch():
    x = P.edge_input()
    r = P.pivot_ratio(x)
    print(f"dm^2/var: even columns {r[::2].min():.2f} .. {r[::2].max():.2f}, odd columns {r[1::2].min():.2f} .. {r[1::2].max():.2f}")
    assert 22.0 < r[::2].min() and r[::2].max() < 24.0 and 27.0 < r[1::2].min() and r[1::2].max() < 29.5
