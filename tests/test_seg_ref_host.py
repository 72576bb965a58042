"""CPU: the references of tests/seg_ref.py against torch in float64 (F.log_softmax, F.nll_loss with ignore_index, index_select / index_add_),
the float32 three-NN restatement against the float64 order, the near-tie recipe, and the rounding bounds of the GPU edge tests against torch's
own float32 CPU log-softmax (a bound that a second correct float32 implementation misses would be a wrong bound)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import seg_ref as SR


def _cloud(rs, B, N, G):
    xyz = rs.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    if N < G:
        return xyz, rs.uniform(-1, 1, size=(B, G, 3)).astype(np.float32)
    return xyz, np.stack([xyz[b, rs.choice(N, G, replace=False)] for b in range(B)])        # centres are cloud points (as FPS picks them)


@pytest.mark.parametrize("B,N,G", [(2, 255, 3), (3, 257, 5), (2, 1000, 127)])
def test_three_nn_f32_agrees_with_float64_order_off_near_ties(B, N, G):
    xyz, ctr = _cloud(np.random.RandomState(N), B, N, G)
    idx, w, off, ent, d3 = SR.three_nn_f32(xyz, ctr)
    order, d = SR.three_nn_order_f64(xyz, ctr)
    k = min(4, G)
    ds = np.take_along_axis(d, order[:, :, :k], -1)
    clear = np.diff(ds, axis=-1).min(-1) > 1e-5 * (1 + ds[:, :, k - 1])
    assert clear.mean() > 0.9
    np.testing.assert_array_equal(idx[clear], order[:, :, :3][clear])
    assert idx.dtype == np.int32 and w.dtype == np.float32 and off.dtype == np.int32 and ent.dtype == np.int32
    r = 1.0 / (np.take_along_axis(d, idx.astype(np.int64), -1) + 1e-8)
    np.testing.assert_allclose(w, r / r.sum(-1, keepdims=True), rtol=1e-5, atol=1e-12)
    assert np.all(np.diff(d3, axis=-1) >= 0)
    # adjacency: a permutation of the entries, every list increasing and holding exactly the entries of its centre
    for b in range(B):
        flat = idx[b].ravel()
        assert off[b, 0] == 0 and off[b, G] == 3 * N
        assert np.array_equal(np.sort(ent[b]), np.arange(3 * N))
        for g in range(G):
            lst = ent[b, off[b, g]:off[b, g + 1]]
            assert np.all(flat[lst] == g) and np.all(np.diff(lst) > 0)


def test_three_nn_f32_ties_go_to_lower_index():
    ctr = np.array([[[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, 2], [0, -1, 0], [5, 5, 5]]], np.float32)
    xyz = np.array([[[0, 0, 0], [0, 0, 1], [5, 5, 5], [1, 0, 0]]], np.float32)
    idx, w, _, _, _ = SR.three_nn_f32(xyz, ctr)
    assert idx[0, 0].tolist() == [0, 1, 2] and idx[0, 1].tolist() == [3, 0, 1] and idx[0, 2, 0] == 5 and idx[0, 3, 0] == 0
    assert np.array_equal(w[0, 0], np.full(3, np.float32(1) / np.float32(3)))


@pytest.mark.parametrize("B,N,G,seed", SR.NEAR_TIE_CASES)
def test_near_tie_recipe_has_ties_among_the_four_nearest(B, N, G, seed):
    """the GPU test relies on this: the lattice recipe gives rows where the float32 expression, not the geometry, decides the order"""
    xyz, ctr = SR.near_tie_clouds(B, N, G, seed)
    ties = SR.rows_with_ties(xyz, ctr)
    assert ties.any()
    # the float32 selection is still an ascending one in float64, up to the rounding of the float32 distance (<= 3 * 2^-24 * d, d < 5)
    idx = SR.three_nn_f32(xyz, ctr)[0]
    d = SR.three_nn_order_f64(xyz, ctr)[1]
    d3 = np.take_along_axis(d, idx.astype(np.int64), -1)
    assert np.all(np.diff(d3, axis=-1) >= -1e-6)


def test_interp_references_vs_torch_index_ops():
    rs = np.random.RandomState(5)
    B, N, G, C = 2, 37, 7, 12
    xyz, ctr = _cloud(rs, B, N, G)
    idx, w, off, ent, _ = SR.three_nn_f32(xyz, ctr)
    P = rs.standard_normal((B * G, C)).astype(np.float32)
    dY = rs.standard_normal((B * N, C)).astype(np.float32)
    wx = rs.standard_normal((C, 3)).astype(np.float32)
    bias = rs.standard_normal(C).astype(np.float32)
    rows = torch.from_numpy(SR._rows(idx, B, N, G))
    Pt, wt = torch.from_numpy(P).double(), torch.from_numpy(w).double().reshape(B * N, 3)
    Yt = sum(wt[:, k, None] * Pt.index_select(0, rows[:, k]) for k in range(3))
    Y, A = SR.interp_fwd_f64(P, idx, w, B, N, G)
    assert np.abs(Y - Yt.numpy()).max() <= 1e-14
    At = sum((wt[:, k, None] * Pt.index_select(0, rows[:, k])).abs() for k in range(3))
    assert np.abs(A - At.numpy()).max() <= 1e-14 and np.all(A >= np.abs(Y) - 1e-14)
    Y2, A2 = SR.interp_fwd_f64(P, idx, w, B, N, G, xyz=xyz.reshape(-1, 3), wxyz=wx, bias=bias)
    Y2t = Yt + torch.from_numpy(xyz).double().reshape(-1, 3) @ torch.from_numpy(wx).double().t() + torch.from_numpy(bias).double()
    assert np.abs(Y2 - Y2t.numpy()).max() <= 1e-13 and np.all(A2 >= np.abs(Y2) - 1e-13)
    dYt = torch.from_numpy(dY).double()
    dPt = torch.zeros(B * G, C, dtype=torch.float64)
    for k in range(3):
        dPt.index_add_(0, rows[:, k], wt[:, k, None] * dYt)
    dP, Ab, L = SR.interp_bwd_f64(dY, idx, w, B, N, G)
    assert np.abs(dP - dPt.numpy()).max() <= 1e-13 and np.all(Ab >= np.abs(dP) - 1e-13)
    assert np.array_equal(L, np.diff(off, axis=1).ravel())
    # the same sum walked over the adjacency lists
    wf = w.reshape(B, 3 * N).astype(np.float64)
    for b in range(B):
        for g in range(G):
            lst = ent[b, off[b, g]:off[b, g + 1]]
            ref = (wf[b, lst, None] * dY[b * N + lst // 3].astype(np.float64)).sum(0)
            assert np.abs(dP[b * G + g] - ref).max() <= 1e-13
    dw, db, Aw, Abias = SR.xyz_grad_f64(dY, xyz.reshape(-1, 3))
    assert np.abs(dw - (dYt.t() @ torch.from_numpy(xyz).double().reshape(-1, 3)).numpy()).max() <= 1e-13
    assert np.abs(db - dYt.sum(0).numpy()).max() <= 1e-13 and np.all(Aw >= np.abs(dw) - 1e-13) and np.all(Abias >= np.abs(db) - 1e-13)


@pytest.mark.parametrize("kind", SR.KINDS)
@pytest.mark.parametrize("C", [1, 2, 13, 50, 64])
def test_log_softmax_reference_and_bounds_vs_torch(kind, C):
    for R in (1, 255, 257):
        z = SR.softmax_inputs(kind, R, C, 100 * C + R)
        out, lse = SR.log_softmax_f64(z)
        zt = torch.from_numpy(z)
        ref = F.log_softmax(zt.double(), dim=1).numpy()
        fin = np.isfinite(ref)
        assert np.array_equal(np.isneginf(out), np.isneginf(ref)) and np.array_equal(fin, ~np.isneginf(z))
        assert np.abs(out[fin] - ref[fin]).max() <= 1e-12 * max(1.0, np.abs(ref[fin]).max())
        if kind == "dominant" and C > 1:
            assert np.sort(z, axis=1)[:, -1].min() - np.sort(z, axis=1)[:, -2].max() > 104
        if C == 1:
            assert np.all(out == 0)
        # torch's float32 CPU kernel stays inside the forward bound
        t32 = F.log_softmax(zt, dim=1).numpy().astype(np.float64)
        bound = SR.log_softmax_fwd_bound(out, lse, C)
        assert np.array_equal(np.isneginf(t32), ~fin)
        assert np.all(np.abs(t32[fin] - out[fin]) <= bound[fin])
        # backward: float64 autograd, then torch's float32 backward inside the backward bound (from the same float32 log-probabilities)
        g = np.random.RandomState(C + R).standard_normal((R, C)).astype(np.float32)
        z64 = zt.double().requires_grad_(True)
        F.log_softmax(z64, dim=1).backward(torch.from_numpy(g).double())
        dz, p, sabs = SR.log_softmax_bwd_f64(out, g)
        assert np.abs(dz - z64.grad.numpy()).max() <= 1e-12 * max(1.0, sabs.max()) and np.all(np.isfinite(dz))
        lp32 = F.log_softmax(zt, dim=1)
        dz32 = torch.ops.aten._log_softmax_backward_data(torch.from_numpy(g), lp32, 1, torch.float32).numpy().astype(np.float64)
        dzr, pr, sr = SR.log_softmax_bwd_f64(lp32.numpy(), g)
        assert np.all(np.abs(dz32 - dzr) <= SR.log_softmax_bwd_bound(g, pr, sr, C))


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("R,C", [(1, 1), (257, 13), (5000, 50), (1000, 64)])
def test_nll_reference_vs_torch_ignore_index(R, C, weighted):
    rs = np.random.RandomState(R + C)
    lp = SR.log_softmax_f64((3 * rs.standard_normal((R, C))).astype(np.float32))[0].astype(np.float32)
    t = rs.randint(0, C, size=R).astype(np.int64)
    t[rs.rand(R) < 0.3] = -100                                              # torch knows one ignore value
    t[0] = 0
    wt = (0.5 + rs.rand(C)).astype(np.float32) if weighted else None
    ref = SR.nll_f64(lp, t, wt, C)
    lp64 = torch.from_numpy(lp).double().requires_grad_(True)
    loss = F.nll_loss(lp64, torch.from_numpy(t), None if wt is None else torch.from_numpy(wt).double(), ignore_index=-100)
    loss.backward()
    assert abs(ref["loss"] - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    assert ref["Anum"] >= abs(ref["num"]) and ref["Aden"] == ref["den"]
    assert ref["correct"] == int(((torch.from_numpy(lp).argmax(1) == torch.from_numpy(t)) & (torch.from_numpy(t) >= 0)).sum())
    d = SR.nll_bwd_f64(t, wt, ref["den"], 1.0, R, C)
    assert np.abs(d - lp64.grad.numpy()).max() <= 1e-15
    assert np.all(d[~ref["valid"]] == 0)
    # the other ignore values behave as -100 does
    t2 = t.copy()
    t2[t == -100] = np.array([-100, -1, C, 255])[rs.randint(0, 4, size=int((t == -100).sum()))]
    ref2 = SR.nll_f64(lp, t2, wt, C)
    assert (ref2["num"], ref2["den"], ref2["correct"]) == (ref["num"], ref["den"], ref["correct"])


def test_nll_terms_matches_the_kernel_map():
    assert SR.nll_terms(1) == 1 + 8 + 1 and SR.nll_terms(257) == 1 + 8 + 2
    assert SR.nll_terms(131072) == 1 + 8 + 512 and SR.nll_terms(131073) == 2 + 8 + 512


def test_confusion_reference_and_mixed_targets():
    rs = np.random.RandomState(9)
    R, C = 3000, 13
    pred = rs.randint(0, 4, size=(R, C)).astype(np.float32)
    t = SR.mixed_targets(rs, R, C)
    v = SR.valid_rows(t, C)
    assert 0.2 < 1 - v.mean() < 0.4 and set(np.unique(t[~v]).tolist()) == {-100, -1, C, 255}
    cm = SR.confusion_ref(pred, t, C)
    am = torch.from_numpy(pred).argmax(1).numpy()
    ref = np.zeros((C, C), np.int64)
    for r in range(R):
        if 0 <= t[r] < C:
            ref[t[r], am[r]] += 1
    assert np.array_equal(cm, ref) and cm.sum() == v.sum()
