"""CPU: the numpy references of tests/norm_rows_ref.py against torch.nn.functional / autograd in float64 (the cosine loss on a zero row, a row of
norm 1e-10 and rows of elements 1e-6 as well: the definition is pinned to the installed torch), the properties of the lattice inputs that
tests/test_gpu_norm_rows_edges.py relies on, and the launch partitions its shapes were chosen for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import norm_rows_ref as N

T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
L64 = lambda a: torch.from_numpy(np.array(a, dtype=np.int64))
_ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]


def _close(a, ref, tol=1e-12):
    return N.rel(np.asarray(a), np.asarray(ref)) <= tol


# ---- the restatements --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,D", [(1, 4), (5, 260), (17, 516), (33, 64)])
def test_layernorm_against_autograd(T, D):
    x, pos, dy, dres = N.ln_real(T, D)
    g, b = N.ln_params(D)
    xin = x + pos
    xd, gd, bd = T64(xin).requires_grad_(True), T64(g).requires_grad_(True), T64(b).requires_grad_(True)
    yr = F.layer_norm(xd, (D,), gd, bd, N.LN_EPS)
    (yr * T64(dy)).sum().backward()
    y, mean, rstd = N.layernorm_fwd(xin, g, b)
    assert _close(y, yr.detach().numpy())
    assert _close(mean, xd.detach().mean(1).numpy()) and _close(rstd, (xd.detach().var(1, unbiased=False) + N.LN_EPS).rsqrt().numpy())
    dx, dg, db = N.layernorm_bwd(dy, xin, g, mean, rstd, dres)
    assert _close(dx, (xd.grad + T64(dres)).numpy()) and _close(dg, gd.grad.numpy()) and _close(db, bd.grad.numpy())
    assert _close(N.layernorm_bwd(dy, xin, g, mean, rstd)[0], xd.grad.numpy())
    assert _close(N.colsum(dy), T64(dy).sum(0).numpy())


@pytest.mark.parametrize("R,C", N.XENT_SHAPES, ids=_ids(N.XENT_SHAPES))
def test_cross_entropy_against_torch(R, C):
    z, lab = N.xent_input(R, C)
    z = z.copy()
    z[0] = 0.25                                                                           # an all-equal row: index 0
    if R > 1 and C > 2:
        z[R - 1, [1, C - 1]] = 50.0                                                       # a tie: the lower index
    zd = T64(z).requires_grad_(True)
    ref = F.cross_entropy(zd, L64(lab))
    (2.5 * ref).backward()
    loss, lse, top1, dz = N.xent(z, lab, 2.5)
    assert _close(loss, ref.item()) and _close(lse, torch.logsumexp(zd.detach(), 1).numpy()) and _close(dz, zd.grad.numpy(), 1e-14)
    first = np.array([int(np.flatnonzero(row == row.max())[0]) for row in z])             # the lowest index attaining the maximum, spelled out
    assert top1 == float((first == lab).sum()) / R and first[0] == 0 and (R == 1 or C <= 2 or first[R - 1] == 1)


def test_cross_entropy_with_infinite_logits():
    z, lab = (a.copy() for a in N.xent_input(9, 65))
    off = np.ones(65, bool)
    off[[3, 64]] = False                                                                  # classes 3 and 64 do not exist
    lab[lab == 3] = 4; lab[lab == 64] = 5
    zi = z.copy(); zi[:, ~off] = -np.inf
    zd = T64(zi).requires_grad_(True)
    ref = F.cross_entropy(zd, L64(lab)); ref.backward()
    loss, _, _, dz = N.xent(zi, lab)
    assert _close(loss, ref.item()) and _close(dz, zd.grad.numpy()) and (dz[:, ~off] == 0).all()
    remap = np.cumsum(off) - 1
    assert _close(loss, N.xent(z[:, off], remap[lab])[0])                                 # the same loss as the row without those classes
    zi[2, lab[2]] = -np.inf                                                               # -inf on the label
    assert N.xent(zi, lab)[0] == np.inf == F.cross_entropy(T64(zi), L64(lab)).item()
    big = 1e4 * np.resize(np.array([-1.0, 0.0, 1.0], np.float32), (5, 63))
    bl = np.array([0, 1, 2, 61, 62])
    bd = T64(big).requires_grad_(True)
    ref = F.cross_entropy(bd, L64(bl)); ref.backward()
    loss, _, _, dz = N.xent(big, bl)
    assert np.isfinite(loss) and _close(loss, ref.item()) and _close(dz, bd.grad.numpy())


@pytest.mark.parametrize("kind", [0, 1])
def test_regression_losses_against_torch(kind):
    r = np.random.default_rng(5)
    s, t = (2 * r.standard_normal((7, 63))).astype(np.float32), r.standard_normal((7, 63)).astype(np.float32)
    s[0, :len(N.KNEE)] = np.array(N.KNEE, np.float32); t[0] = 0
    assert np.array_equal(s[0, :len(N.KNEE)].astype(np.float64), np.array(N.KNEE))       # the knee values are float32 numbers
    sd = T64(s).requires_grad_(True)
    ref = F.mse_loss(sd, T64(t)) if kind == 0 else F.smooth_l1_loss(sd, T64(t))
    (3.0 * ref).backward()
    loss, ds = N.regression(s, t, kind, 3.0)
    assert _close(loss, ref.item()) and _close(ds, sd.grad.numpy(), 1e-15)


def _torch_cosine(s, t, g):
    sd = T64(s).requires_grad_(True)
    cos = F.cosine_similarity(sd, T64(t), dim=-1, eps=N.COS_EPS)
    (g * (1 - cos).mean()).backward()
    return (1 - cos).detach().numpy(), sd.grad.numpy()


def test_cosine_is_the_installed_torchs_definition():
    s, t, names = N.cos_clamp_input()
    row, ds = _torch_cosine(s, t, 3.0)
    loss, row_ref, ds_ref = N.cosine(s, t, g=3.0)
    assert _close(row_ref, row) and _close(ds_ref, ds, 1e-14) and _close(loss, row.mean())
    assert row_ref[1] == 1.0 and row_ref[2] == 1.0 and row_ref[3] == 1.0 and (ds_ref[3] == 0).all() and (ds_ref[2] == 0).all()
    tn = np.linalg.norm(t[1].astype(np.float64))
    assert _close(ds_ref[1], -3.0 / len(s) * t[1] / (tn * N.COS_EPS), 1e-14)              # a zero student row: -g / R t / (|t| eps)
    for a, b in ((s, t), (t, s)):                                                         # every norm: 0, or a factor of 100 from eps
        n = np.linalg.norm(a.astype(np.float64), axis=1)
        assert ((n == 0) | (n >= 100 * N.COS_EPS) | (n <= 1.0001 * N.COS_EPS / 100)).all(), n      # (1e-10, rounded to float32 elements)
    # rows of elements ~1e-6 (norms ~1e-5): the separate clamps leave the true cosine, the product clamp does not
    r = np.random.default_rng(3)
    s6, t6 = (1e-6 * r.standard_normal((4, 384))).astype(np.float32), (1e-6 * r.standard_normal((4, 384))).astype(np.float32)
    row6, ds6 = _torch_cosine(s6, t6, 1.0)
    _, row6_ref, ds6_ref = N.cosine(s6, t6)
    true = 1 - (s6.astype(np.float64) * t6).sum(1) / (np.linalg.norm(s6.astype(np.float64), axis=1) * np.linalg.norm(t6.astype(np.float64), axis=1))
    assert _close(row6_ref, row6) and _close(ds6_ref, ds6, 1e-14) and _close(row6_ref, true)
    assert np.abs((1 - N.cosine_product_clamp(s6, t6)) - true).max() > 1e-3
    # ordinary rows: both definitions agree
    so, to = N.cos_input(5, 63)
    rowo, dso = _torch_cosine(so, to, 1.0)
    assert _close(N.cosine(so, to)[1], rowo) and _close(N.cosine(so, to)[2], dso, 1e-14) and _close(1 - N.cosine_product_clamp(so, to), rowo)


def test_row_gate_add_and_prompt_rows_against_torch():
    r = np.random.default_rng(11)
    x = r.standard_normal((12, 8)).astype(np.float32); gate = np.array([0.0, 1.0 / (1 - 0.1), 1.0, 1.25], np.float32)
    ref = (torch.from_numpy(x).view(-1, 3, 8) * torch.from_numpy(gate).view(-1, 1, 1)).view(12, 8)
    assert np.array_equal(N.scale_rows(x, gate, 3), ref.numpy()) and N.scale_rows(x, gate, 3).dtype == np.float32
    assert np.array_equal(N.add(x, x[::-1]), (torch.from_numpy(x) + torch.from_numpy(x[::-1].copy())).numpy())
    B, P, D = 5, 3, 8
    tok, ppos = r.standard_normal((P, D)), r.standard_normal((P, D))
    mask = (r.random((B * P, D)) < 0.5).astype(np.float64); dy = r.standard_normal((B * P, D))
    td, pd = T64(tok).requires_grad_(True), T64(ppos).requires_grad_(True)
    y = (td.expand(B, P, D) * T64(mask).view(B, P, D) * 2.0 + pd.expand(B, P, D)).reshape(B * P, D)
    (y * T64(dy)).sum().backward()
    assert _close(N.prompt_rows_fwd(tok, ppos, mask, B, 2.0), y.detach().numpy())
    dtok, dppos = N.prompt_rows_bwd(dy, mask, B, P, 2.0)
    assert _close(dtok, td.grad.numpy()) and _close(dppos, pd.grad.numpy())
    dyi = r.integers(-2, 3, (B * P, D)).astype(np.float32)
    ti, pi = N.prompt_rows_bwd(dyi, mask.astype(np.float32), B, P, 2.0)
    assert ti.dtype == np.int64 and np.array_equal(ti, (dyi.astype(np.float64) * mask * 2).reshape(B, P, D).sum(0)) and np.array_equal(pi, dyi.reshape(B, P, D).sum(0))


# ---- the lattices ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M", N.FAR_MEAN, ids=[f"{d}@{int(m)}" for d, m in N.FAR_MEAN])
def test_far_mean_lattice_tells_the_two_pass_form_from_the_one_pass_form(D, M):
    x = N.far_mean_rows(N.FAR_T, D, M)
    g, b = N.ln_params(D)
    k = (x.astype(np.float64) - M) * 8
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max() <= 32 and (k.sum(1) == 0).all()
    assert abs(M) * D + 4 * D <= 2 ** 21                                                  # every partial sum: a multiple of 1/8 below 2^24 / 8
    for order in (np.arange(D), np.random.default_rng(D).permutation(D)):                 # ... so float32 adds a row exactly, in any order
        assert np.array_equal(np.cumsum(x[:, order], axis=1, dtype=np.float32).astype(np.float64), np.cumsum(x[:, order].astype(np.float64), axis=1))
    assert (x.sum(1, dtype=np.float32) / np.float32(D) == np.float32(M)).all()
    y, mean, _ = N.layernorm_fwd(x, g, b)
    assert (mean == M).all()
    two, one = N.rel(N.layernorm_y32(x, g, b, N.LN_EPS, False), y), N.rel(N.layernorm_y32(x, g, b, N.LN_EPS, True), y)
    print(f"D = {D}, M = {M}: float32 two-pass {two:.2e}, one-pass {one:.2e}")
    assert two <= 2e-5 < one


@pytest.mark.parametrize("T", list(N.LN_EXACT_T))
def test_layernorm_backward_lattice_sums_are_exact_in_float32(T):
    D = N.LN_EXACT_D
    xin, dy, mean, rstd, gamma = N.ln_bwd_lattice(T, D)
    assert np.abs(xin - mean[:, None]).max() <= 4 and np.abs(dy).max() <= 2 and (rstd == 0.5).all()
    assert (np.abs(dy) * np.abs(xin - mean[:, None])).sum(0).max() + 2 ** 20 < 2 ** 24    # units of 1/2, with room for an accumulated base
    _, dg, db = N.layernorm_bwd(dy, xin, gamma, mean, rstd)
    ig, ib = N.ln_bwd_lattice_sums(T, D)
    assert np.array_equal(dg, ig) and np.array_equal(db, ib)
    assert np.array_equal(dg.astype(np.float32).astype(np.float64), dg)


def test_the_other_lattices_are_exact_in_float32():
    for R, C in N.COLSUM_SHAPES:
        x = N.colsum_lattice(R, C)
        assert np.array_equal(x, np.rint(x)) and (R == 0 or np.abs(x).max() <= 8) and 8 * R + 2 ** 20 < 2 ** 24
        assert np.array_equal(N.colsum(x), x.astype(np.int64).sum(0))
    B, P, D = N.PROMPT
    assert B * P * D // 4 > N.GRID_CAP and (B - 1) * P * D // 4 <= N.GRID_CAP and 2 * 2 * B < 2 ** 24 and B * P * D * 4 < 35e6


# ---- the partitions ----------------------------------------------------------------------------------------------------------------------------
def test_layernorm_backward_partitions():
    assert N.ln_bwd_blocks(16411) == (20, 821, 11)                                        # rows_per_block grows past 16; a last workgroup of 11 rows
    assert N.ln_bwd_blocks(16384) == (16, 1024, 16) and N.ln_bwd_blocks(16385) == (20, 820, 5)
    assert N.LN_BWD_BIG[0] == 16411
    for T, nblk in N.LN_EXACT_T.items():
        assert N.ln_bwd_blocks(T)[:2] == (16, nblk), T
    assert sorted(N.LN_EXACT_T.values()) == [1, 2, 5, 33, 820]
    assert [N.ln_bwd_blocks(T) for T in N.LN_BWD_T] == [(16, 1, 1), (16, 1, 15), (16, 1, 16), (16, 2, 1), (16, 3, 1)]
    assert N.ln_bwd_workspace_floats(16411, 64) == 821 * 64 * 2
    # ACT_LN_BWD_RPB: below 4 it is ignored, otherwise rounded up to a multiple of 4 and a floor
    assert N.ln_bwd_blocks(100, 32) == (32, 4, 4) and N.ln_bwd_blocks(100, 4) == (4, 25, 4) and N.ln_bwd_blocks(100, 8) == (8, 13, 4)
    assert N.ln_bwd_blocks(33, 4) == (4, 9, 1) and N.ln_bwd_blocks(100, 3) == N.ln_bwd_blocks(100) and N.ln_bwd_blocks(100, 5) == (8, 13, 4)
    assert N.ln_bwd_blocks(16411, 4) == (20, 821, 11)


def test_colsum_partitions():
    for (R, C), row in N.COLSUM.items():
        assert N.colsum_parts(R, C) == row, (R, C)
        assert N.colsum_workspace_floats(R, C) == row[0] * C >= row[2] * C
    assert N.colsum_parts(32800, 8)[0] == 1024 < (32800 + 31) // 32                       # the cap binds
    assert N.colsum_parts(32768, 8)[2] == 1024                                            # ... and here 1,024 parts are launched
    # stage 1 per row-lane (rows r0 + ry, step 4): the 8-deep loop runs while r + 28 < r1
    assert N.COLSUM[(100, 64)][1] < 32 <= N.COLSUM[(1000, 130)][1] and N.COLSUM[(32800, 8)][1] == 36
    assert N.COLSUM[(1000, 130)][3] == 8
    for T, D, rps in N.SCALE_ROWS[-1:]:
        assert T * D // 4 > N.GRID_CAP and T % rps == 0
    assert N.ADD_N[-1] // 4 > N.GRID_CAP and N.REG_SHAPES[-1][0] * N.REG_SHAPES[-1][1] > N.GRID_CAP
    assert [(R + 1023) // 1024 for R, _ in N.XENT_SHAPES[-2:]] == [2, 3]                  # mean_kernel's per
