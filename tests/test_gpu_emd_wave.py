"""GPU: the one-wave-per-pair Earth Mover's Distance (csrc/emd.hip emd_wave_kernel, ``solver="wave"`` of extensions/emd) and the Stage-I loss
built on it (model key ``emd_loss``), against the numpy restatement of tests/emd_wave_ref.py and the Hungarian optimum of tests/emd_ref.py.

Bars.  There is no tolerance in this file except the two the auction itself states.
  * Every output (assignment, dist, info, eps_used) EQUALS the restatement's: the kernel and the restatement round every cost, value, bid and
    eps in the same order, and every choice (bidder, object, tie) is by lowest index.
  * Lattices (integer coordinates, eps_final = 2^-10, eps_rel = 0, N * eps < 1): nothing is rounded, so sum(dist) == optimum.
  * Real values: optimum (1 - 1e-9) <= sum(dist) <= optimum + N * eps_used in float64, the guarantee itself.
  * dist is bit-equal to the float32 cost chain of emd_ref.sqdist gathered by the returned assignment, and the assignment a permutation, in
    every case."""
import argparse
import copy

import numpy as np
import pytest
import torch

from tests import emd_ref as R
from tests import emd_wave_ref as W
from tests.golden.fill import TINY_DVAE, TINY_STAGE2, fill_module

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS_LATTICE = 2.0 ** -10
EPS, EPS_REL = 1e-12, 2.0 ** -18
SIZES = [1, 2, 3, 31, 32, 33, 63, 64]


def _E():
    from act_amd.extensions import emd as E
    return E


def _solve(x1, x2, eps, eps_rel=0.0, max_bids=100000):
    """-> dist, assignment, info, eps_used as numpy"""
    out = _E().emd_cuda.forward(torch.from_numpy(x1).to(DEV), torch.from_numpy(x2).to(DEV), eps, max_bids, solver="wave", eps_rel=eps_rel,
                                want_eps=True)
    assert len(out) == 4
    return [t.cpu().numpy() for t in out]


def _check_consistent(x1, x2, dist, assignment):
    B, N = assignment.shape
    assert dist.dtype == np.float32 and assignment.dtype == np.int32 and dist.shape == (B, N)
    for b in range(B):
        assert np.array_equal(np.sort(assignment[b]), np.arange(N)), b
        assert np.array_equal(dist[b], R.sqdist(x1[b], x2[b])[np.arange(N), assignment[b]], equal_nan=True), b


def _check_equals_restatement(got, x1, x2, eps, eps_rel=0.0, max_bids=100000):
    dist, assignment, info, eps_used = got
    a, d, i, e = W.solve_batch(x1, x2, eps, eps_rel, max_bids)
    assert np.array_equal(info, i), (info, i)
    assert np.array_equal(eps_used.view(np.int32), e.view(np.int32))
    assert np.array_equal(assignment, a)
    assert np.array_equal(dist.view(np.int32), d.view(np.int32))


def _patches(rs, B, N, scales):
    """group patches around a non-zero centre; pair b has the spread scales[b % len(scales)]"""
    s = np.asarray(scales, dtype=np.float64)[np.arange(B) % len(scales)][:, None, None]
    c = rs.uniform(-0.5, 0.5, (B, 1, 3))
    return (c + s * rs.standard_normal((B, N, 3))).astype(np.float32), (c + s * rs.standard_normal((B, N, 3))).astype(np.float32)


def _sphere(rs, B, N, scale=1.0):
    x = rs.standard_normal((B, N, 3))
    return (scale * x / np.linalg.norm(x, axis=2, keepdims=True)).astype(np.float32)


# ---- lattices and ties --------------------------------------------------------------------------------------------------------------------
def _check_exact(x1, x2):
    got = _solve(x1, x2, EPS_LATTICE)
    dist, assignment, info, eps_used = got
    N = x1.shape[1]
    assert (info >= N).all() and (eps_used == np.float32(EPS_LATTICE)).all()
    _check_consistent(x1, x2, dist, assignment)
    for b in range(x1.shape[0]):
        opt, s = R.emd_optimum(x1[b], x2[b]), float(dist[b].astype(np.float64).sum())
        print(f"N = {N} pair {b}: bids {info[b]}, sum(dist) {s}, optimum {opt}")
        assert s == opt, (b, s, opt)
    _check_equals_restatement(got, x1, x2, EPS_LATTICE)


@pytest.mark.parametrize("N", SIZES)
def test_exact_on_lattices(N):
    rs = np.random.RandomState(2000 + N)
    assert N * EPS_LATTICE < 1
    _check_exact(rs.randint(0, 16, (3, N, 3)).astype(np.float32), rs.randint(0, 16, (3, N, 3)).astype(np.float32))


def test_ties_everywhere():
    """coordinates in {0, 1}^3 at N = 64: eight distinct points, every value tied many times over"""
    rs = np.random.RandomState(7)
    _check_exact(rs.randint(0, 2, (3, 64, 3)).astype(np.float32), rs.randint(0, 2, (3, 64, 3)).astype(np.float32))


# ---- real values --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [32, 64])
def test_bound_and_restatement_on_real_valued_patches(N):
    rs = np.random.RandomState(5000 + N)
    x1, x2 = _patches(rs, 64, N, (0.05, 0.2, 1.0))
    got = _solve(x1, x2, EPS, EPS_REL)
    dist, assignment, info, eps_used = got
    assert (info >= N).all()
    _check_consistent(x1, x2, dist, assignment)
    worst = 0.0
    for b in range(64):
        opt, s = R.emd_optimum(x1[b], x2[b]), float(dist[b].astype(np.float64).sum())
        worst = max(worst, (s - opt) / (N * float(eps_used[b])))
        assert opt - 1e-9 * opt <= s <= opt + N * float(eps_used[b]), (b, s, opt, eps_used[b])
    print(f"N = {N}: bids median {np.median(info)}, max {info.max()}; largest (sum(dist) - optimum) / (N * eps_used) = {worst:.3f}")
    _check_equals_restatement(got, x1, x2, EPS, EPS_REL)


# ---- batch independence -------------------------------------------------------------------------------------------------------------------
def test_deterministic_and_independent_of_the_batch():
    """B = 257 at N = 32: 65 workgroups of four waves, the last with one pair"""
    rs = np.random.RandomState(9)
    x1, x2 = _patches(rs, 257, 32, (0.05, 0.2, 1.0))
    a, b = _solve(x1, x2, EPS, EPS_REL), _solve(x1, x2, EPS, EPS_REL)
    assert all(np.array_equal(p.view(np.int32), q.view(np.int32)) for p, q in zip(a, b))
    _check_consistent(x1, x2, a[0], a[1])
    assert (a[2] >= 32).all()
    for i in (0, 3, 4, 255, 256):
        alone = _solve(x1[i:i + 1], x2[i:i + 1], EPS, EPS_REL)
        assert all(np.array_equal(p[i:i + 1].view(np.int32), q.view(np.int32)) for p, q in zip(a, alone)), i
    for B in (1, 3, 4, 5):
        part = _solve(x1[:B], x2[:B], EPS, EPS_REL)
        assert all(np.array_equal(p[:B].view(np.int32), q.view(np.int32)) for p, q in zip(a, part)), B
    empty = _E().emd_cuda.forward(torch.zeros(0, 32, 3, device=DEV), torch.zeros(0, 32, 3, device=DEV), EPS, solver="wave", eps_rel=EPS_REL)
    assert [tuple(t.shape) for t in empty] == [(0, 32), (0, 32), (0,)]


# ---- the cap ------------------------------------------------------------------------------------------------------------------------------
def test_the_bid_cap_still_returns_a_bijection():
    rs = np.random.RandomState(13)
    x1, x2 = _sphere(rs, 1, 64), _sphere(rs, 1, 64, 0.9)
    full = _solve(x1, x2, 1e-5)
    assert full[2][0] > 100
    got = _solve(x1, x2, 1e-5, max_bids=5)
    assert got[2][0] == -5
    _check_consistent(x1, x2, got[0], got[1])
    assert (np.diff(got[1][0][5:]) > 0).all()                       # only bidders 0 .. 4 can hold an object after five bids; the rest: ascending
    _check_equals_restatement(got, x1, x2, 1e-5, max_bids=5)       # the fill order
    # one bid short of the full solve: capped; exactly enough: not
    n = int(full[2][0])
    assert _solve(x1, x2, 1e-5, max_bids=n)[2][0] == n and _solve(x1, x2, 1e-5, max_bids=n - 1)[2][0] == -(n - 1)


def test_all_points_equal():
    x = np.full((2, 32, 3), 0.25, dtype=np.float32)
    dist, assignment, info, eps_used = _solve(x, x, EPS, EPS_REL)
    assert (info == 32).all() and (dist == 0).all() and (eps_used == np.float32(EPS)).all()
    _check_consistent(x, x, dist, assignment)


def test_a_nan_coordinate_ends_at_the_cap():
    """the termination guarantee: with a NaN among the coordinates no bid is ever settled, and max_bids ends the solve"""
    rs = np.random.RandomState(17)
    x1, x2 = _patches(rs, 1, 32, (0.2,))
    x1[0, 3, 1] = np.nan
    dist, assignment, info, _ = _solve(x1, x2, EPS, EPS_REL, max_bids=200)
    assert info[0] < 0
    assert np.array_equal(np.sort(assignment[0]), np.arange(32))


# ---- surface ------------------------------------------------------------------------------------------------------------------------------
def test_surface_and_the_default_solver_is_unchanged():
    E = _E()
    rs = np.random.RandomState(19)
    big = torch.zeros(1, 65, 3, device=DEV)
    with pytest.raises(ValueError, match=r"\b64\b"):
        E.emd_cuda.forward(big, big, solver="wave")
    x1, x2 = (torch.from_numpy(t).to(DEV) for t in _patches(rs, 5, 32, (0.2, 1.0)))
    for bad in (-1e-6, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            E.emd_cuda.forward(x1, x2, solver="wave", eps_rel=bad)
    with pytest.raises(ValueError):
        E.emd_cuda.forward(x1, x2, eps_rel=1e-6)
    with pytest.raises(ValueError):
        E.emd_cuda.forward(x1, x2, solver="wave", want_evals=True)
    with pytest.raises(ValueError):
        E.emd_cuda.forward(x1, x2, solver="lane")
    plain, named = E.emd_cuda.forward(x1, x2), E.emd_cuda.forward(x1, x2, solver="workgroup")
    assert len(plain) == 3 and all(torch.equal(p, q) for p, q in zip(plain, named))
    pos = E.emd_cuda.forward(x1, x2, E.DEFAULT_EPS, E.DEFAULT_MAX_ROUNDS, True)
    assert len(pos) == 4 and all(torch.equal(p, q) for p, q in zip(plain, pos)) and pos[3].dtype == torch.int64
    # the two solvers answer the same question: both within N * eps of each other's sum
    wave = E.emd_cuda.forward(x1, x2, E.DEFAULT_EPS, solver="wave")
    assert (wave[2] > 0).all() and ((wave[0].double().sum(1) - plain[0].double().sum(1)).abs() <= 32 * E.DEFAULT_EPS).all()
    # the C entry refuses what the Python surface refuses
    from act_amd import _C
    dist, asg, info = (torch.empty_like(t) for t in plain)
    call = lambda n, eps, rel, cap: _C.lib.act_emd_wave_fwd_f32(_C.ptr(x1), _C.ptr(x2), 5, n, eps, rel, cap, _C.ptr(dist), _C.ptr(asg), _C.ptr(info),
                                                               None, _C.stream())
    assert _C.lib.act_emd_wave_max_points() == 64 == E.wave_max_points()
    bad = [call(65, 1e-5, 0.0, 10), call(0, 1e-5, 0.0, 10), call(32, 0.0, 0.0, 10), call(32, float("inf"), 0.0, 10), call(32, 1e-5, -1.0, 10),
           call(32, 1e-5, float("inf"), 10), call(32, 1e-5, float("nan"), 10), call(32, 1e-5, 0.0, 0)]
    assert len(set(bad)) == 1 and bad[0] != 0
    assert _C.lib.act_emd_wave_fwd_f32(None, None, 0, 32, 1e-5, 0.0, 10, None, None, None, None, _C.stream()) == 0       # B == 0: a no-op
    assert _C.lib.act_emd_wave_fwd_f32(None, _C.ptr(x2), 5, 32, 1e-5, 0.0, 10, _C.ptr(dist), _C.ptr(asg), _C.ptr(info), None, _C.stream()) \
        not in (0, bad[0])


# ---- backward -----------------------------------------------------------------------------------------------------------------------------
def test_backward_of_the_wave_solver_is_the_existing_kernel_bit_for_bit():
    E = _E()
    rs = np.random.RandomState(23)
    h1, h2 = _patches(rs, 6, 32, (0.05, 1.0))
    x1, x2 = torch.from_numpy(h1).to(DEV).requires_grad_(True), torch.from_numpy(h2).to(DEV).requires_grad_(True)
    mod = E.EarthMoverDistance(eps=EPS, solver="wave", eps_rel=EPS_REL)
    loss = mod(x1, x2)
    dist, assignment, info = E.emd_cuda.forward(x1.detach(), x2.detach(), EPS, solver="wave", eps_rel=EPS_REL)
    assert torch.equal(mod.last_info, info) and (info > 0).all()
    assert loss.dim() == 0 and torch.equal(loss.detach(), torch.mean(torch.sqrt(dist)))
    loss.backward()
    d = dist.clone().requires_grad_(True)
    torch.sqrt(d).mean().backward()
    gx1, gx2 = E.emd_cuda.backward(x1.detach(), x2.detach(), assignment, d.grad)
    assert torch.equal(x1.grad, gx1) and torch.equal(x2.grad, gx2) and torch.isfinite(gx1).all() and (gx1 != 0).any()


# ---- model --------------------------------------------------------------------------------------------------------------------------------
def _tiny_dvae(**kw):
    from act_amd.models.dvae import DiscreteVAE
    from act_amd.utils.config import EasyDict
    torch.manual_seed(0)
    return fill_module(DiscreteVAE(EasyDict(dict(TINY_DVAE, num_group=4, group_size=8, **kw))), "emdloss.").to(DEV).train()


def _manual_chamfer(model, ret):
    _, _, coarse, fine, group_gt, _ = ret
    bg = coarse.shape[0] * coarse.shape[1]
    c, f, g = (t.reshape(bg, -1, 3).contiguous() for t in (coarse, fine, group_gt))
    return model.loss_func_cdl1(c, g) + model.loss_func_cdl1(f, g), f, g


def test_model_loss_with_and_without_the_key():
    E = _E()
    rs = np.random.RandomState(29)
    pts = torch.from_numpy(_sphere(rs, 2, 64) * rs.uniform(0.2, 1.0, (2, 64, 1)).astype(np.float32)).to(DEV)
    model = _tiny_dvae(emd_loss=dict(weight=0.5))
    ret = model(pts, temperature=1.0, hard=False)
    loss = model.recon_loss(ret, pts)
    base, f, g = _manual_chamfer(model, ret)
    dist, assignment, info = E.emd_cuda.forward(f.detach(), g.detach(), 1e-12, 100000, solver="wave", eps_rel=2.0 ** -18)
    assert dist.shape == (8, 8) and torch.equal(model.emd_last_info, info) and model.emd_last_info.is_cuda and (info > 0).all()
    assert torch.equal(loss.detach(), (base + 0.5 * torch.mean(torch.sqrt(dist))).detach())
    assert model.emd_capped.is_cuda and model.emd_capped.dtype == torch.int64 and int(model.emd_capped) == 0
    # the gradient of the extra term reaches fine (ret[3]) and not coarse (ret[2]): the Chamfer kernels are bit-reproducible, so the
    # gradients of the loss and of the manual Chamfer sum differ by that term alone
    gc, gf = torch.autograd.grad(loss, [ret[2], ret[3]], retain_graph=True)
    bc, bf = torch.autograd.grad(base, [ret[2], ret[3]], retain_graph=True)
    assert torch.equal(gc, bc)
    d = dist.clone().requires_grad_(True)
    (0.5 * torch.sqrt(d).mean()).backward()
    extra = E.emd_cuda.backward(f.detach(), g.detach(), assignment, d.grad)[0].reshape(ret[3].shape)
    assert torch.isfinite(extra).all() and (extra != 0).any() and torch.equal(gf, bf + extra)
    # a cap of one bid: every pair is capped, and the counter accumulates over calls without a host read in between
    capped = _tiny_dvae(emd_loss=dict(max_bids=1))
    with torch.no_grad():
        r = capped(pts, temperature=1.0, hard=False)
        capped.recon_loss(r, pts); capped.recon_loss(r, pts)
    assert int(capped.emd_capped) == 16 and (capped.emd_last_info == -1).all()
    # without the key: the loss of before, and the extension is not touched
    plain = _tiny_dvae()
    ret0 = plain(pts, temperature=1.0, hard=False)
    assert plain.emd_loss is None and torch.equal(plain.recon_loss(ret0, pts), _manual_chamfer(plain, ret0)[0])
    assert not hasattr(plain, "emd_capped")


# ---- runner -------------------------------------------------------------------------------------------------------------------------------
def test_two_training_steps_of_the_emd_loss_recipe(tmp_path):
    from act_amd.tools import runner_autoencoder as RA
    from act_amd.utils.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file("cfgs/synthetic/act_dvae_emd_loss.yaml")
    assert cfg.model.emd_loss is True and cfg.model.NAME == "ACTPromptedDiscreteVAEwithVIT"
    cfg.model.update(copy.deepcopy(TINY_STAGE2["dvae_config"]))                  # the 2-layer teacher; NAME and emd_loss stay the recipe's
    assert cfg.model.emd_loss is True and cfg.model.visual_embed_depth == 2
    for split in cfg.dataset.values():
        split._base_.update(NUM_SAMPLES=8)
        split.others.update(bs=2, npoints=128)
    cfg.total_bs = 2
    args = argparse.Namespace(log_name="test_emd_loss", use_gpu=True, local_rank=0, distributed=False, sync_bn=False, resume=False,
                              start_ckpts=None, experiment_path=str(tmp_path), num_workers=0, world_size=1, val_freq=1)
    seen = []
    real = RA.train_step

    def step(base_model, *a, **k):
        out = real(base_model, *a, **k)
        seen.append((base_model.module.emd_last_info, base_model.module.emd_capped))
        return out
    RA.train_step, keep = step, RA.train_step
    try:
        torch.manual_seed(0)
        log = RA.run_net(args, cfg, max_steps=2, log_every=1)
    finally:
        RA.train_step = keep
    assert len(log) == 2 and np.isfinite(log).all() and all(l1 > 0 for l1, _ in log)
    assert len(seen) == 2 and seen[0][0].shape == (2 * 16,) and (seen[1][0] > 0).all() and int(seen[1][1]) == 0
