"""Host: the numpy restatement of the one-wave-per-pair auction (tests/emd_wave_ref.py) against the Hungarian optimum of tests/emd_ref.py, and
the parts of the wave solver's surface that need no GPU: argument checks of extensions/emd, the ``emd_loss`` model key, the recipe.

Bars.  Lattices (integer coordinates in [0,16)^3, eps_final = 2^-10, eps_rel = 0, N * eps < 1): every cost is an integer and every eps, bid and
price a multiple of 2^-10 below 2^14, so nothing is rounded and sum(dist) <= optimum + N * eps < optimum + 1 makes the integer sum EQUAL to
the optimum.  Real values: the auction's own guarantee, sum(dist) <= optimum + N * eps_used, in float64 over the float32 costs."""
import os

import numpy as np
import pytest
import torch

from tests import emd_ref as R
from tests import emd_wave_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 31, 32, 33, 63, 64]
EPS_LATTICE = 2.0 ** -10


def _lattice(N, B=3):
    rs = np.random.RandomState(2000 + N)
    return rs.randint(0, 16, (B, N, 3)).astype(np.float32), rs.randint(0, 16, (B, N, 3)).astype(np.float32)


def _patches(rs, B, N, scale):
    """group patches: points around a non-zero centre, spread ``scale``"""
    c = rs.uniform(-0.5, 0.5, (B, 1, 3))
    return (c + scale * rs.standard_normal((B, N, 3))).astype(np.float32), (c + scale * rs.standard_normal((B, N, 3))).astype(np.float32)


def _is_bijection(a, N):
    return a.dtype == np.int32 and np.array_equal(np.sort(a), np.arange(N))


@pytest.mark.parametrize("N", SIZES)
def test_exact_on_lattices(N):
    assert N * EPS_LATTICE < 1
    x1, x2 = _lattice(N)
    for b in range(x1.shape[0]):
        a, dist, info, eps_used = W.solve(x1[b], x2[b], EPS_LATTICE)
        assert _is_bijection(a, N) and info >= N and eps_used == np.float32(EPS_LATTICE)
        assert dist.dtype == np.float32 and np.array_equal(dist, R.sqdist(x1[b], x2[b])[np.arange(N), a])
        assert float(dist.astype(np.float64).sum()) == R.emd_optimum(x1[b], x2[b]), (N, b, info)


@pytest.mark.parametrize("N", SIZES)
def test_bound_on_random_patches(N):
    rs = np.random.RandomState(3000 + N)
    for scale in (0.05, 1.0):
        x1, x2 = _patches(rs, 2, N, scale)
        for b in range(2):
            a, dist, info, eps_used = W.solve(x1[b], x2[b], 1e-12, 2.0 ** -18)
            d = R.sqdist(x1[b], x2[b])
            assert _is_bijection(a, N) and info >= N
            assert eps_used == max(np.float32(1e-12), np.float32(np.float32(2.0 ** -18) * d.max()))
            got, opt = float(dist.astype(np.float64).sum()), R.emd_optimum(x1[b], x2[b])
            assert opt - 1e-9 * opt <= got <= opt + N * float(eps_used), (N, scale, b, got, opt)


def test_the_cap_hands_out_the_free_objects_in_ascending_order():
    rs = np.random.RandomState(13)
    x1, x2 = _patches(rs, 1, 64, 1.0)
    x1, x2 = x1[0], x2[0]
    _, _, full, _ = W.solve(x1, x2, 1e-5)
    assert full > 100
    a, dist, info, _ = W.solve(x1, x2, 1e-5, max_bids=5)
    assert info == -5 and _is_bijection(a, 64)
    # the bidder is always the lowest unassigned one, so after five bids only bidders 0 .. 4 can hold an object: everybody from 5 on (and
    # whoever of 0 .. 4 was evicted) takes the free objects in ascending order
    d = R.sqdist(x1, x2)
    assert np.array_equal(dist, d[np.arange(64), a])
    assert (np.diff(a[5:]) > 0).all()
    # a cap that is not met changes nothing
    assert W.solve(x1, x2, 1e-5, max_bids=full)[2] == full and W.solve(x1, x2, 1e-5, max_bids=full - 1)[2] == -(full - 1)


def test_all_points_equal_take_one_bid_each():
    x = np.full((32, 3), 0.25, dtype=np.float32)
    a, dist, info, eps_used = W.solve(x, x, 1e-12, 2.0 ** -18)
    assert info == 32 and np.array_equal(a, np.arange(32)) and (dist == 0).all() and eps_used == np.float32(1e-12)


def test_a_nan_coordinate_ends_at_the_cap():
    rs = np.random.RandomState(17)
    x1, x2 = _patches(rs, 1, 32, 0.2)
    x1[0, 3, 1] = np.nan
    a, _, info, _ = W.solve(x1[0], x2[0], 1e-12, 2.0 ** -18, max_bids=200)
    assert info == -200 and _is_bijection(a, 32)


# ---- surface ----------------------------------------------------------------------------------------------------------------------------
class _Fake(torch.Tensor):
    is_cuda = True               # passes the device check: everything below is refused before anything is launched


def test_solver_arguments_are_checked_before_anything_is_launched():
    from act_amd.extensions import emd as E
    assert E.wave_max_points() == 64 and E.max_points() >= 2048
    x = torch.zeros(1, 32, 3).as_subclass(_Fake)
    big = torch.zeros(1, 65, 3).as_subclass(_Fake)
    with pytest.raises(ValueError, match=r"\b64\b"):
        E.emd_cuda.forward(big, big, solver="wave")
    with pytest.raises(ValueError, match="want_evals"):
        E.emd_cuda.forward(x, x, solver="wave", want_evals=True)
    with pytest.raises(ValueError, match="solver"):
        E.emd_cuda.forward(x, x, solver="jacobi")
    with pytest.raises(ValueError, match="eps_rel"):
        E.emd_cuda.forward(x, x, eps_rel=1e-6)                        # the workgroup solver takes no relative eps
    with pytest.raises(ValueError, match="eps_rel"):
        E.emd_cuda.forward(x, x, solver="workgroup", eps_rel=1e-6)
    for bad in (-1e-6, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="eps_rel"):
            E.emd_cuda.forward(x, x, solver="wave", eps_rel=bad)
        with pytest.raises(ValueError, match="eps_rel"):
            E.emdModule(solver="wave", eps_rel=bad)
    with pytest.raises(ValueError, match="solver"):
        E.EarthMoverDistance(solver="simd")
    m = E.EarthMoverDistance(solver="wave", eps_rel=2.0 ** -18)
    assert m.solver == "wave" and m.eps_rel == 2.0 ** -18 and m.eps == E.DEFAULT_EPS
    d = E.emd()
    assert d.solver == "workgroup" and d.eps_rel == 0.0              # the default never depends on N


def _tiny(**kw):
    from act_amd.utils.config import EasyDict
    from tests.golden.fill import TINY_DVAE
    return EasyDict(dict(TINY_DVAE, **kw))


def test_the_emd_loss_key_is_parsed_at_construction():
    from act_amd.models.dvae import DiscreteVAE, EMD_LOSS_DEFAULTS
    assert EMD_LOSS_DEFAULTS == dict(weight=1.0, eps=1.0e-12, eps_rel=3.814697265625e-06, max_bids=100000) and 2.0 ** -18 == 3.814697265625e-06
    for off in (_tiny(), _tiny(emd_loss=False), _tiny(emd_loss=None)):
        m = DiscreteVAE(off)
        assert m.emd_loss is None and not hasattr(m, "emd_capped") and not hasattr(m, "emd_last_info")
    keys = set(DiscreteVAE(_tiny()).state_dict())
    m = DiscreteVAE(_tiny(emd_loss=True))
    assert m.emd_loss == EMD_LOSS_DEFAULTS and m.emd_last_info is None
    assert m.emd_capped.dtype == torch.int64 and m.emd_capped.dim() == 0 and int(m.emd_capped) == 0
    assert set(m.state_dict()) == keys                                # the checkpoint keeps the reference's keys
    m = DiscreteVAE(_tiny(emd_loss=dict(weight=0.5, max_bids=2000)))
    assert m.emd_loss == dict(weight=0.5, eps=1.0e-12, eps_rel=2.0 ** -18, max_bids=2000)
    m = DiscreteVAE(_tiny(emd_loss=dict(weight=2, eps=1e-9, eps_rel=0, max_bids=7)))
    assert m.emd_loss == dict(weight=2.0, eps=1e-9, eps_rel=0.0, max_bids=7)
    assert DiscreteVAE(_tiny(group_size=64, emd_loss=True)).emd_loss is not None
    with pytest.raises(ValueError, match=r"\b68\b.*\b64\b"):
        DiscreteVAE(_tiny(group_size=68, emd_loss=True))
    DiscreteVAE(_tiny(group_size=68))                                 # without the key the limit does not apply
    with pytest.raises(ValueError, match="wieght"):
        DiscreteVAE(_tiny(emd_loss=dict(wieght=1.0)))


def test_the_emd_loss_recipe_is_the_stage1_recipe_plus_the_keys():
    from act_amd.utils.config import cfg_from_yaml_file
    cwd = os.getcwd()
    os.chdir(os.path.join(ROOT, "act_amd"))
    try:
        cfg = cfg_from_yaml_file("cfgs/synthetic/act_dvae_emd_loss.yaml")
        base = cfg_from_yaml_file("cfgs/synthetic/act_dvae_with_pretrained_transformer.yaml")
    finally:
        os.chdir(cwd)
    assert cfg.model.emd_loss is True and cfg.emd_val is True
    assert "emd_loss" not in base.model and not base.get("emd_val", None)
    rest = {k: v for k, v in cfg.items() if k != "emd_val"}
    rest["model"] = {k: v for k, v in cfg.model.items() if k != "emd_loss"}
    assert rest == dict(base)
