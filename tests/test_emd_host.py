"""Host: the numpy restatement of the Earth Mover's Distance tests (tests/emd_ref.py) against scipy, and the parts of extensions/emd,
utils/metrics and the synthetic recipe that need no GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import emd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(seed):
    """odd seeds: integer lattices (ties, exact sums); even seeds: real-valued clouds"""
    rs = np.random.RandomState(seed)
    n = int(rs.randint(1, 65))
    if seed % 2:
        return rs.randint(0, 16, (n, 3)).astype(np.float32), rs.randint(0, 16, (n, 3)).astype(np.float32)
    return rs.standard_normal((n, 3)).astype(np.float32), rs.standard_normal((n, 3)).astype(np.float32)


def test_sqdist_is_the_float32_chain():
    x1, x2 = _problem(2)
    d = R.sqdist(x1, x2)
    assert d.dtype == np.float32 and d.shape == (x1.shape[0], x2.shape[0])
    i, j = 3 % x1.shape[0], 5 % x2.shape[0]
    dx, dy, dz = (np.float32(x1[i, k]) - np.float32(x2[j, k]) for k in range(3))
    assert d[i, j] == np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz))


@pytest.mark.parametrize("seed", range(10))
def test_emd_optimum_agrees_with_scipy(seed):
    opt = pytest.importorskip("scipy.optimize")
    x1, x2 = _problem(seed)
    c = R.sqdist(x1, x2).astype(np.float64)
    rows, cols = opt.linear_sum_assignment(c)
    want = c[rows, cols].sum()
    got, a = R.emd_assignment(x1, x2)
    assert sorted(a.tolist()) == list(range(x1.shape[0]))
    assert got == c[np.arange(len(a)), a].sum()
    # two optimal matchings may differ and their float64 sums with them, by rounding alone: n terms of at most ~50, each within 2^-53 relative
    assert abs(got - want) <= 1e-12 * max(want, 1.0)
    if seed % 2:
        assert got == want                                            # integer costs: every sum is exact
    assert R.emd_optimum(x1, x2) == got


def test_the_extension_refuses_cpu_tensors():
    from act_amd.extensions.emd import EarthMoverDistance, emd, emd_cuda, emdModule
    assert emd is emdModule
    x = torch.zeros(2, 8, 3)
    with pytest.raises(RuntimeError):
        emd()(x, x)
    with pytest.raises(RuntimeError):
        EarthMoverDistance()(x, x)
    with pytest.raises(RuntimeError):
        emd_cuda.forward(x, x)
    with pytest.raises(RuntimeError):
        emd_cuda.backward(x, x, torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, 8))


def test_unequal_counts_raise_value_error_naming_both():
    from act_amd.extensions.emd import emd, max_points
    with pytest.raises(ValueError, match=r"\b48\b.*\b64\b"):
        emd()(torch.zeros(1, 48, 3), torch.zeros(1, 64, 3))
    assert max_points() >= 2048
    n = max_points() + 1
    with pytest.raises(ValueError, match=str(n)):
        emd()(torch.zeros(1, n, 3), torch.zeros(1, n, 3))


def test_eps_and_max_rounds_are_checked_before_anything_is_launched():
    """(the tensors pass the device check by claiming to be CUDA tensors)"""
    from act_amd.extensions import emd as E

    class Fake(torch.Tensor):
        is_cuda = True
    x = torch.zeros(1, 4, 3).as_subclass(Fake)
    for kw in (dict(eps=0.0), dict(eps=float("inf")), dict(eps=float("nan")), dict(max_rounds=0)):
        with pytest.raises(ValueError):
            E.emd_cuda.forward(x, x, **kw)


def test_emd_distance_refuses_a_prediction_smaller_than_the_ground_truth():
    from act_amd.utils.metrics import emd_distance
    with pytest.raises(ValueError, match=r"\b32\b.*\b64\b"):
        emd_distance(torch.zeros(1, 32, 3), torch.zeros(1, 64, 3))


def test_the_emd_recipe_parses():
    from act_amd.utils.config import cfg_from_yaml_file
    cwd = os.getcwd()
    os.chdir(os.path.join(ROOT, "act_amd"))
    try:
        cfg = cfg_from_yaml_file("cfgs/synthetic/act_dvae_emd_val.yaml")
        base = cfg_from_yaml_file("cfgs/synthetic/act_dvae_with_pretrained_transformer.yaml")
    finally:
        os.chdir(cwd)
    assert cfg.emd_val and isinstance(cfg.emd_val, dict) and cfg.emd_val.eps == 1e-5
    assert cfg.model.NAME == "ACTPromptedDiscreteVAEwithVIT" and cfg.consider_metric == "CDL1"
    assert not base.get("emd_val", None)
    rest = {k: v for k, v in cfg.items() if k != "emd_val"}
    assert rest == dict(base)                                         # the Stage-I recipe, plus the key


def test_metrics_names_are_unchanged_with_the_module_imported():
    import act_amd.extensions.emd  # noqa: F401
    from act_amd.utils import metrics
    assert metrics.Metrics.names() == ['F-Score', 'CDL1', 'CDL2'] and len(metrics.Metrics.ITEMS) == 3
    assert callable(metrics.emd_distance)


def test_the_runner_does_not_import_the_extension():
    code = ("import sys, act_amd.tools.runner_autoencoder, act_amd.utils.metrics; "
            "assert 'act_amd.extensions.emd' not in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def test_aggregate_emd_is_the_macro_average():
    from act_amd.tools.runner_autoencoder import aggregate_emd
    rows = np.array([[1.0, 10], [3.0, 12], [10.0, -7], [5.0, 3]])
    agg = aggregate_emd(rows, ["a", "a", "b", "a"])
    assert agg["per_taxonomy"] == {"a": 3.0, "b": 10.0} and agg["overall"] == 6.5 and agg["capped"] == 1
    assert agg["values"].tolist() == [1.0, 3.0, 10.0, 5.0] and agg["info"].tolist() == [10, 12, -7, 3]
