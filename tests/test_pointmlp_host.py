"""CPU: the restatements of tests/pointmlp_ref.py against plain torch -- the yardsticks the GPU tests of tests/test_gpu_pointmlp.py measure with."""
import pytest
import torch

from tests import pointmlp_ref as P

GROUPER_SHAPES = [(1, 2, 1, 2, 1), (3, 70, 33, 24, 67), (2, 40, 5, 40, 130), (2, 9, 4, 3, 8)]


@pytest.mark.parametrize("B,N,S,k,D", GROUPER_SHAPES)
def test_grouper_restatement_equals_the_plain_composition(B, N, S, k, D):
    c = P.grouper_case(B, N, S, k, D)
    mine, sigma = P.geo_affine(c["feat"], c["fps"], c["idx"], c["alpha"], c["beta"], cat=True)
    plain = P.geo_affine_plain(c["feat"], c["fps"], c["idx"], c["alpha"], c["beta"])
    assert mine.shape == (B, S, k, 2 * D) and sigma.shape == (B,)
    assert P.rel(mine, plain) < 1e-13                      # e * (1 / s) against e / s: two float64 roundings
    assert torch.equal(mine[..., D:], plain[..., D:])


@pytest.mark.parametrize("hub", [False, True])
@pytest.mark.parametrize("B,N,S,k,D", GROUPER_SHAPES)
def test_analytic_grouper_backward_equals_float64_autograd(B, N, S, k, D, hub):
    c = P.grouper_case(B, N, S, k, D, seed=1, hub=hub)
    for cat in (False, True):
        want = P.grouper_run(c, torch.float64, cat)
        dfeat, dalpha, dbeta = P.geo_affine_backward(c["feat"], c["fps"], c["idx"], c["alpha"], c["g"], c["h"] if cat else None)
        assert P.rel(dfeat, want["dfeat"]) < 1e-12 and P.rel(dalpha, want["dalpha"]) < 1e-12 and P.rel(dbeta, want["dbeta"]) < 1e-12


def test_hub_case_has_a_hub_unlisted_points_and_repeats():
    c = P.grouper_case(2, 40, 12, 6, 8, seed=1, hub=True)
    idx = c["idx"]
    assert bool((idx[:, :, 0] == 0).all()) and int(idx.max()) < 20 and bool((idx[:, :, 1] == idx[:, :, 2]).all())
    assert all(len(set(row.tolist())) == row.numel() for row in c["fps"])


@pytest.mark.parametrize("variant", ["pointmlp", "elite"])
@pytest.mark.parametrize("tiny", [False, True])
def test_network_restatement_has_the_keys_and_shapes_of_the_layer_table(variant, tiny):
    cfg = P.config(variant, **(P.TINY if tiny else {}))
    table = P.layer_table(cfg, 40)
    sd = P.Model(40, **cfg).state_dict()
    assert sorted(sd) == sorted(table)
    assert all(tuple(sd[n].shape) == tuple(table[n]) for n in table)
    if not tiny:                                           # the published sizes: 13.2 M (pointmlp) and 0.72 M (elite) parameters
        count = sum(v.numel() for n, v in sd.items() if "running" not in n and "tracked" not in n)
        assert abs(count / (13.24e6 if variant == "pointmlp" else 0.717e6) - 1) < 0.02, count


@pytest.mark.parametrize("R,C", P.TAIL_TRAIN_ROWS)
def test_tail_cases_keep_every_pre_activation_clear_of_zero(R, C):
    c = P.tail_train_case(R, C)
    z = P.tail_run(c, torch.float64)["z"]
    assert float(z.abs().min()) >= P.MARGIN


@pytest.mark.parametrize("R,C", P.TAIL_EVAL_ROWS)
def test_tail_exact_cases_are_exact_in_float32(R, C):
    c = P.tail_exact_case(R, C)
    a = P.tail(c["y"], c["res"], c["gamma"], c["beta"], c["rm"], c["rv"], False, eps=0.0)[0]
    b = P.tail(*(c[n].float() for n in ("y", "res", "gamma", "beta", "rm", "rv")), False, eps=0.0)[0]
    assert torch.equal(a, b.double())


@pytest.mark.parametrize("variant", ["pointmlp", "elite"])
def test_tiny_network_float32_restatement_stays_close_to_float64(variant):
    model, _ = P.tiny_net(variant)
    pts, masks, cot = P.tiny_inputs(variant)
    draws = dict(masks)
    want = P.net_run(model, pts, draws, cot, torch.float64)
    assert all(f"fps.{i}" in draws and f"knn.{i}" in draws for i in range(1, 5))
    f32 = P.net_run(model, pts, draws, cot, torch.float32)
    errs = {n: P.rel(f32[n], want[n]) for n in want}
    worst = max(errs, key=errs.get)
    assert errs[worst] < 2.5e-5, (worst, errs[worst])
    assert all(float(want[n].abs().max()) > 0 for n in want)
