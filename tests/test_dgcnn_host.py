"""CPU: the numpy references of tests/dgcnn_ref.py against torch float64 autograd, the case tables of tests/test_gpu_dgcnn_edges.py against the
dispatch rules of csrc/dgcnn.hip (every path name is reached, every boundary is hit on both sides), and the margins that let the GPU backward
comparison run without exclusions."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dgcnn_ref as R
from tests import test_gpu_dgcnn_edges as E

T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _close(a, ref, tol=1e-12):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() <= tol * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("B,G,k,C,groups,graph", [(2, 7, 3, 12, 3, True), (3, 5, 4, 16, 4, True), (2, 9, 1, 8, 2, False)])
def test_edge_tail_references_against_autograd(B, G, k, C, groups, graph):
    rng = np.random.default_rng(G * 10 + C)
    zoff = C if graph else -1
    yz = rng.standard_normal((B * G, 2 * C if graph else C))
    idx = R.graph(rng, B, G, k) if graph else None
    gamma = R.gammas(rng, C, groups, zero=False).astype(np.float64); beta = 0.1 * rng.standard_normal(C); dout = rng.standard_normal((B * G, C))
    assert (gamma < 0).any() and (gamma > 0).any()
    yd, wd, bd = T(yz).requires_grad_(True), T(gamma).requires_grad_(True), T(beta).requires_grad_(True)
    y = yd[:, :C].reshape(B, G, C)
    pre = y[torch.arange(B).view(B, 1, 1), torch.from_numpy(idx)] if graph else y.unsqueeze(1)
    if graph:
        pre = pre + yd[:, C:].reshape(B, 1, G, C)
    pre = pre.permute(0, 3, 2, 1)                                                              # [B, C, G, k]: the reference formulation
    ref = F.leaky_relu(F.group_norm(pre, groups, wd, bd, R.EPS), R.SLOPE).max(dim=-1)[0].transpose(1, 2).reshape(B * G, C)
    (ref * T(dout)).sum().backward()
    out, mean, rstd = R.edge_tail(yz, zoff, idx, B, G, k, C, groups, gamma, beta)
    dyz, dg, db = R.edge_tail_bwd(yz, zoff, idx, B, G, k, C, groups, gamma, beta, dout)
    assert _close(out, ref.detach().numpy()) and _close(dyz, yd.grad.numpy()) and _close(dg, wd.grad.numpy()) and _close(db, bd.grad.numpy())
    x5 = pre.detach().numpy().reshape(B, groups, -1)
    assert _close(mean, x5.mean(-1)) and _close(rstd, 1 / np.sqrt(x5.var(-1) + R.EPS), 1e-10)


def test_tokenizer_references_against_autograd():
    rng = np.random.default_rng(3)
    B, G, C, tau = 2, 3, 20, 0.7
    logits, noise, dy = (rng.standard_normal((B, G, C)) for _ in range(3))
    ld = T(logits).requires_grad_(True)
    yr = F.softmax((ld + T(noise)) / tau, dim=-1)
    (yr * T(dy)).sum().backward()
    y = R.gumbel_softmax(logits, noise, tau)
    assert _close(y, yr.detach().numpy()) and _close(R.gumbel_softmax_bwd(y, dy, tau), ld.grad.numpy())
    ld2 = T(logits).requires_grad_(True)
    lq = torch.log(F.softmax(ld2, dim=-1).mean(dim=1))
    lu = torch.log(torch.tensor([1.0 / C], dtype=torch.float64)).expand(B, C)
    ref = F.kl_div(lq, lu, None, None, "batchmean", log_target=True)
    (ref * 1.7).backward()
    assert abs(R.kl_uniform(logits) - ref.item()) <= 1e-12 and _close(R.kl_uniform_bwd(logits, 1.7), ld2.grad.numpy())
    h = rng.standard_normal((B * G, C)); gamma = rng.standard_normal(C); beta = rng.standard_normal(C); cb = rng.standard_normal((C, 4))
    lg, index, codes, gap, _, _ = R.gumbel_argmax_gather(h, B, G, C, 4, gamma, beta, noise, tau, cb)
    lr = F.leaky_relu(F.group_norm(T(h).view(B, G, C).transpose(1, 2), 4, T(gamma), T(beta), R.EPS), R.SLOPE).transpose(1, 2).reshape(B * G, C)
    assert _close(lg, lr.numpy()) and np.array_equal(index, ((lr + T(noise).view(B * G, C)) / tau).argmax(-1).numpy())
    assert np.array_equal(codes, cb[index]) and (gap > 0).all()


def test_case_tables_reach_every_forward_path_and_boundary():
    fp = lambda c: R.forward_path(c["G"], c["k"], c["C"], c["groups"], c["ldy"], c["zoff"], c["idx"])
    for c in E.FORWARD + [c for c in E.FAR if c["path"] != "token"]:
        assert fp(c) == c["path"], c
    assert {c["path"] for c in E.FORWARD} == {"fused", "slab", "generic", "head"}
    have = {(c["path"], c["G"], c["k"], c["C"], c["groups"]) for c in E.FORWARD}
    # either side of the 140 KB rule, of G = 512 for the slab form, of GN_SPLIT slabs per group, of cpg % 4; one, two and eight slabs per group
    for case in [("fused", 271, 4, 256, 4), ("slab", 272, 4, 256, 4), ("slab", 512, 4, 1024, 4), ("generic", 513, 4, 1024, 4), ("generic", 513, 4, 256, 4),
                 ("slab", 64, 4, 128, 4), ("generic", 64, 4, 288, 1), ("generic", 20, 4, 24, 4), ("generic", 600, 3, 256, 4), ("generic", 7, 2, 12, 3)]:
        assert case in have, case
    assert (2 * 271 * 64 + 4 * 271) * 4 == 143088 <= 140 * 1024 < (2 * 272 * 64 + 4 * 272) * 4
    assert (512 * 32 + 4 * 512) * 4 == 72 * 1024 < (513 * 32 + 4 * 513) * 4
    assert {c["C"] // c["groups"] // 32 for c in E.FORWARD if c["path"] == "slab"} == {1, 2, 8} and 288 // 32 == R.GN_SPLIT + 1
    assert any(c["G"] % 8 for c in E.FORWARD if c["path"] == "slab") and any(c["G"] % 8 == 0 for c in E.FORWARD if c["path"] == "slab")
    assert any(c["k"] * c["G"] > 1024 for c in E.FORWARD if c["path"] == "fused")                # second trip of the index staging
    assert any(c["G"] * c["k"] * c["C"] // c["groups"] < 256 for c in E.FORWARD if c["path"] == "generic")
    for path in ("generic", "head"):                                                          # second trip of the 8192-block grid-stride loops
        assert any(c["B"] * c["G"] * c["C"] > 8192 * 256 for c in E.FORWARD if c["path"] == path)
    assert max(c["B"] * c["G"] * c["ldy"] * 4 for c in E.FORWARD) <= 22 * 2 ** 20
    for path in ("fused", "slab", "generic", "head", "token"):                                # far pivots: every form at cpg = 64, cpg = 4 where it exists
        cpgs = {c["C"] // c["groups"] for c in E.FAR if c["path"] == path}
        assert 64 in cpgs and (4 in cpgs or path == "slab"), (path, cpgs)
    assert {c["path"] for c in E.SWITCH} == {"fused", "slab", "generic", "head", "token"}


def test_case_tables_reach_every_backward_path_and_boundary():
    bp = lambda c: R.backward_path(c["G"], c["k"], c["idx"])
    for c in E.BACKWARD + E.TIES + [E.REFUSED]:
        assert bp(c) == c["path"], c
    assert {bp(c) for c in E.BACKWARD} | {bp(E.REFUSED)} == {"lds16", "lds32", "gl4", "gl2", "gl1", "head", "refused"}
    graphs = {(c["G"], c["k"]) for c in E.BACKWARD if c["idx"]} | {(E.REFUSED["G"], E.REFUSED["k"])}
    for lo, hi, k in [(64, 65, 4), (128, 129, 4), (256, 257, 4), (512, 513, None)]:            # either side of every G boundary
        assert any(g == lo and (k is None or kk == k) for g, kk in graphs) and any(g == hi and (k is None or kk == k) for g, kk in graphs), (lo, hi)
    assert any(c["k"] != 4 and c["G"] <= 128 for c in E.BACKWARD if c["idx"]) and any(c["k"] == 1 and c["idx"] for c in E.BACKWARD)
    for kind in ("hub", "same"):
        paths = {c["path"][:2] for c in E.BACKWARD if c["graph"] == kind}
        assert paths == {"ld", "gl"}, (kind, paths)
    assert {c["path"][:2] for c in E.BACKWARD if c["plant"]} == {"ld", "gl"}
    assert {R.backward_path(c["G"], c["k"], True, lds=False) for c in E.TIES if c["G"] <= 128} == {"gl4"}


@pytest.mark.parametrize("c", E.BACKWARD + [E.REFUSED], ids=E._id)
def test_backward_inputs_keep_every_decision_clear(c):
    """with its committed seed every backward case keeps |y| >= 1e-4 at every selected pre-activation and 1e-4 between the best and the second-best
    neighbour of another source row: no admissible forward error flips a LeakyReLU side or an arg-max, so the GPU comparison excludes nothing"""
    B, G, k, C, groups = E._geom(c)
    yz, idx, gamma, beta, dout = R.backward_inputs(c)
    ymin, gap = R.margins(yz, C if c["idx"] else -1, idx, B, G, k, C, groups, gamma, beta)
    print(f"{E._id(c)}: min |y| {ymin:.2e}, min gap {gap:.2e}")
    assert ymin >= 1e-4 and gap >= 1e-4 and (gamma != 0).all() and (gamma < 0).any()
    if c["graph"] == "hub":
        assert R.unnamed_rows(idx, G)[0].sum() >= 3 and (idx[0] == 3).sum() == (k - 1) * G + 1
    if c["graph"] == "same":
        assert (idx[:, :, 2] == 7).all()
    if c["plant"]:
        assert (R.pivot_ratio(yz, C, idx, B, G, k, C, groups) > 10 * R.FAR_PIVOT).all()                  # far past the switch (a small group dilutes d = 300)


@pytest.mark.parametrize("c", E.TIES, ids=E._id)
def test_tie_inputs_are_exact_and_clear_of_zero(c):
    B, G, k, C, groups = E._geom(c)
    yz, idx, gamma, beta, dout = R.tie_inputs(c)
    assert (yz[:, :C] * 8 == np.round(yz[:, :C] * 8)).all() and (yz[:, C:] == np.round(yz[:, C:])).all() and (dout == np.round(dout)).all()
    assert set(np.abs(gamma)) <= {1.0, 2.0} and (gamma < 0).any() and (beta * 2 % 2 == 1).all()
    ymin, gap = R.margins(yz, C, idx, B, G, k, C, groups, gamma, beta)
    print(f"{E._id(c)}: min |y| {ymin:.2e}, min gap between different sources {gap:.2e}")
    assert ymin >= 1e-4 and gap == 0.0                                                         # ties between different sources exist; no y is near 0


@pytest.mark.parametrize("c", [c for c in E.FAR if c["path"] == "token"], ids=E._id)
def test_tokenizer_far_pivot_rows_left_out(c):
    """fewer than 1 % of the rows have their two best float64 scores within 1e-4 of each other, at every planting"""
    B, G, k, C, groups = E._geom(c)
    noise, cb = E.token_noise_and_codebook(c)
    assert np.isfinite(noise).all()
    for kind, where in E.PLANTINGS:
        for d in E.FAR_D + E.SWITCH_D:
            h, _, gamma, beta = E._far_inputs(c, kind, where, d)
            gap = R.gumbel_argmax_gather(h, B, G, C, groups, gamma, beta, noise, 1.0, cb)[3]
            assert (gap <= 1e-4).mean() < 0.01, (kind, where, d)


@pytest.mark.parametrize("c", E.SWITCH, ids=E._id)
def test_switch_cases_sit_on_their_side(c):
    B, G, k, C, groups = E._geom(c)
    for d, past in zip(E.SWITCH_D, (False, True)):
        yz, idx, _, _ = E._far_inputs(c, "element", "first", d)
        ratio = R.pivot_ratio(yz, c["zoff"], idx, B, G, k, C, groups)
        assert (ratio > R.FAR_PIVOT * 1.02).all() if past else (ratio < R.FAR_PIVOT * 0.98).all(), (d, ratio)
