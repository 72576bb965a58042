"""GPU: the Earth Mover's Distance (csrc/emd.hip, extensions/emd, utils/metrics.emd_distance, runner_autoencoder.evaluate with ``emd_val``)
against the exact assignment optimum of tests/emd_ref.py (numpy Hungarian) and, at N = 1024 and 2048, of tests/golden/g24_emd.npz (scipy).

Bars.  There is no tolerance in this file.
  * Lattices (integer coordinates, eps_final = 2^-10, N * eps_final < 1): every cost is an integer, every eps of the ladder is 2^-10 times a
    power of two and every price and bid a multiple of 2^-10 below 2^14, so the auction runs without a single rounding and its guarantee
    sum(dist) <= optimum + N * eps_final < optimum + 1 makes the integer sum(dist) EQUAL to the optimum.
  * Real-valued clouds: optimum (1 - 1e-9) <= sum(dist) <= optimum + N * eps_final in float64, the guarantee itself.
  * dist is bit-equal to the float32 cost chain of emd_ref.sqdist gathered by the returned assignment; the backward is bit-equal to torch's
    evaluation of the same expression."""
import numpy as np
import pytest
import torch

from tests import emd_ref as R
from tests.conftest import golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS_LATTICE = 2.0 ** -10


def _E():
    from act_amd.extensions import emd as E
    return E


def _solve(x1, x2, eps, max_rounds=None, **kw):
    E = _E()
    out = E.emd_cuda.forward(torch.from_numpy(x1).to(DEV), torch.from_numpy(x2).to(DEV), eps, E.DEFAULT_MAX_ROUNDS if max_rounds is None else max_rounds,
                             **kw)
    return [t.cpu().numpy() for t in out]


def _check_consistent(x1, x2, dist, assignment):
    """assignment is a permutation and dist the float32 cost chain gathered by it, bit for bit"""
    B, N = assignment.shape
    assert dist.dtype == np.float32 and assignment.dtype == np.int32
    for b in range(B):
        assert np.array_equal(np.sort(assignment[b]), np.arange(N)), b
        assert np.array_equal(dist[b], R.sqdist(x1[b], x2[b])[np.arange(N), assignment[b]]), b


def _check_exact(x1, x2, eps):
    dist, assignment, info = _solve(x1, x2, eps)
    assert (info > 0).all(), info
    _check_consistent(x1, x2, dist, assignment)
    for b in range(x1.shape[0]):
        opt = R.emd_optimum(x1[b], x2[b])
        got = float(dist[b].astype(np.float64).sum())
        print(f"N = {x1.shape[1]} cloud {b}: rounds {info[b]}, sum(dist) {got}, optimum {opt}")
        assert got == opt, (b, got, opt)
    return info


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 256, 257, 511])
def test_exact_on_lattices(N):
    """the wave edges, one odd size beyond a tile and the largest N with N * 2^-10 < 1"""
    rs = np.random.RandomState(1000 + N)
    x1 = rs.randint(0, 16, (3, N, 3)).astype(np.float32)
    x2 = rs.randint(0, 16, (3, N, 3)).astype(np.float32)
    assert N * EPS_LATTICE < 1
    _check_exact(x1, x2, EPS_LATTICE)


def test_ties_everywhere():
    """coordinates in {0, 1}^3: eight distinct points, massive duplicates -- a price war or a wrong tie rule shows here"""
    rs = np.random.RandomState(7)
    x1 = rs.randint(0, 2, (3, 64, 3)).astype(np.float32)
    x2 = rs.randint(0, 2, (3, 64, 3)).astype(np.float32)
    _check_exact(x1, x2, EPS_LATTICE)


def test_known_matching():
    """xyz2 = xyz1[perm] with distinct lattice points: every other matching costs at least 2 > N * eps_final, so the inverse permutation is the
    only admissible answer"""
    rs = np.random.RandomState(11)
    B, N = 2, 300
    x1 = np.stack([np.stack(np.unravel_index(rs.choice(16 ** 3, N, replace=False), (16, 16, 16)), axis=1) for _ in range(B)]).astype(np.float32)
    perm = np.stack([rs.permutation(N) for _ in range(B)])
    x2 = np.stack([x1[b][perm[b]] for b in range(B)])
    dist, assignment, info = _solve(x1, x2, EPS_LATTICE)
    assert (info > 0).all() and (dist == 0).all()
    assert np.array_equal(assignment, np.argsort(perm, axis=1))


def _sphere(rs, B, N, scale=1.0):
    x = rs.standard_normal((B, N, 3))
    return (scale * x / np.linalg.norm(x, axis=2, keepdims=True)).astype(np.float32)


def _check_bound(x1, x2, optimum, eps):
    dist, assignment, info = _solve(x1, x2, eps)
    assert (info > 0).all(), info
    _check_consistent(x1, x2, dist, assignment)
    N = x1.shape[1]
    for b in range(x1.shape[0]):
        got, opt = float(dist[b].astype(np.float64).sum()), float(optimum[b])
        print(f"N = {N} cloud {b}: rounds {info[b]}, sum(dist) - optimum = {got - opt:.3e}, N * eps = {N * eps:.3e}")
        assert got <= opt + N * eps, (b, got, opt)
        assert got >= opt - 1e-9 * opt, (b, got, opt)               # nothing beats the optimum


def test_bound_on_real_valued_clouds():
    rs = np.random.RandomState(5)
    x1, x2 = _sphere(rs, 4, 256), _sphere(rs, 4, 256, 0.9)
    _check_bound(x1, x2, [R.emd_optimum(x1[b], x2[b]) for b in range(4)], _E().DEFAULT_EPS)


@pytest.mark.parametrize("N", [1024, 2048])
def test_bound_on_the_golden_problems(N):
    g = golden("g24_emd")
    _check_bound(g[f"x1_{N}"], g[f"x2_{N}"], g[f"opt_{N}"], _E().DEFAULT_EPS)


def test_deterministic_and_independent_of_the_batch():
    rs = np.random.RandomState(9)
    x1, x2 = _sphere(rs, 3, 257), _sphere(rs, 3, 257, 0.9)
    a, b = _solve(x1, x2, 1e-5, want_evals=True), _solve(x1, x2, 1e-5, want_evals=True)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert (a[3] >= a[2]).all() and (a[3] <= a[2].astype(np.int64) * 257).all()          # bids: between one and N per round
    for i in range(3):
        alone = _solve(x1[i:i + 1], x2[i:i + 1], 1e-5, want_evals=True)
        assert all(np.array_equal(p[i:i + 1], q) for p, q in zip(a, alone)), i


def test_the_round_cap_still_returns_a_bijection():
    """max_rounds = 1 on a problem that needs hundreds of rounds: the exit path, info < 0, the rest handed out in ascending order"""
    rs = np.random.RandomState(13)
    x1, x2 = _sphere(rs, 2, 64), _sphere(rs, 2, 64, 0.9)
    _, _, full = _solve(x1, x2, 1e-5)
    assert (full > 100).all(), full
    dist, assignment, info = _solve(x1, x2, 1e-5, max_rounds=1)
    assert (info == -1).all(), info
    _check_consistent(x1, x2, dist, assignment)
    # one Jacobi round from zero prices: bidder i wants its nearest object (lowest index on ties), the lowest bidder among equal bids gets it ...
    for b in range(2):
        d = R.sqdist(x1[b], x2[b])
        want = np.argmin(d, axis=1)
        kept = assignment[b] == want
        assert kept.sum() == len(set(want.tolist()))                 # ... exactly one winner per object that was bid on
        rest_i, rest_j = np.nonzero(~kept)[0], np.sort(assignment[b][~kept])
        assert np.array_equal(assignment[b][rest_i], rest_j)         # the others: free objects in ascending order
    dist7, assignment7, info7 = _solve(x1, x2, 1e-5, max_rounds=7)
    assert (info7 == -7).all()
    _check_consistent(x1, x2, dist7, assignment7)


def test_backward_is_torchs_expression_bit_for_bit():
    E = _E()
    rs = np.random.RandomState(17)
    x1 = torch.from_numpy(_sphere(rs, 2, 65)).to(DEV)
    x2 = torch.from_numpy(_sphere(rs, 2, 65, 0.9)).to(DEV)
    g = torch.from_numpy(rs.standard_normal((2, 65)).astype(np.float32)).to(DEV)
    _, assignment, _ = E.emd_cuda.forward(x1, x2)
    gx1, gx2 = E.emd_cuda.backward(x1, x2, assignment, g)
    idx = assignment.long()[..., None].expand(-1, -1, 3)
    want1 = (2 * (x1 - x2.gather(1, idx))) * g[..., None]
    assert torch.equal(gx1, want1)
    assert torch.equal(gx2, torch.zeros_like(x2).scatter_(1, idx, -want1))
    # through autograd: dist's gradient is the kernel's, the assignment has none
    a1, a2 = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
    mod = E.emd()
    dist, asg = mod(a1, a2)
    assert not asg.requires_grad and torch.equal(asg, assignment) and mod.last_info.is_cuda and mod.last_info.dtype == torch.int32
    (dist * g).sum().backward()
    assert torch.equal(a1.grad, gx1) and torch.equal(a2.grad, gx2)
    # the historical call shape: positional eps, iters
    dist_h, asg_h = mod(x1, x2, 1e-5, 1000000)
    assert torch.equal(dist_h, dist.detach()) and torch.equal(asg_h, asg)


def test_earth_mover_distance_backpropagates_to_both_inputs():
    E = _E()
    rs = np.random.RandomState(19)
    x1 = torch.from_numpy(_sphere(rs, 2, 65)).to(DEV).requires_grad_(True)
    x2 = torch.from_numpy(_sphere(rs, 2, 65, 0.9)).to(DEV).requires_grad_(True)
    loss = E.EarthMoverDistance()(x1, x2)
    dist, _ = E.emd()(x1.detach(), x2.detach())
    assert loss.dim() == 0 and torch.equal(loss.detach(), torch.mean(torch.sqrt(dist)))
    loss.backward()
    for t in (x1, x2):
        assert t.grad is not None and torch.isfinite(t.grad).all() and (t.grad != 0).any()


# ---- metric and runner ----------------------------------------------------------------------------------------------------------------------
def test_emd_distance_reduces_the_prediction_by_fps():
    from act_amd.utils.metrics import emd_distance
    from act_amd.utils.misc import fps
    E = _E()
    rs = np.random.RandomState(23)
    pred = torch.from_numpy(_sphere(rs, 3, 128, 0.8)).to(DEV)
    gt = torch.from_numpy(_sphere(rs, 3, 64)).to(DEV)
    val, info = emd_distance(pred, gt)
    assert val.dtype == torch.float64 and val.shape == (3,) and val.is_cuda and info.is_cuda and info.dtype == torch.int32 and (info > 0).all()
    reduced = fps(pred, 64)
    assert torch.equal(reduced[:, 0], pred[:, 0])                                         # start index 0
    dist, _ = E.emd()(reduced, gt)
    assert torch.equal(val, dist.double().sqrt().mean(dim=1) * 1000)
    same, _ = emd_distance(reduced, gt, eps=E.DEFAULT_EPS)
    assert torch.equal(same, val)
    with pytest.raises(ValueError):
        emd_distance(gt, pred)


class _Writer:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, key, value, epoch):
        self.scalars[key] = value


def test_evaluate_with_and_without_emd_val(tmp_path, capsys, monkeypatch):
    """the tiny Stage-I model and file-backed ShapeNet layout of tests/test_gpu_recon_eval.py, three taxonomies of two clouds of 64 points (the
    dense output has 128: the FPS rule is on the path).  With equal-sized taxonomies the footing row of the table, which is the mean over
    taxonomies of the per-taxonomy means for every column, is also the mean of the per-cloud values."""
    import sys
    from tests import test_gpu_recon_eval as RE
    from act_amd.utils.config import EasyDict
    from act_amd.utils.metrics import Metrics
    monkeypatch.setattr(RE, "TAXONOMIES", (("02691156", 2), ("03001627", 2), ("99999999", 2)))
    monkeypatch.setattr(RE, "NPTS", 64)
    model, loader, args, cfg, ids = RE._setup(tmp_path, DEV)
    assert "emd_val" not in cfg

    def run(c):
        capsys.readouterr()
        w = _Writer()
        m = RE._evaluate(model, loader, args, c, val_writer=w)
        return m, w.scalars, capsys.readouterr().out

    m0, w0, out0 = run(cfg)
    m0b, w0b, out0b = run(cfg)
    off = EasyDict(dict(cfg)); off["emd_val"] = False
    m0c, w0c, out0c = run(off)
    for m, w, out in ((m0b, w0b, out0b), (m0c, w0c, out0c)):
        assert m.state_dict() == m0.state_dict() and np.array_equal(m.rows, m0.rows, equal_nan=True) and m.per_taxonomy == m0.per_taxonomy
        assert w == w0 and out == out0
    assert Metrics.names() == ['F-Score', 'CDL1', 'CDL2'] and len(m0.state_dict()) == 3 and not hasattr(m0, "emd")
    assert "EMD" not in out0 and "Metric/EMD" not in w0 and sorted(w0) == ['Loss/Epoch/Dense', 'Loss/Epoch/Sparse', 'Metric/CDL1', 'Metric/CDL2',
                                                                          'Metric/F-Score']

    on = EasyDict(dict(cfg)); on["emd_val"] = True
    m1, w1, out1 = run(on)
    on_eps = EasyDict(dict(cfg)); on_eps["emd_val"] = EasyDict(eps=1e-5)
    m2, w2, out2 = run(on_eps)
    # everything that was there is unchanged
    assert m1.state_dict() == m0.state_dict() and np.array_equal(m1.rows, m0.rows, equal_nan=True) and m1.per_taxonomy == m0.per_taxonomy
    assert {k: v for k, v in w1.items() if k != "Metric/EMD"} == w0
    # the column
    e = m1.emd
    assert e["values"].shape == (6,) and (e["values"] > 0).all() and (e["info"] > 0).all() and e["capped"] == 0
    assert abs(e["overall"] - e["values"].mean()) <= 1e-12 * e["overall"]
    for t in set(ids):
        assert e["per_taxonomy"][t] == np.mean([v for v, i in zip(e["values"], ids) if i == t])
    assert w1["Metric/EMD"] == e["overall"]
    header = [ln for ln in out1.splitlines() if ln.startswith("| Taxonomy")][0]
    assert [c.strip() for c in header.strip("|").split("|")] == ['Taxonomy', '#Sample', 'F-Score', 'CDL1', 'CDL2', 'EMD', 'Category']
    footing = [ln for ln in out1.splitlines() if ln.startswith("| Overall")][0]
    assert [c.strip() for c in footing.strip("|").split("|")][5] == '%.3f' % e["overall"]
    assert np.array_equal(m2.emd["values"], e["values"]) and out2 == out1 and w2 == w1              # eps: 1e-5 is the default
    # the values are those of the metric on the model's own outputs
    from act_amd.utils.metrics import emd_distance
    cap = []
    RE._evaluate(model, loader, args, on, capture=cap)
    dense = torch.from_numpy(np.concatenate([c[2] for c in cap])).to(DEV)
    gt = torch.from_numpy(np.concatenate([c[0] for c in cap])).to(DEV)
    assert dense.shape[1] == 128 and gt.shape[1] == 64
    assert np.array_equal(emd_distance(dense, gt)[0].cpu().numpy(), e["values"])
    assert "act_amd.extensions.emd" in sys.modules
