"""GPU: the linear-SVM validation of pretrained features (csrc/svm.hip, utils/svm.py, tools/runner_pretrain.validate) against float64 numpy and
sklearn's liblinear on the problems of tests/svm_ref.py.  The solver bars are derived, not chosen: every one-vs-rest objective is strongly
convex with modulus 1 (the 1/2 (|w|^2 + b^2) term), so a point whose float64 gradient is g lies within |g| of the minimiser and its objective
within 1/2 |g|^2 of the minimum."""
import argparse
import copy
import math
import os

import numpy as np
import pytest
import torch

from tests import svm_ref as R
from tests.golden.fill import TINY_STAGE2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS32 = float(np.finfo(np.float32).eps)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_FITS = {}


def _fit(name):
    """one device fit per problem, shared by the tests that read it"""
    if name not in _FITS:
        from act_amd.utils.svm import LinearSVC
        X, y, _, _, _ = R.problem(name)
        _FITS[name] = LinearSVC().fit(_dev(X), _dev(y))
    return _FITS[name]


# ---- 1. hinge ------------------------------------------------------------------------------------------------------------------------------
def check_hinge(N, K):
    """R bit-equal to the float32 numpy expression (margins of exactly 1, an inactive column, one ulp either side of the margin), the float64 sums
    within N 2^-52 of math.fsum, two calls bit-identical; shared with tests/test_gpu_svm_edges.py"""
    from act_amd import kernels as Kn
    r = np.random.default_rng(N + K)
    classes = np.sort(r.choice(100, K, replace=False)).astype(np.int64)
    labels = classes[r.integers(0, K, N)]
    Y = np.where(labels[:, None] == classes[None, :], np.float32(1), np.float32(-1))
    M = r.normal(size=(N, K)).astype(np.float32) * np.float32(1.5)
    M[::7] = Y[::7]                                        # margins of exactly 1.0: y m == 1, h == 0
    M[:, 1] = np.float32(2) * Y[:, 1]                      # a column with no active row
    M[3, 2] = Y[3, 2] * np.float32(1 + 2.0 ** -23)         # one ulp inside: inactive; one ulp outside: active
    M[4, 2] = Y[4, 2] * np.float32(1 - 2.0 ** -24)
    H = np.maximum(np.float32(0), np.float32(1) - Y * M)
    ref = Y * H
    assert ref.dtype == np.float32
    Rd, sums = Kn.svm_hinge(_dev(M), _dev(labels), _dev(classes))
    Rd2, sums2 = Kn.svm_hinge(_dev(M), _dev(labels), _dev(classes))
    got = Rd.cpu().numpy()
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))
    assert np.array_equal((got != 0), (Y * M < 1))
    s = sums.cpu().numpy()
    assert s.dtype == np.float64 and s[1] == 0.0
    for c in range(K):
        exact = math.fsum((H[:, c].astype(np.float64) ** 2).tolist())
        print(f"hinge N={N} K={K} class {c}: |sum - fsum| / fsum = {abs(s[c] - exact) / max(exact, 1e-300):.2e} (bar {N * 2.0 ** -52:.2e})")
        assert abs(s[c] - exact) <= N * 2.0 ** -52 * exact
    assert torch.equal(Rd.view(torch.int32), Rd2.view(torch.int32)) and torch.equal(sums.view(torch.int64), sums2.view(torch.int64))


@pytest.mark.parametrize("N,K", [(257, 5), (1000, 40), (130, 64)])
def test_hinge_bits_sums_and_determinism(N, K):
    check_hinge(N, K)


# ---- 2. the two products -------------------------------------------------------------------------------------------------------------------
def _product_problem(name, N, D, K):
    X = R.problem(name)[0]
    assert X.shape == (N, D)
    r = np.random.default_rng(N)
    P = r.normal(size=(N, K)).astype(np.float32)
    P[r.random((N, K)) < 0.4] = 0                          # the sparsity of a hinge / an active mask
    return X, P


@pytest.mark.parametrize("name,N,D,K", [("n257_d33_k5", 257, 33, 5), ("n1000_d64_k10_x3", 1000, 64, 10)])
def test_transposed_product_forward_bound(name, N, D, K):
    """P^T X and the column sums of P against float64 numpy; bar per element: rows x fp32 epsilon x sum_i |p_ic x_id| (the forward error bound of a
    sum of N products in any order)"""
    from act_amd import kernels as Kn
    X, P = _product_problem(name, N, D, K)
    out, colsum = Kn.svm_tprod(_dev(P), _dev(X))
    out2, colsum2 = Kn.svm_tprod(_dev(P), _dev(X))
    P64, X64 = P.astype(np.float64), X.astype(np.float64)
    err = np.abs(out.cpu().numpy().astype(np.float64) - P64.T @ X64)
    bar = N * EPS32 * (np.abs(P64).T @ np.abs(X64))
    errb = np.abs(colsum.cpu().numpy().astype(np.float64) - P64.sum(0))
    print(f"tprod {name}: max err / bar = {(err / bar).max():.3e}, column sums {(errb / (N * EPS32 * np.abs(P64).sum(0))).max():.3e}")
    assert (err <= bar).all() and (errb <= N * EPS32 * np.abs(P64).sum(0)).all()
    assert torch.equal(out, out2) and torch.equal(colsum, colsum2)


@pytest.mark.parametrize("name,N,D,K", [("n257_d33_k5", 257, 33, 5), ("n1000_d64_k10_x3", 1000, 64, 10)])
def test_scores_forward_bound_and_mask(name, N, D, K):
    """X W^T + b against float64 numpy, bar (D + 1) x fp32 epsilon x (sum_d |x w| + |b|); a masked score is exactly zero"""
    from act_amd import kernels as Kn
    X, P = _product_problem(name, N, D, K)
    r = np.random.default_rng(D)
    W, b = r.normal(size=(K, D)).astype(np.float32), r.normal(size=K).astype(np.float32)
    X64, W64, b64 = X.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    ref = X64 @ W64.T + b64
    bar = (D + 1) * EPS32 * (np.abs(X64) @ np.abs(W64).T + np.abs(b64))
    got = Kn.svm_scores(_dev(X), _dev(W), _dev(b)).cpu().numpy()
    assert (np.abs(got - ref) <= bar).all()
    masked = Kn.svm_scores(_dev(X), _dev(W), _dev(b), mask=_dev(P)).cpu().numpy()
    assert np.array_equal(masked, np.where(P != 0, got, np.float32(0)))
    nob = Kn.svm_scores(_dev(X), _dev(W)).cpu().numpy()
    assert (np.abs(nob - X64 @ W64.T) <= bar).all()


# ---- 3. the solver -------------------------------------------------------------------------------------------------------------------------
def check_solver(name, clf):
    """Every figure (largest float64 gradient norm over the classes, Newton steps, rows left out by the gap rule) is printed before the
    assertions; notebook/svm_val.md keeps them.  Shared with tests/test_gpu_svm_edges.py"""
    X, y, Xt, _, classes = R.problem(name)
    K = len(classes)
    assert np.array_equal(clf.classes_.cpu().numpy(), classes)
    W, b = clf.coef_.cpu().numpy(), clf.intercept_.cpu().numpy()
    assert W.shape == (K, X.shape[1]) and b.shape == (K,) and W.dtype == np.float32
    status = clf.status_.numpy()
    f, gW, gb = R.objective_and_gradient(W, b, X, y, classes)
    g = np.sqrt((gW * gW).sum(1) + gb * gb)
    Wo, bo = R.oracle(name)
    go = R.grad_norms(Wo, bo, X, y, classes)
    dist = np.sqrt(((W - Wo) ** 2).sum(1) + (b - bo) ** 2)
    Wd, bd = R.oracle(name, tight=False)
    fd = R.objective_and_gradient(Wd, bd, X, y, classes)[0]
    X1 = np.sqrt((Xt.astype(np.float64) ** 2).sum(1) + 1.0)
    so = Xt.astype(np.float64) @ Wo.T + bo
    top = np.sort(so, axis=1)
    keep = (top[:, -1] - top[:, -2]) > 2.0 * X1 * 2.0 * g.max()
    pred = clf.predict(_dev(Xt)).cpu().numpy()
    print(f"{name}: status {status.tolist()} newton {clf.n_iter_} cg {clf.n_cg_}  max |g| {g.max():.3e} (oracle {go.max():.3e})  "
          f"max |[W,b] - oracle| {dist.max():.3e}  max (f - f_default) {(f - fd).max():.3e}  rows left out {int((~keep).sum())} / {R.N_TEST}  "
          f"differing kept rows {int((pred != classes[so.argmax(1)])[keep].sum())}")
    assert (status != 0).all() and clf.n_iter_ < clf.max_newton           # a stopping rule ended every class, not the iteration cap
    assert (dist <= g + go).all()
    assert (f <= fd + 0.5 * g * g).all()
    assert (~keep).sum() <= 0.01 * R.N_TEST                                # a solver that stops early fails here instead of hiding
    assert np.array_equal(pred[keep], classes[so.argmax(1)][keep])


@pytest.mark.parametrize("name", list(R.CASES))
def test_solver_against_liblinear(name):
    check_solver(name, _fit(name))


# ---- 4. classes_ with a skipped id -----------------------------------------------------------------------------------------------------------
def test_skipped_class_id_gets_no_column():
    from act_amd.tools.runner_pretrain import evaluate_svm
    X, y, Xt, yt, classes = R.problem("n300_d24_skip")
    assert len(classes) == 5 and 2 not in classes and classes.max() == 5
    clf = _fit("n300_d24_skip")
    assert clf.coef_.shape == (5, X.shape[1]) and clf.intercept_.shape == (5,)
    assert clf.decision_function(_dev(Xt)).shape == (R.N_TEST, 5)
    pred = clf.predict(_dev(Xt)).cpu().numpy()
    assert set(pred.tolist()) <= set(classes.tolist())
    acc = evaluate_svm(_dev(X), _dev(y), _dev(Xt), _dev(yt))
    assert isinstance(acc, float) and acc == 100.0 * np.mean(pred == yt)
    assert acc > 100.0 / 5                                                 # the clusters are separable enough to beat chance


def test_predict_ties_go_to_the_lowest_index():
    from act_amd.utils.svm import LinearSVC
    clf = LinearSVC()
    clf.classes_ = torch.tensor([3, 5, 9], device=DEV)
    clf.coef_ = torch.tensor([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]], device=DEV)
    clf.intercept_ = torch.zeros(3, device=DEV)
    x = torch.tensor([[2.0, 1.0], [1.0, 2.0], [1.0, 1.0]], device=DEV)
    assert clf.predict(x).tolist() == [3, 9, 3]


# ---- 5. determinism --------------------------------------------------------------------------------------------------------------------------
def test_two_fits_are_bit_identical():
    from act_amd.utils.svm import LinearSVC
    X, y, _, _, _ = R.problem("n515_d48_k7")
    Xd, yd = _dev(X), _dev(y)
    a, b = LinearSVC().fit(Xd, yd), LinearSVC().fit(Xd, yd)
    assert torch.equal(a.coef_.view(torch.int32), b.coef_.view(torch.int32))
    assert torch.equal(a.intercept_.view(torch.int32), b.intercept_.view(torch.int32)) and a.n_iter_ == b.n_iter_


# ---- 6. the runner ---------------------------------------------------------------------------------------------------------------------------
def _args(tmp, **kw):
    a = argparse.Namespace(log_name="test", use_gpu=True, local_rank=0, distributed=False, sync_bn=False, resume=False, start_ckpts=None,
                           experiment_path=str(tmp), num_workers=0, world_size=1, val_freq=1)
    a.__dict__.update(kw)
    return a


def _config(extra_train, svm_val=None, bs=8, npoints=128, max_epoch=1):
    """tests/test_gpu_runner.py's tiny Stage-II run (two steps an epoch), the validation splits as the reference's pretrain YAML has them:
    val = ModelNet test, extra_train = ModelNet train"""
    from act_amd.utils.config import EasyDict
    shp = lambda subset: dict(_base_=dict(NAME="ShapeNet", N_POINTS=8192, SYNTHETIC=True, NUM_SAMPLES=16, DATA_PATH="none", PC_PATH="none"),
                              others=dict(subset=subset, npoints=npoints, bs=bs))
    mn = lambda subset: dict(_base_=dict(NAME="ModelNet", N_POINTS=256, NUM_CATEGORY=4, USE_NORMALS=False, SYNTHETIC=True, NUM_SAMPLES=48,
                                         DATA_PATH="none"), others=dict(subset=subset, bs=16))
    dataset = dict(train=shp("train"), val=mn("test"))
    if extra_train:
        dataset["extra_train"] = mn("train")
    cfg = EasyDict(optimizer=dict(type="AdamW", kwargs=dict(lr=1e-3, weight_decay=0.05)), scheduler=dict(type="CosLR", kwargs=dict(epochs=300, initial_epochs=10)),
                   dataset=dataset, model=copy.deepcopy(TINY_STAGE2), total_bs=bs, step_per_update=1, max_epoch=max_epoch, consider_metric="CDL1")
    if svm_val is not None:
        cfg["svm_val"] = svm_val
    return cfg


def test_run_net_validates_and_keeps_the_best(tmp_path, monkeypatch):
    from act_amd.tools import runner_pretrain as RP
    seen = []
    real_eval = RP.evaluate_svm

    def spy(trf, trl, tef, tel):
        acc = real_eval(trf, trl, tef, tel)
        seen.append((acc, tuple(trf.shape), tuple(tef.shape), trf.is_cuda, trl.is_cuda))
        return acc
    metrics = []
    real_validate = RP.validate

    def validate(*a, **k):
        metrics.append(real_validate(*a, **k))
        return metrics[-1]
    monkeypatch.setattr(RP, "evaluate_svm", spy)
    monkeypatch.setattr(RP, "validate", validate)
    torch.manual_seed(0)
    log = RP.run_net(_args(tmp_path), _config(True, svm_val=True), log_every=1)
    assert len(log) == 4 and all(math.isfinite(v) for v in log)             # epochs 0 and 1, two steps each
    assert len(metrics) == 2 and len(seen) == 2
    for m, (acc, trs, tes, c1, c2) in zip(metrics, seen):
        assert isinstance(m, RP.Acc_Metric) and 0.0 <= m.acc <= 100.0 and m.acc == acc
        assert trs == (48, 32) and tes == (48, 32) and c1 and c2           # cls_dim features of both splits, on the device
    ck = torch.load(os.path.join(tmp_path, "ckpt-best.pth"), map_location="cpu")
    assert ck["best_metrics"]["acc"] == max(m.acc for m in metrics) and ck["metrics"]["acc"] == ck["best_metrics"]["acc"]
    last = torch.load(os.path.join(tmp_path, "ckpt-last.pth"), map_location="cpu")
    assert last["metrics"]["acc"] == metrics[-1].acc and last["best_metrics"]["acc"] == ck["best_metrics"]["acc"]


def test_run_net_with_the_switch_off_is_the_run_without_extra_train(tmp_path):
    """svm_val off (absent or False) with an extra_train section: the loss list is bit-identical to the run whose config has no extra_train at
    all (the loop as it was before the validation existed), and no ckpt-best appears"""
    from act_amd.tools.runner_pretrain import run_net
    logs = []
    for i, cfg in enumerate((_config(False), _config(True), _config(True, svm_val=False))):
        torch.manual_seed(0)
        out = tmp_path / str(i)
        out.mkdir()
        logs.append(run_net(_args(out), cfg, log_every=1))
        assert not os.path.exists(out / "ckpt-best.pth") and os.path.exists(out / "ckpt-last.pth")
    assert len(logs[0]) == 4
    assert np.array_equal(np.array(logs[0]).view(np.int64), np.array(logs[1]).view(np.int64))
    assert np.array_equal(np.array(logs[0]).view(np.int64), np.array(logs[2]).view(np.int64))
