"""CPU: the float64 objective the linear-SVM tests measure against is liblinear's (the regularised bias included), LinearSVC refuses CPU
tensors, and run_net never validates unless it is asked to."""
import argparse

import numpy as np
import pytest
import torch

from tests import svm_ref as R


@pytest.mark.parametrize("name", list(R.CASES))
def test_float64_objective_is_liblinears(name):
    """the minimiser of svm_ref.objective_and_gradient (L-BFGS from 0, one class at a time) against the tight sklearn oracle: both objectives are
    strongly convex with modulus 1, so each solution is within its own gradient norm of the common minimiser -- IF the objectives are the same"""
    from scipy.optimize import minimize
    X, y, _, _, classes = R.problem(name)
    Wo, bo = R.oracle(name)
    go = R.grad_norms(Wo, bo, X, y, classes)
    D = X.shape[1]
    for c in range(len(classes)):
        def fg(v, c=c):
            f, gW, gb = R.objective_and_gradient(v[None, :D], v[D:], X, y, classes[c:c + 1])
            return f[0], np.concatenate([gW[0], gb])
        res = minimize(fg, np.zeros(D + 1), jac=True, method="L-BFGS-B", options=dict(maxiter=20000, maxfun=40000, ftol=0.0, gtol=1e-9, maxcor=30))
        gm = np.linalg.norm(fg(res.x)[1])
        dist = np.linalg.norm(res.x - np.concatenate([Wo[c], bo[c:c + 1]]))
        print(f"{name} class {c}: |min - oracle| = {dist:.3e}, gradient norms {gm:.3e} (L-BFGS) {go[c]:.3e} (oracle)")
        assert gm < 1e-4                                    # L-BFGS did reach a minimiser
        assert dist <= gm + go[c]


@pytest.mark.parametrize("name", list(R.WIDE_CASES))
def test_wide_cases_leave_room_for_the_gap_rule(name):
    """a property of the wide problems and their oracle, checked before any device is used: a device result whose gradient norm is under
    G_ALLOW_MIN (eight times the largest ending norm notebook/svm_val.md records) loses at most 1 % of the test rows to the gap rule"""
    assert name not in R.CASES and len(R.problem(name)[4]) == R.WIDE_CASES[name][2]      # every id occurs in the draw
    ga = R.g_allow(name)
    print(f"{name}: g_allow = {ga:.3e} (bar {R.G_ALLOW_MIN:.0e})")
    assert ga >= R.G_ALLOW_MIN


def test_fit_refuses_cpu_tensors():
    from act_amd._C import ActHipError
    from act_amd.utils.svm import LinearSVC
    X, y, _, _, _ = R.problem("n257_d33_k5")
    with pytest.raises(ActHipError):
        LinearSVC().fit(torch.from_numpy(X.copy()), torch.from_numpy(y.copy()))


def test_no_sklearn_under_the_package():
    import os
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "act_amd")
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".py"):
                with open(os.path.join(d, f)) as fh:
                    text = fh.read()
                assert "import sklearn" not in text and "from sklearn" not in text, f


def test_run_net_without_svm_val_never_validates(monkeypatch, tmp_path):
    """the validation is opt-in: with an extra_train section and val_freq 1 but no ``svm_val: True``, run_net neither builds the extra loader nor
    calls validate (the model, the loaders, the step and the checkpoint writer are stand-ins: the loop itself runs on the CPU, one batch an epoch)"""
    from act_amd.tools import runner_pretrain as RP
    from act_amd.utils.config import EasyDict
    called, built = [], []

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

    class Batch:                                     # what the loop moves to the device: stays where it is
        def to(self, *a, **k):
            return torch.zeros(2, 8, 3)

    def dataset_builder(args, cfg):
        built.append(cfg.others.subset)
        return None, [("synthetic", "000000", Batch())]

    monkeypatch.setattr(RP, "validate", lambda *a, **k: called.append(a) or RP.Acc_Metric(1.0))
    monkeypatch.setattr(RP.builder, "dataset_builder", dataset_builder)
    monkeypatch.setattr(RP.builder, "model_builder", lambda cfg: Model())
    monkeypatch.setattr(RP.builder, "save_checkpoint", lambda *a, **k: None)
    monkeypatch.setattr(RP, "train_step", lambda *a, **k: torch.tensor(0.5))
    ds = lambda subset: dict(_base_=dict(NAME="ShapeNet"), others=dict(subset=subset, npoints=8, bs=2))
    args = argparse.Namespace(log_name="test", use_gpu=False, local_rank=0, distributed=False, sync_bn=False, resume=False, start_ckpts=None,
                              experiment_path=str(tmp_path), num_workers=0, world_size=1, val_freq=1)

    def cfg(**kw):
        return EasyDict(optimizer=dict(type="AdamW", kwargs=dict(lr=1e-3, weight_decay=0.05)), scheduler=dict(type="CosLR", kwargs=dict(epochs=3, initial_epochs=1)),
                        dataset=dict(train=ds("train"), val=ds("test"), extra_train=ds("extra")), model=dict(NAME="none"), total_bs=2, step_per_update=1,
                        max_epoch=1, **kw)

    RP.run_net(args, cfg(), log_every=1)
    RP.run_net(args, cfg(svm_val=False), log_every=1)
    assert called == [] and "extra" not in built
    RP.run_net(args, cfg(svm_val=True), log_every=1)                    # and the switch does switch it on: epochs 0 and 1
    assert len(called) == 2 and built.count("extra") == 1
    args.val_freq = 0
    RP.run_net(args, cfg(svm_val=True), log_every=1)
    assert len(called) == 2
