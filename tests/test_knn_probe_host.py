"""CPU: the weighted k-NN probe is declared through every layer (header, ABI table, config), its float64 oracle has the properties the GPU tests
lean on, KNNClassifier refuses CPU tensors, and run_net never evaluates it unless it is asked to."""
import argparse
import os
import re

import pytest
import torch

from tests import knn_probe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("act_knn_probe_normalize_f32", "act_knn_probe_splits", "act_knn_probe_workspace", "act_knn_probe_search_f32", "act_knn_probe_vote_f32")


def test_entry_points_are_declared_in_the_header_and_the_abi_table():
    from act_amd import _abi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "act_hip.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert name in _abi.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert os.path.exists(os.path.join(ROOT, "act_amd", "csrc", "knn_probe.hip"))
    from act_amd import build
    assert "knn_probe.hip" in build.sources()


def test_fit_refuses_cpu_tensors_and_bad_k():
    from act_amd._C import ActHipError
    from act_amd.utils.knn_probe import KNNClassifier
    with pytest.raises(ActHipError):
        KNNClassifier().fit(torch.zeros(8, 4), torch.zeros(8, dtype=torch.int64))
    with pytest.raises(ActHipError, match="257"):
        KNNClassifier(k=257)
    with pytest.raises(ActHipError):
        KNNClassifier(k=[20, 10])


def _problem():
    bank = torch.randn(60, 5, generator=torch.Generator().manual_seed(3))
    bank[53:] = bank[:7]                                              # rows 53 .. 59 repeat rows 0 .. 6
    labels = torch.arange(60) % 4
    return bank, labels


def test_oracle_k1_on_the_bank_returns_each_rows_own_label():
    bank, labels = _problem()
    _, idx = R.search(bank, bank, 1)
    assert torch.equal(labels[idx[:, 0]][7:53], labels[7:53])         # a row is its own nearest neighbour under the cosine ...
    assert torch.equal(idx[:53, 0], torch.arange(53))                 # ... and the first of its duplicates wins the tie
    assert torch.equal(idx[53:, 0], torch.arange(7))


def test_oracle_exclude_self_never_returns_the_diagonal_and_finds_the_duplicate():
    bank, _ = _problem()
    _, idx = R.search(bank, bank, 59, exclude_self=True)
    assert not (idx == torch.arange(60).unsqueeze(1)).any()
    assert torch.equal(idx[:7, 0], torch.arange(53, 60)) and torch.equal(idx[53:, 0], torch.arange(7))


def test_oracle_lists_are_prefixes_and_duplicates_go_by_index():
    bank, labels = _problem()
    q = R.lattice(9, 5, seed=4)
    s20, i20 = R.search(q, bank, 20, normalize_rows=False)
    s5, i5 = R.search(q, bank, 5, normalize_rows=False)
    assert torch.equal(i20[:, :5], i5) and torch.equal(s20[:, :5], s5)
    sall, iall = R.search(q, bank, 60, normalize_rows=False)
    tie = sall[:, 1:] == sall[:, :-1]
    assert tie.any() and (iall[:, 1:][tie] > iall[:, :-1][tie]).all()
    sc = R.vote(s20, i20, labels, 4, [5, 20], 0.5)
    assert (R.rank_of(sc[:, 1], R.predict(sc[:, 1])) == 0).all()


def test_the_knn_config_loads():
    from act_amd.utils.config import cfg_from_yaml_file
    cwd = os.getcwd()
    os.chdir(os.path.join(ROOT, "act_amd"))
    try:
        cfg = cfg_from_yaml_file("cfgs/synthetic/pretrain_act_distill_knn.yaml")
    finally:
        os.chdir(cwd)
    assert list(cfg.knn_val.k) == [10, 20] and cfg.knn_val.T == 0.07 and not cfg.get("svm_val", False)
    assert cfg.dataset.extra_train.others.subset == "train" and cfg.dataset.val.others.subset == "test"


def test_run_net_without_knn_val_never_calls_evaluate_knn(monkeypatch, tmp_path):
    """stand-ins for the model, the loaders, the step and the checkpoint writer, as tests/test_svm_host.py has them: with svm_val alone the k-NN
    probe is neither called nor imported; knn_val alone switches the validation on"""
    import sys
    from act_amd.tools import runner_pretrain as RP
    from act_amd.utils.config import EasyDict
    knn_calls, svm_calls, built = [], [], []

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

    class Batch:
        def to(self, *a, **k):
            return torch.zeros(2, 8, 3)

    def dataset_builder(args, cfg):
        built.append(cfg.others.subset)
        return None, [("synthetic", "000000", Batch())]

    feats = (torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64))
    monkeypatch.setattr(RP, "extract_features", lambda *a, **k: feats)
    monkeypatch.setattr(RP, "evaluate_knn", lambda *a, **k: knn_calls.append(a[4:]) or {"knn@%d" % k_: 50.0 + k_ for k_ in a[4]})
    monkeypatch.setattr(RP, "evaluate_svm", lambda *a, **k: svm_calls.append(1) or 25.0)
    monkeypatch.setattr(RP.builder, "dataset_builder", dataset_builder)
    monkeypatch.setattr(RP.builder, "model_builder", lambda cfg: Model())
    monkeypatch.setattr(RP.builder, "save_checkpoint", lambda *a, **k: None)
    monkeypatch.setattr(RP, "train_step", lambda *a, **k: torch.tensor(0.5))
    sys.modules.pop("act_amd.utils.knn_probe", None)
    ds = lambda subset: dict(_base_=dict(NAME="ShapeNet"), others=dict(subset=subset, npoints=8, bs=2))
    args = argparse.Namespace(log_name="test", use_gpu=False, local_rank=0, distributed=False, sync_bn=False, resume=False, start_ckpts=None,
                              experiment_path=str(tmp_path), num_workers=0, world_size=1, val_freq=1)

    def cfg(**kw):
        return EasyDict(optimizer=dict(type="AdamW", kwargs=dict(lr=1e-3, weight_decay=0.05)), scheduler=dict(type="CosLR", kwargs=dict(epochs=3, initial_epochs=1)),
                        dataset=dict(train=ds("train"), val=ds("test"), extra_train=ds("extra")), model=dict(NAME="none"), total_bs=2, step_per_update=1,
                        max_epoch=0, **kw)

    RP.run_net(args, cfg(), log_every=1)
    assert knn_calls == [] and svm_calls == [] and "extra" not in built
    RP.run_net(args, cfg(svm_val=True), log_every=1)
    assert knn_calls == [] and svm_calls == [1] and "act_amd.utils.knn_probe" not in sys.modules
    metrics = []
    real_validate = RP.validate
    monkeypatch.setattr(RP, "validate", lambda *a, **k: metrics.append(real_validate(*a, **k)) or metrics[-1])
    RP.run_net(args, cfg(knn_val=dict(k=[3, 7], T=0.1)), log_every=1)
    assert knn_calls == [([3, 7], 0.1)] and svm_calls == [1] and metrics[-1].acc == 53.0          # the first k's top-1 is the metric
    RP.run_net(args, cfg(knn_val=dict(k=[3, 7], T=0.1), svm_val=True), log_every=1)
    assert len(knn_calls) == 2 and svm_calls == [1, 1] and metrics[-1].acc == 25.0                # next to the SVM, the SVM's stays the metric
    args.val_freq = 0
    RP.run_net(args, cfg(knn_val=dict(k=[3, 7], T=0.1)), log_every=1)
    assert len(knn_calls) == 2
