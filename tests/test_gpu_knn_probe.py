"""GPU: the weighted k-NN probe (csrc/knn_probe.hip, utils/knn_probe.py, tools/runner_pretrain.validate) against the float64 oracle of
tests/knn_probe_ref.py.

Bars.  Lattice inputs (integers in [-4, 4], normalize off): every dot product is exact in fp32 in any order, so idx and sim must equal the
oracle's element for element, ties included.  Cosine mode: tau = 2 (D + 4) 2^-24 bounds the rounding of an fp32 dot product of unit vectors plus
the two normalisations; a query whose k-th and (k+1)-th oracle similarities are within tau is exempt from the set comparison, and at most 2 % of
the queries may be (asserted on the oracle alone, first).  An isotropic Gaussian does not meet that cap at D = 770 (its cosines have standard
deviation 1/sqrt(D), so about one query in ten has such a near-tie at rank 20 of 1000: measured 11 and 14 of 130 on two seeds), so the features
are Gaussian with a power-law spectrum (coordinate d scaled by 1 / (1 + d)), which is also what trained features look like; seed 1 gives 0 of 130
exempt at D = 64 and 2 of 130 at D = 770."""
import argparse
import copy

import pytest
import torch

from tests import knn_probe_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# tile edges of the kernels: 64 / 32 queries per workgroup (k <= 128 / above), 128 bank rows per tile, 16-deep feature chunks, list
# capacities 32 / 128 / 256
K_EDGES = (1, 20, 32, 33, 128, 129)


def _K():
    import act_amd.kernels as K
    return K


def _lattice_case(D, Nq, Nb):
    bank = R.lattice(Nb, D, seed=1000 * D + Nb, duplicates=min(5, Nb // 2))     # exact duplicate rows: ties that only the index breaks
    q = R.lattice(Nq, D, seed=7 + 1000 * D + Nq)
    q[0] = bank[0]
    return q, bank


@pytest.mark.parametrize("Nb", [21, 129, 1000])
@pytest.mark.parametrize("Nq", [1, 65, 130])
@pytest.mark.parametrize("D", [3, 5, 64])
def test_exact_lattice(D, Nq, Nb):
    K = _K()
    q, bank = _lattice_case(D, Nq, Nb)
    kfull = min(256, Nb)
    s_ref, i_ref = R.search(q, bank, kfull, normalize_rows=False)
    for k in sorted(set(kk for kk in K_EDGES if kk <= Nb) | {kfull}):
        sim, idx = K.knn_probe_search(q.to(DEV), bank.to(DEV), k, normalize=False)
        assert torch.equal(idx.cpu().long(), i_ref[:, :k]), (D, Nq, Nb, k)
        assert torch.equal(sim.cpu().double(), s_ref[:, :k]), (D, Nq, Nb, k)


@pytest.mark.parametrize("D,Nq,Nb", [(16, 64, 128), (17, 33, 257), (15, 32, 127), (48, 63, 256)])
def test_exact_lattice_at_the_tile_edges(D, Nq, Nb):
    """exactly one query tile / bank tile / feature chunk, and one more or one fewer"""
    K = _K()
    q, bank = _lattice_case(D, Nq, Nb)
    kfull = min(256, Nb)
    s_ref, i_ref = R.search(q, bank, kfull, normalize_rows=False)
    for k in sorted(set(kk for kk in K_EDGES if kk <= Nb) | {kfull}):
        for splits in (0, 2):
            sim, idx = K.knn_probe_search(q.to(DEV), bank.to(DEV), k, normalize=False, splits=splits)
            assert torch.equal(idx.cpu().long(), i_ref[:, :k]), (k, splits)
            assert torch.equal(sim.cpu().double(), s_ref[:, :k]), (k, splits)


def _gauss(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, D, generator=g) * (1.0 + torch.arange(D)).pow(-1.0)


_COS = {}


def _cosine_case(D):
    """the inputs, the oracle's 21 best and its scores, computed once"""
    if D not in _COS:
        bank, q = _gauss(1000, D, 1), _gauss(130, D, 1001)
        labels = (torch.arange(1000) * 7 + 3) % 10
        s, i = R.search(q, bank, 21)
        _COS[D] = dict(bank=bank, q=q, labels=labels, s=s, i=i, scores=R.vote(s[:, :20], i[:, :20], labels, 10, [20], 0.07))
    return _COS[D]


@pytest.mark.parametrize("D", [64, 770])
def test_cosine_mode_against_the_oracle(D):
    K = _K()
    c = _cosine_case(D)
    k, T = 20, 0.07
    tau = 2.0 * (D + 4) * 2.0 ** -24
    exempt = (c["s"][:, k - 1] - c["s"][:, k]) <= tau
    print(f"D = {D}: tau = {tau:.3e}, exempt {int(exempt.sum())} of {exempt.numel()}")
    assert exempt.sum().item() <= 0.02 * exempt.numel()                       # on the oracle alone: the cap cannot hide a failure
    sim, idx = K.knn_probe_search(c["q"].to(DEV), c["bank"].to(DEV), k)
    scores, pred, _ = K.knn_probe_vote(sim, idx, c["labels"].to(DEV).int(), 10, [k], T)
    sim, idx, scores, pred = sim.cpu().double(), idx.cpu().long(), scores.cpu().double()[:, 0], pred.cpu()[:, 0]
    keep = ~exempt
    assert torch.equal(idx[keep].sort(dim=1).values, c["i"][keep, :k].sort(dim=1).values)
    err = (sim - c["s"][:, :k]).abs().max().item()
    print(f"max |sim - oracle| = {err:.3e}")
    assert err <= tau
    ref = c["scores"][:, 0]
    rel = 2.0 * tau / T
    serr = ((scores - ref).abs()[keep] / ref[keep].clamp_min(1e-300)).max().item() if (ref[keep] > 0).any() else 0.0
    bad = ((scores - ref).abs() > rel * ref)[keep]
    print(f"max relative class-score error = {serr:.3e} (bar {rel:.3e})")
    assert not bad.any()
    top2 = ref.topk(2, dim=1).values
    clear = keep & ((top2[:, 0] - top2[:, 1]) > rel * top2[:, 0])
    assert clear.sum() > 100 and torch.equal(pred[clear], R.predict(ref)[clear])


@pytest.mark.parametrize("k", [20, 200])
def test_result_does_not_depend_on_the_splits(k):
    K = _K()
    c = _cosine_case(64)
    q, bank, cls = c["q"].to(DEV), c["bank"].to(DEV), c["labels"].to(DEV).int()
    assert [K.lib.act_knn_probe_splits(130, 1000, k, s) for s in (1, 2, 7)] == [1, 2, 7]
    outs = []
    for splits in (1, 2, 7, 7, 0):
        sim, idx = K.knn_probe_search(q, bank, k, splits=splits)
        scores, pred, _ = K.knn_probe_vote(sim, idx, cls, 10, [5, k], 0.07)
        outs.append((idx, sim.view(torch.int32), scores.view(torch.int32), pred))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], o))


def test_zero_rows_produce_no_nan():
    K = _K()
    bank, q = _gauss(200, 24, 5), _gauss(70, 24, 6)
    bank[17] = 0
    q[3] = 0
    assert torch.equal(K.knn_probe_normalize(bank.to(DEV))[17].cpu(), torch.zeros(24))
    sim, idx = K.knn_probe_search(q.to(DEV), bank.to(DEV), 200)
    scores, pred, _ = K.knn_probe_vote(sim, idx, (torch.arange(200) % 3).int().to(DEV), 3, [20, 200], 0.07)
    assert torch.isfinite(sim).all() and torch.isfinite(scores).all()
    assert torch.equal(sim[3].cpu(), torch.zeros(200)) and torch.equal(idx[3].cpu().long(), torch.arange(200))     # all ties: index order
    pos = (idx.cpu() == 17).nonzero()
    assert pos.shape[0] == 70 and (sim.cpu()[pos[:, 0], pos[:, 1]] == 0).all()
    s_ref, _ = R.search(q, bank, 200)
    assert (sim.cpu().double() - s_ref).abs().max() <= 2.0 * 28 * 2.0 ** -24


def test_labels_map_through_classes_and_counts_match_the_scores():
    from act_amd.utils.knn_probe import KNNClassifier
    K = _K()
    bank, q = _gauss(300, 40, 11), _gauss(90, 40, 12)
    names = torch.tensor([3, 7, 39])
    yb, yq = names[torch.arange(300) % 3], names[(torch.arange(90) * 5) % 3]
    yq[4] = 1000                                                           # a label the bank does not have: never a hit
    clf = KNNClassifier(k=[1, 20]).fit(bank.to(DEV), yb.to(DEV))
    assert torch.equal(clf.classes_.cpu(), names)
    pred = clf.predict(q.to(DEV)).cpu()
    assert set(pred.tolist()) <= {3, 7, 39}
    _, i1 = clf.kneighbors(q.to(DEV))
    assert torch.equal(pred, yb[i1[:, 0].cpu().long()])                     # k = 1: the nearest row's label
    acc = clf.score(q.to(DEV), yq.to(DEV))
    assert acc["knn@1"] == (pred == yq).sum().item() * 100.0 / 90
    # ten classes: top-5 is not trivial; the device counts against the ranks of the returned scores
    cb, cq = (torch.arange(300) * 7 + 1) % 10, (torch.arange(90) * 3) % 10
    sim, idx = K.knn_probe_search(q.to(DEV), bank.to(DEV), 20)
    scores, dpred, counts = K.knn_probe_vote(sim, idx, cb.int().to(DEV), 10, [1, 5, 20], 0.07, q_cls=cq.int().to(DEV))
    scores = scores.cpu().double()
    for j in range(3):
        assert counts[j].tolist() == list(R.hits(scores[:, j], cq))
        assert torch.equal(dpred[:, j].cpu(), R.predict(scores[:, j]))
    assert counts[2, 0] <= counts[2, 1]


def test_exclude_self_by_index_returns_the_duplicate():
    from act_amd.utils.knn_probe import KNNClassifier
    bank = _gauss(150, 33, 21)
    bank[140:] = bank[:10]
    clf = KNNClassifier(k=[1, 149]).fit(bank.to(DEV), (torch.arange(150) % 4).to(DEV))
    sim, idx = clf.kneighbors(bank.to(DEV), exclude_self=True)
    idx = idx.cpu().long()
    assert not (idx == torch.arange(150).unsqueeze(1)).any()
    assert torch.equal(idx[:10, 0], torch.arange(140, 150)) and torch.equal(idx[140:, 0], torch.arange(10))
    assert torch.equal(idx.sort(dim=1).values, R.search(bank, bank, 149, exclude_self=True)[1].sort(dim=1).values)
    # lattice: exact, the whole order
    q, lb = _lattice_case(5, 130, 130)
    K = _K()
    _, li = K.knn_probe_search(lb.to(DEV), lb.to(DEV), 129, normalize=False, exclude_self=True)
    assert torch.equal(li.cpu().long(), R.search(lb, lb, 129, normalize_rows=False, exclude_self=True)[1])


def test_bad_arguments_raise_and_name_the_value():
    from act_amd._C import ActHipError
    from act_amd.utils.knn_probe import KNNClassifier
    x, y = _gauss(30, 8, 1).to(DEV), (torch.arange(30) % 3).to(DEV)
    with pytest.raises(ActHipError, match="31"):
        KNNClassifier(k=31).fit(x, y).kneighbors(x)
    with pytest.raises(ActHipError, match="30"):
        KNNClassifier(k=30).fit(x, y).kneighbors(x, exclude_self=True)
    with pytest.raises(ActHipError, match="257"):
        KNNClassifier(k=257)
    with pytest.raises(ActHipError, match="float64"):
        KNNClassifier().fit(x.double(), y)
    with pytest.raises(ActHipError, match="float32"):
        KNNClassifier().fit(x, y.float())
    K = _K()
    with pytest.raises(ActHipError):
        K.knn_probe_search(x.cpu(), x, 3)
    ws = torch.empty(1 << 20, dtype=torch.float32, device=DEV)
    out = torch.empty(30, 31, dtype=torch.int32, device=DEV)
    rc = K.lib.act_knn_probe_search_f32(K.ptr(x), 30, K.ptr(x), 30, 8, 31, 1, 0, 0, K.ptr(out), None, K.ptr(ws), ws.numel() * 4, K.stream())
    assert rc != 0                                                          # the C entry refuses k > Nb by itself


# ---- the runner ----------------------------------------------------------------------------------------------------------------------------------
def _config(**kw):
    from act_amd.utils.config import EasyDict
    from tests.golden.fill import TINY_STAGE2
    shp = dict(_base_=dict(NAME="ShapeNet", N_POINTS=8192, SYNTHETIC=True, NUM_SAMPLES=16, DATA_PATH="none", PC_PATH="none"),
               others=dict(subset="train", npoints=128, bs=8))
    mn = lambda subset: dict(_base_=dict(NAME="ModelNet", N_POINTS=256, NUM_CATEGORY=4, USE_NORMALS=False, SYNTHETIC=True, NUM_SAMPLES=48,
                                         DATA_PATH="none"), others=dict(subset=subset, bs=16))
    return EasyDict(optimizer=dict(type="AdamW", kwargs=dict(lr=1e-3, weight_decay=0.05)), scheduler=dict(type="CosLR", kwargs=dict(epochs=300, initial_epochs=10)),
                    dataset=dict(train=shp, val=mn("test"), extra_train=mn("train")), model=copy.deepcopy(TINY_STAGE2), total_bs=8, step_per_update=1,
                    max_epoch=0, consider_metric="CDL1", **kw)


@pytest.mark.parametrize("with_svm", [False, True])
def test_validate_logs_the_knn_accuracy(tmp_path, monkeypatch, with_svm):
    from act_amd.tools import runner_pretrain as RP
    from act_amd.utils.knn_probe import KNNClassifier
    seen, lines, metrics, svm = [], [], [], []
    real_knn, real_svm, real_validate, real_log = RP.evaluate_knn, RP.evaluate_svm, RP.validate, RP.print_log

    def spy_knn(trf, trl, tef, tel, ks, T):
        seen.append((trf.clone(), trl.clone(), tef.clone(), tel.clone(), list(ks), T))
        return real_knn(trf, trl, tef, tel, ks, T)
    monkeypatch.setattr(RP, "evaluate_knn", spy_knn)
    monkeypatch.setattr(RP, "evaluate_svm", lambda *a: svm.append(real_svm(*a)) or svm[-1])
    monkeypatch.setattr(RP, "validate", lambda *a, **k: metrics.append(real_validate(*a, **k)) or metrics[-1])
    monkeypatch.setattr(RP, "print_log", lambda msg, logger=None: lines.append(str(msg)) or real_log(msg, logger=logger))
    args = argparse.Namespace(log_name="test", use_gpu=True, local_rank=0, distributed=False, sync_bn=False, resume=False, start_ckpts=None,
                              experiment_path=str(tmp_path), num_workers=0, world_size=1, val_freq=1)
    torch.manual_seed(0)
    kw = dict(knn_val=dict(k=[5, 10], T=0.07))
    if with_svm:
        kw["svm_val"] = True
    RP.run_net(args, _config(**kw), log_every=1)
    assert len(seen) == 1 and len(metrics) == 1 and len(svm) == int(with_svm)
    trf, trl, tef, tel, ks, T = seen[0]
    assert ks == [5, 10] and T == 0.07 and trf.is_cuda and tuple(trf.shape) == (48, 32)
    acc = KNNClassifier(k=[5, 10], T=0.07).fit(trf, trl).score(tef, tel)
    for k in (5, 10):
        assert any(("knn@%d = %.4f" % (k, acc["knn@%d" % k])) in ln and "[Validation] EPOCH: 0" in ln for ln in lines), lines
    assert metrics[0].acc == (svm[0] if with_svm else acc["knn@5"])
