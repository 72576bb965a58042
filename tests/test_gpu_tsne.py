"""GPU: the exact t-SNE of classifier features (csrc/tsne.hip, utils/tsne.py, tools/runner_tsne.py) against the float64 numpy restatement of
tests/tsne_ref.py, stage by stage with injected inputs, then a whole fit against the reference's own noise floor."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import tsne_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FLIP_SHARE = 1e-3                  # the share of elements a legitimate gain flip may move (the project's flip-tolerant bar)


def _dev(a, dtype=None):
    a = np.array(a, dtype=dtype, order="C")                     # a writable copy: the reference arrays are frozen
    return torch.from_numpy(a).to(DEV)


def _csr32(label):
    """the reference's CSR with float32 values, on the device, and the dense float64 P those float32 values make"""
    _, _, _, _, indptr, indices, values = R.affinities(label)
    v32 = values.astype(np.float32)
    N = len(indptr) - 1
    P = np.zeros((N, N))
    P[np.repeat(np.arange(N), np.diff(indptr)), indices] = v32.astype(np.float64)
    return (_dev(indptr), _dev(indices), _dev(v32)), P


# ---- 1. kNN -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["A", "B", "C"])
def test_knn_sets_and_distances(label):
    from act_amd import kernels as K
    X, _, _, k = R.problem(label)
    ridx, rdist, gap = R.knn(label)
    idx, dist = K.tsne_knn_cosine(_dev(X), k)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert idx.dtype == np.int32 and idx.shape == (X.shape[0], k) and dist.shape == idx.shape
    decided = gap > 1e-5                                     # a smaller gap cannot be decided by fp32 products
    print(f"{label}: {int((~decided).sum())} of {len(gap)} rows left out; max |dist - ref| = {np.abs(dist - rdist).max():.2e}")
    assert (~decided).mean() <= 0.02
    assert np.array_equal(np.sort(idx[decided], axis=1), np.sort(ridx[decided], axis=1))
    assert np.all(idx != np.arange(X.shape[0])[:, None])
    assert np.abs(dist - rdist)[decided].max() <= 1e-5 and np.all(np.diff(dist, axis=1) >= 0)


def test_knn_clamp_self_ties_and_zero_row():
    from act_amd import kernels as K
    X, _, perp, k = R.problem("D")
    N = X.shape[0]
    assert k == N - 1 == 19 < 3 * perp
    idx, dist = K.tsne_knn_cosine(_dev(X), k)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    others = [np.array([j for j in range(N) if j != i]) for i in range(N)]
    for i in range(N):
        assert np.array_equal(np.sort(idx[i]), others[i]) and np.all(np.diff(dist[i]) >= 0)
    assert np.array_equal(idx[R.D_ZERO], others[R.D_ZERO]) and np.all(dist[R.D_ZERO] == 1.0)        # distance 1 to every row, index order
    assert idx[R.D_DUP_OF, 0] == R.D_DUP and idx[R.D_DUP, 0] == R.D_DUP_OF and abs(dist[R.D_DUP_OF, 0]) <= 1e-6
    for i in range(N):
        if i in (R.D_DUP, R.D_DUP_OF, R.D_ZERO):                                                 # (the zero row: every distance ties, checked above)
            continue
        row = idx[i].tolist()
        a, b = row.index(R.D_DUP_OF), row.index(R.D_DUP)
        assert b == a + 1 and dist[i, a] == dist[i, b]                                            # equal distances: the lower index first
        assert dist[i, row.index(R.D_ZERO)] == 1.0
    assert np.abs(dist - R.knn("D")[1]).max() <= 1e-5


# ---- 2. conditional p -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["A", "B", "C"])
def test_conditional_p(label):
    from act_amd import kernels as K
    _, _, perp, _ = R.problem(label)
    _, rdist, rp = R.affinities(label)[:3]
    p = K.tsne_conditional_p(_dev(rdist, np.float32), perp).cpu().numpy().astype(np.float64)
    got = R.row_perplexity(p)
    worst = (np.abs(p - rp) / rp.max(1, keepdims=True)).max()
    print(f"{label}: max |row sum - 1| = {np.abs(p.sum(1) - 1).max():.2e}, max relative perplexity error = {np.abs(got / perp - 1).max():.2e}, "
          f"max |p - ref| / row max = {worst:.2e}")
    assert np.abs(p.sum(1) - 1).max() <= 1e-6
    assert np.abs(got / perp - 1).max() <= 1e-4
    assert worst <= 1e-4


# ---- 3. CSR -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["A", "B", "C", "D"])
def test_symmetrize_pattern_values_and_determinism(label):
    from act_amd import kernels as K
    _, _, perp, _ = R.problem(label)
    ridx, rdist, _ = R.knn(label)
    p = K.tsne_conditional_p(_dev(rdist, np.float32), perp)
    idx = _dev(ridx)
    indptr, indices, values = K.tsne_symmetrize(idx, p)
    again = K.tsne_symmetrize(idx, p)
    _, rptr, rind, rval = R.symmetrize(ridx, p.cpu().numpy())
    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32
    assert np.array_equal(indptr.cpu().numpy(), rptr) and np.array_equal(indices.cpu().numpy(), rind)
    v = values.cpu().numpy().astype(np.float64)
    print(f"{label}: nnz = {len(v)}, max relative value error = {(np.abs(v - rval) / np.maximum(rval, 1e-300))[rval > 0].max():.2e}")
    assert np.all(np.abs(v - rval) <= 1e-6 * rval)
    assert abs(v.sum() - 1) <= 1e-5
    for a, b in zip((indptr, indices, values), again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 4. gradient and step ---------------------------------------------------------------------------------------------------------------------
def _close(dev, ref, alternatives, small, what):
    """element-wise to 1e-4 of max |ref|; where the reference gradient vanishes either gain branch is legitimate"""
    tol = 1e-4 * np.abs(ref).max()
    err = np.abs(dev - ref)
    print(f"    {what}: max error / max |.| = {err[~small].max() / np.abs(ref).max():.2e}")
    assert np.all(err[~small] <= tol), what
    if small.any():
        assert np.all(np.min([np.abs(dev - alt) for alt in alternatives], axis=0)[small] <= tol), what


@pytest.mark.parametrize("exaggeration", [12.0, 1.0])
@pytest.mark.parametrize("state", [0, 1])
@pytest.mark.parametrize("label", ["A", "B", "C"])
def test_one_step_and_kl(label, state, exaggeration):
    from act_amd import kernels as K
    csr, P = _csr32(label)
    N = P.shape[0]
    Y0, U0, G0 = (a.astype(np.float32) for a in R.embeddings(label)[state])
    mom, lr = 0.8, np.float32(R.learning_rate(N))
    Y, U, G = _dev(Y0), _dev(U0), _dev(G0)
    kl_dev = float(K.tsne_kl(csr, Y))
    kl_ref = R.kl(P, Y0)
    print(f"{label} state {state} ex {exaggeration}: KL {kl_dev:.9f} vs {kl_ref:.9f} (relative {abs(kl_dev / kl_ref - 1):.2e})")
    assert abs(kl_dev - kl_ref) <= 1e-6 * abs(kl_ref)
    K.tsne_step(csr, Y, U, G, exaggeration, mom, lr)
    Yr, Ur, Gr, g = R.step(P, Y0, U0, G0, exaggeration, mom, float(lr))
    Y0, U0, G0 = (a.astype(np.float64) for a in (Y0, U0, G0))
    small = np.abs(g) < 1e-6 * np.abs(g).max()
    assert small.mean() <= FLIP_SHARE
    alts_u, alts_y = [], []
    for gains in (np.maximum(G0 + 0.2, 0.01), np.maximum(G0 * 0.8, 0.01)):
        u = mom * U0 - float(lr) * gains * g
        y = Y0 + u
        alts_u.append(u); alts_y.append(y - (Y0 + Ur).mean(0))
    _close(U.cpu().numpy(), Ur, alts_u, small, "update")
    _close(Y.cpu().numpy(), Yr, alts_y, small, "Y")
    assert np.abs(Y.cpu().numpy().astype(np.float64).mean(0)).max() <= 1e-6 * np.abs(Yr).max()


# ---- 5. ten steps -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["A", "B"])
def test_ten_steps_in_one_call(label):
    from act_amd import kernels as K
    csr, P = _csr32(label)
    N = P.shape[0]
    Y0, U0, G0 = (a.astype(np.float32) for a in R.embeddings(label)[0])
    lr = np.float32(R.learning_rate(N))
    one = [_dev(Y0), _dev(U0), _dev(G0)]
    for _ in range(10):
        K.tsne_step(csr, *one, 12.0, 0.5, lr)
    ten = [_dev(Y0), _dev(U0), _dev(G0)]
    K.tsne_steps(csr, *ten, 10, 12.0, 0.5, lr)
    for a, b in zip(one, ten):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    Yr, Ur, Gr = Y0.astype(np.float64), U0.astype(np.float64), G0.astype(np.float64)
    for _ in range(10):
        Yr, Ur, Gr, _ = R.step(P, Yr, Ur, Gr, 12.0, 0.5, float(lr))
    for dev, ref, what in ((ten[0], Yr, "Y"), (ten[1], Ur, "update")):
        off = np.abs(dev.cpu().numpy() - ref) > 1e-4 * np.abs(ref).max()
        print(f"{label} {what}: {off.mean():.2e} of the elements beyond 1e-4 of max |.|")
        assert off.mean() <= FLIP_SHARE


# ---- 6. PCA initialisation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["A", "B"])
def test_pca_initialisation(label):
    from act_amd import kernels as K
    X = R.problem(label)[0]
    Yr, lam = R.pca_init(X)
    Y, info = K.tsne_pca_init(_dev(X), want_info=True)
    Y, info = Y.cpu().numpy().astype(np.float64), info.cpu().numpy()
    err = np.abs(Y - Yr).max(0) / np.sqrt((Yr * Yr).sum(0))
    print(f"{label}: lambda2/lambda1 = {lam[1] / lam[0]:.4f}, lambda3/lambda2 = {lam[2] / lam[1]:.4f}, sweeps = {int(info[2])}, last change = {info[3]:.1e}, "
          f"max column error / column norm = {err.max():.2e}, eigenvalue errors = {abs(info[0] / lam[0] - 1):.1e} {abs(info[1] / lam[1] - 1):.1e}")
    assert np.all(err <= 1e-4)
    assert abs(Y[:, 0].std() / 1e-4 - 1) <= 1e-5


# ---- 7. whole fit -----------------------------------------------------------------------------------------------------------------------------
def test_whole_fit_against_the_reference_noise_floor():
    """t-SNE trajectories are chaotic, so the bar is not an element-wise match but the reference's own spread over five orderings of problem A
    (exact arithmetic is permutation-equivariant)."""
    from act_amd.utils.tsne import TSNE
    X, y, perp, _ = R.problem("A")
    N = X.shape[0]
    kls, agr = R.fit_floor()
    P = R.affinities("A")[3]
    (n0, ex, m0), (n1, _, m1) = R.FIT_SCHEDULE
    init = _dev(R.fit_init(N), np.float32)
    fits = []
    for _ in range(2):
        t = TSNE(perplexity=perp, early_exaggeration=ex, early_exaggeration_iter=n0, n_iter=n1, initial_momentum=m0, final_momentum=m1,
                 initialization=init)
        fits.append((t.fit(_dev(X)), t))
    Y, t = fits[0]
    assert Y.shape == (N, 2) and Y.dtype == torch.float32 and Y.is_cuda and t.n_iter_ == n0 + n1 and len(t.affinities_) == 3
    assert torch.equal(Y.view(torch.int32), fits[1][0].view(torch.int32)) and t.kl_divergence_ == fits[1][1].kl_divergence_
    Yh = Y.cpu().numpy().astype(np.float64)
    kl, agreement = R.kl(P, Yh), R.knn_label_agreement(Yh, y)
    print(f"reference KL over five orderings: {['%.4f' % v for v in kls]}, 10-NN agreement {['%.4f' % v for v in agr]}; "
          f"device KL {kl:.4f} (its own figure {t.kl_divergence_:.4f}), agreement {agreement:.4f}")
    assert abs(t.kl_divergence_ - kl) <= 1e-4 * kl                  # the device's P is fp32 and comes from its own kNN and search
    assert kl <= max(kls) + (max(kls) - min(kls))
    assert agreement >= min(agr) - 0.02


# ---- 8. runner --------------------------------------------------------------------------------------------------------------------------------
def test_runner_writes_both_plots(tmp_path, monkeypatch):
    from act_amd.tools import tsne_run_net
    from act_amd.tools import runner_tsne as RT
    from act_amd.utils.config import cfg_from_yaml_file
    config = cfg_from_yaml_file("cfgs/synthetic/tsne_modelnet.yaml")
    base = config.dataset.test._base_
    base.NUM_SAMPLES, base.NUM_CATEGORY, base.N_POINTS = 64, 4, 2048
    for m in (config.model_pretrained, config.model_finetuned):
        m.cls_dim = 4
    seen = []
    real_plot = RT.tsne_utils.plot_tsne

    def spy(x, y, **kw):
        seen.append((tuple(x.shape), int(y.numel()), x.is_cuda))
        return real_plot(x, y, **kw)
    monkeypatch.setattr(RT.tsne_utils, "plot_tsne", spy)
    args = argparse.Namespace(log_name="test_tsne", use_gpu=True, local_rank=0, distributed=False, num_workers=0, world_size=1,
                              experiment_path=str(tmp_path), ckpts_pretrained="none", ckpts_finetuned="none", perplexity=5,
                              tsne_dir=str(tmp_path / "tsne"), tsne_name="synthetic")
    torch.manual_seed(0)
    with pytest.warns(UserWarning, match="RANDOMLY INITIALISED"):
        out = tsne_run_net(args, config)
    assert 0.0 <= out["acc"] <= 100.0 and out["n_correct"] == round(out["acc"] * 64 / 100) >= 4
    assert seen == [((out["n_correct"], 2), out["n_correct"], True)] * 2
    for which, path in zip(("pretrained", "finetuned"), out["files"]):
        stem = str(tmp_path / "tsne" / f"synthetic_{which}.png")
        assert path in (stem, stem + ".txt") and os.path.getsize(path) > 0
        if path.endswith(".txt"):
            assert np.loadtxt(path).shape == (out["n_correct"], 3)
    assert all(np.isfinite(v) for v in out["kl"])


def test_forward_features_is_the_same_forward():
    from act_amd.models import build_model_from_cfg
    from act_amd.utils.config import cfg_from_yaml_file
    config = cfg_from_yaml_file("cfgs/synthetic/tsne_modelnet.yaml")
    torch.manual_seed(1)
    model = build_model_from_cfg(config.model_finetuned).to(DEV).eval()
    pts = torch.randn(3, 1024, 3, device=DEV)
    with torch.no_grad():
        logits, f = model.forward_features(pts)
        assert torch.equal(logits.view(torch.int32), model(pts).view(torch.int32))
    assert f.shape == (3, 2 * config.model_finetuned.embed_dim) and logits.shape == (3, 40)


# ---- 9. errors --------------------------------------------------------------------------------------------------------------------------------
def test_fit_refuses_what_it_cannot_embed():
    from act_amd._C import ActHipError
    from act_amd.utils.tsne import TSNE
    x = torch.randn(32, 8, device=DEV)
    with pytest.raises(ActHipError):
        TSNE(perplexity=5).fit(x.cpu())
    with pytest.raises(ActHipError):
        TSNE(perplexity=5).fit(x[:3])
    with pytest.raises(ActHipError):
        TSNE(perplexity=0).fit(x)
    bad = x.clone()
    bad[4, 2] = float("nan")
    with pytest.raises(ActHipError):
        TSNE(perplexity=5).fit(bad)
    with pytest.raises(ActHipError):
        TSNE(perplexity=5, metric="euclidean")
