"""CPU: the float64 t-SNE reference of tests/tsne_ref.py checked against its own definitions (no package is an authority), and the text fallback of
utils.tsne_utils.plot_tsne."""
import builtins

import numpy as np
import pytest

from tests import tsne_ref as R


@pytest.mark.parametrize("label", ["A", "B", "C"])
def test_conditional_p_has_the_target_perplexity(label):
    _, _, perp, k = R.problem(label)
    p = R.affinities(label)[2]
    assert p.shape[1] == k == min(p.shape[0] - 1, 3 * perp)
    assert np.abs(p.sum(1) - 1).max() < 1e-12
    got = R.row_perplexity(p)
    print(f"{label}: max |2^H - perplexity| = {np.abs(got - perp).max():.2e}")
    assert np.abs(got - perp).max() < 1e-6


@pytest.mark.parametrize("label", ["A", "B", "C"])
def test_joint_p_is_symmetric_and_sums_to_one(label):
    idx, _, p, P, indptr, indices, values = R.affinities(label)
    assert np.array_equal(P, P.T) and abs(P.sum() - 1) < 1e-12
    N = P.shape[0]
    assert indptr[0] == 0 and indptr[-1] == len(indices) == len(values)
    for i in (0, N // 2, N - 1):
        cols = indices[indptr[i]:indptr[i + 1]]
        assert np.all(np.diff(cols) > 0) and set(idx[i]) <= set(cols) and i not in cols
        assert np.array_equal(values[indptr[i]:indptr[i + 1]], P[i, cols])


@pytest.mark.parametrize("label", ["A", "C"])
def test_gradient_is_a_quarter_of_the_kl_gradient(label):
    """central differences of KL(P || Q(Y)) against 4 g (openTSNE's g drops the factor 4), on 12 coordinates"""
    P = R.affinities(label)[3]
    N = P.shape[0]
    Y = np.random.default_rng(7).normal(size=(N, 2))
    g, _ = R.gradient(P, Y, 1.0)
    r = np.random.default_rng(8)
    h, worst = 1e-5, 0.0
    for i, c in zip(r.integers(0, N, 12), r.integers(0, 2, 12)):
        Yp, Ym = Y.copy(), Y.copy()
        Yp[i, c] += h; Ym[i, c] -= h
        num = (R.kl(P, Yp) - R.kl(P, Ym)) / (2 * h)
        worst = max(worst, abs(num - 4 * g[i, c]) / np.abs(4 * g).max())
    print(f"{label}: max |central difference - 4 g| / max |4 g| = {worst:.2e}")
    assert worst < 1e-6


def test_a_step_leaves_the_embedding_centred_and_follows_the_gain_rule():
    P = R.affinities("C")[3]
    N = P.shape[0]
    r = np.random.default_rng(9)
    Y, upd, gains = r.normal(size=(N, 2)), r.normal(size=(N, 2)) * 0.1, np.full((N, 2), 0.011)
    Y2, upd2, gains2, g = R.step(P, Y, upd, gains, 12.0, 0.5, 200.0)
    assert np.abs(Y2.mean(0)).max() < 1e-14
    flip = np.sign(g) != np.sign(upd)
    assert flip.any() and (~flip).any()
    assert np.allclose(gains2[flip], 0.211) and np.all(gains2[~flip] == 0.01)          # 0.011 * 0.8 is under the floor
    assert np.allclose(upd2, 0.5 * upd - 200.0 * gains2 * g)


def test_plot_tsne_writes_its_text_fallback(tmp_path, monkeypatch):
    from act_amd.utils import tsne_utils
    real_import = builtins.__import__

    def no_matplotlib(name, *a, **k):
        if name.split(".")[0] == "matplotlib":
            raise ImportError(name)
        return real_import(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_matplotlib)
    x = np.random.default_rng(0).normal(size=(17, 2)).astype(np.float32)
    y = np.arange(17) % 5
    target = tmp_path / "sub" / "points.png"
    path = tsne_utils.plot_tsne(x, y, filename=str(target))
    assert path == str(target) + ".txt" and not target.exists()
    rows = np.loadtxt(path)
    assert rows.shape == (17, 3) and np.array_equal(rows[:, 2], y) and np.allclose(rows[:, :2], x, rtol=1e-7)
