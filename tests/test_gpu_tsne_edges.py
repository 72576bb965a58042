"""GPU: csrc/tsne.hip at the sizes where its loops take a second round -- k past one wave and up to TSNE_MAXK, N past one scan chunk, in-lists past
one staging chunk, repulsion splits of 128 and 320 points with ragged tails, more than 64 partials in every list sum, D past one round of the
eigenvector kernel and up to its LDS panels, split-K covariance -- against the float64 numpy restatement of tests/tsne_ref.py.  The bars are those
of tests/test_gpu_tsne.py for the same stage; every test prints what it measured before it asserts."""
import functools

import numpy as np
import pytest
import torch

from tests import tsne_ref as R
from tests.test_gpu_tsne import FLIP_SHARE, _close, _dev

pytestmark = pytest.mark.gpu

# (N, D, k, seed): three slabs of 512 + 512 + 76 rows on the float4 path; the scalar path with a ragged last k-tile (1023 = 31 * 32 + 31); four
# rounds of the output loop; exactly TSNE_MAXK
KNN_CASES = [(1100, 384, 90, 21), (1300, 1023, 300, 22), (1300, 260, 1023, 23), (1100, 64, 1024, 24)]
KNN_IDS = ["1100x384k90", "1300x1023k300", "1300x260k1023", "1100x64k1024"]
RUNNER = (2468, 768, 90, 25)                # ModelNet40's test split, the wider feature, the default perplexity of 30
UNIFORM_ROW = 5


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _knn_case(case):
    """-> (X, reference idx, dist, gap)"""
    N, D, k, seed = case
    X = R.make_lowrank(N, D, 40 if case == RUNNER else 8, seed, 1.0)[0]
    return _frozen(X, *R.knn_of(X, k))


def _check_knn(X, k, ridx, rdist, gap, what):
    """the assertions of test_gpu_tsne.test_knn_sets_and_distances -> (idx, dist) of the device"""
    from act_amd import kernels as K
    N = X.shape[0]
    decided = gap > 1e-5                                     # a smaller gap cannot be decided by fp32 products
    assert (~decided).mean() <= 0.02                         # a property of the inputs: before the device is consulted
    idx, dist = K.tsne_knn_cosine(_dev(X), k)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert idx.dtype == np.int32 and idx.shape == (N, k) and dist.shape == idx.shape
    print(f"{what}: {int((~decided).sum())} of {N} rows left out; max |dist - ref| = {np.abs(dist - rdist)[decided].max():.2e} (bar 1e-5)")
    assert np.array_equal(np.sort(idx[decided], axis=1), np.sort(ridx[decided], axis=1))
    assert np.all(idx != np.arange(N)[:, None])
    assert np.abs(dist - rdist)[decided].max() <= 1e-5 and np.all(np.diff(dist, axis=1) >= 0)
    return idx, dist


# ---- 1. kNN -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KNN_CASES, ids=KNN_IDS)
def test_knn_past_one_slab_one_k_tile_and_one_output_round(case):
    X, ridx, rdist, gap = _knn_case(case)
    _check_knn(X, case[2], ridx, rdist, gap, f"N, D, k = {case[:3]}")


def test_knn_ties_across_a_slab_edge_and_a_zero_row_in_the_last_slab():
    """the assertions of test_knn_clamp_self_ties_and_zero_row at three slabs and k = TSNE_MAXK: rows 511 and 512 (the last of the first slab, the
    first of the second) are equal, so are two rows of the last slab, and a row of the last slab is zero"""
    N, D, k = 1100, 384, 1024
    pairs, zero = ((511, 512), (1030, 1090)), 1050
    X = R.make_lowrank(N, D, 8, 31, 1.0)[0]
    for a, b in pairs:
        X[b] = X[a]
    X[zero] = 0
    ridx, rdist, gap = R.knn_of(X, k)
    idx, dist = _check_knn(X, k, ridx, rdist, gap, "planted ties")
    assert np.abs(dist - rdist).max() <= 1e-5                                                      # sorted values: every row, decided or not
    assert np.array_equal(idx[zero], np.array([j for j in range(N) if j != zero][:k])) and np.all(dist[zero] == 1.0)
    special = {zero} | {i for p in pairs for i in p}
    both = 0
    for a, b in pairs:
        assert idx[a, 0] == b and idx[b, 0] == a and abs(dist[a, 0]) <= 1e-6 and abs(dist[b, 0]) <= 1e-6
    for i in range(N):
        if i in special:
            continue
        row = idx[i].tolist()
        for a, b in pairs:
            if b in row:                                                                           # equal distances: the lower index first
                assert row.index(b) == row.index(a) + 1 and dist[i, row.index(a)] == dist[i, row.index(b)]
                both += 1
            elif a in row:                                                                         # the pair straddles k: the lower index is in
                assert row.index(a) == k - 1
        if zero in row:
            assert dist[i, row.index(zero)] == 1.0
    with_zero = int((idx == zero).any(1).sum())
    print(f"planted ties: {both} (row, pair) lists hold both members, {with_zero} rows list the zero row")
    assert both >= N and with_zero >= N // 2


def test_knn_refuses_k_past_the_limit_and_k_equal_to_n():
    from act_amd import kernels as K
    from act_amd._C import ActHipError
    x = _dev(_knn_case(KNN_CASES[3])[0])
    with pytest.raises(ActHipError):
        K.tsne_knn_cosine(x, 1025)
    with pytest.raises(ActHipError):
        K.tsne_knn_cosine(x[:600].contiguous(), 600)
    assert K.tsne_knn_cosine(x[:600].contiguous(), 599)[0].shape == (600, 599)


# ---- 2. conditional p -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cond_p_case(case):
    """the reference distances of a kNN case as the device gets them (fp32), one row made constant -> (dist fp32, perplexity, reference p)"""
    k = case[2]
    d32 = _knn_case(case)[2].astype(np.float32)
    d32[UNIFORM_ROW] = d32[UNIFORM_ROW, 0]
    perp = min(k // 3, 341)
    return _frozen(d32, np.float64(perp), R.conditional_p(d32.astype(np.float64), perp)[0])


@pytest.mark.parametrize("case", KNN_CASES, ids=KNN_IDS)
def test_conditional_p_past_one_wave_of_neighbours(case):
    """k = 90, 300, 1023, 1024: 2, 5 and 16 rounds of the lane loop, the last one ragged but for 1024"""
    from act_amd import kernels as K
    d32, perp, rp = _cond_p_case(case)
    perp, k = float(perp), d32.shape[1]
    p32 = K.tsne_conditional_p(_dev(d32), perp).cpu().numpy()
    p = p32.astype(np.float64)
    rows = np.arange(len(p)) != UNIFORM_ROW                  # a constant row has perplexity k whatever beta is
    got = R.row_perplexity(p)
    worst = (np.abs(p - rp) / rp.max(1, keepdims=True)).max()
    print(f"k = {k}, perplexity {perp:.0f}: max |row sum - 1| = {np.abs(p.sum(1) - 1).max():.2e} (bar 1e-6), max relative perplexity error = "
          f"{np.abs(got / perp - 1)[rows].max():.2e} (bar 1e-4), max |p - ref| / row max = {worst:.2e} (bar 1e-4)")
    assert np.all(np.isfinite(p32)) and np.all(p32[UNIFORM_ROW] == np.float32(1.0 / k))
    assert np.abs(p.sum(1) - 1).max() <= 1e-6
    assert np.abs(got / perp - 1)[rows].max() <= 1e-4
    assert worst <= 1e-4


# ---- 3. CSR -----------------------------------------------------------------------------------------------------------------------------------
HUBS = {7: 1299, 650: 600, 1000: 0}          # in-lists of two 1024-entry passes and six 256-row rounds, of three rounds, and an empty one


@functools.lru_cache(maxsize=None)
def _table(name):
    if name == "knn1100k90":
        idx = _knn_case(KNN_CASES[0])[1]
    elif name == "knn1300k300":
        idx = _knn_case(KNN_CASES[1])[1]
    elif name == "random1100k1024":
        r = np.random.default_rng(41).random((1100, 1100))
        np.fill_diagonal(r, np.inf)
        idx = np.argsort(r, axis=1)[:, :1024].astype(np.int32)
    elif name == "hubs1300k5":
        idx = R.hub_idx(1300, 5, HUBS)
    else:
        idx = _knn_case(RUNNER)[1]
    N, k = idx.shape
    p = np.random.default_rng(42).uniform(0.5, 1.5, (N, k))
    p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    return _frozen(np.ascontiguousarray(idx), p)


@pytest.mark.parametrize("name", ["knn1100k90", "knn1300k300", "random1100k1024", "hubs1300k5", "runner2468k90"])
def test_symmetrize_past_one_scan_chunk_and_one_list_chunk(name):
    from act_amd import kernels as K
    ridx, p32 = _table(name)
    N, k = ridx.shape
    indeg = np.bincount(ridx.ravel(), minlength=N)
    if name == "hubs1300k5":
        assert indeg[7] == 1299 > 1024 and 256 < indeg[650] <= 1024 and indeg[1000] == 0
    idx, p = _dev(ridx), _dev(p32)
    indptr, indices, values = K.tsne_symmetrize(idx, p)
    again = K.tsne_symmetrize(idx, p)
    _, rptr, rind, rval = R.symmetrize(ridx, p32)
    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32
    assert np.array_equal(indptr.cpu().numpy(), rptr) and np.array_equal(indices.cpu().numpy(), rind)
    v = values.cpu().numpy().astype(np.float64)
    print(f"{name}: scan chunk {-(-N // 1024)}, largest in-list {indeg.max()}, nnz = {len(v)}, max relative value error = "
          f"{(np.abs(v - rval) / rval).max():.2e} (bar 1e-6), |sum - 1| = {abs(v.sum() - 1):.2e} (bar 1e-5)")
    assert np.all(rval > 0) and np.all(np.abs(v - rval) <= 1e-6 * rval)
    assert abs(v.sum() - 1) <= 1e-5
    for a, b in zip((indptr, indices, values), again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 4. gradient, step and KL -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _csr(N):
    """-> (indptr, indices, fp32 values, the float64 of those fp32 values)"""
    indptr, indices, values = R.random_csr(N, 80, N)
    assert (np.diff(indptr) > 64).mean() > 0.5
    v32 = values.astype(np.float32)
    return _frozen(indptr, indices, v32, v32.astype(np.float64))


@functools.lru_cache(maxsize=None)
def _state(N, which):
    """-> (Y, update, gains in fp32, the all-pairs sums of that fp32 Y in float64: the one block pass of this (N, state))"""
    Y, U, G = (a.astype(np.float32) for a in R.edge_state(N, which))
    R_, Z = R.repulsion(Y)
    return _frozen(Y, U, G, R_) + (Z,)


# N = 1100: 90 partials of Z, 69 of the centre.  N = 4200: splits of 128 points, the last holds 104 (sub-chunks of 64 and 40).  N = 8200: splits
# of 320 (staging rounds of 256 and 64), the last holds 200 (sub-chunks 64, 64, 64, 8)
@pytest.mark.parametrize("N,state,exaggeration", [(1100, 0, 12.0), (1100, 0, 1.0), (1100, 1, 12.0), (1100, 1, 1.0), (4200, 0, 12.0), (4200, 1, 1.0),
                                                  (8200, 0, 12.0), (8200, 1, 1.0)])
def test_one_step_and_kl_past_one_repulsion_chunk(N, state, exaggeration):
    from act_amd import kernels as K
    indptr, indices, v32, v64 = _csr(N)
    Y0, U0, G0, Rp, Z = _state(N, state)
    pairs = (Rp, Z)
    csr = (_dev(indptr), _dev(indices), _dev(v32))
    mom, lr = 0.8, np.float32(R.learning_rate(N))
    Y, U, G = _dev(Y0), _dev(U0), _dev(G0)
    kl_dev = float(K.tsne_kl(csr, Y))
    kl_ref = R.kl_csr(indptr, indices, v64, Y0, pairs=pairs)
    print(f"N {N} state {state} ex {exaggeration}: KL {kl_dev:.9f} vs {kl_ref:.9f} (relative {abs(kl_dev / kl_ref - 1):.2e}, bar 1e-6)")
    assert abs(kl_dev - kl_ref) <= 1e-6 * abs(kl_ref)
    K.tsne_step(csr, Y, U, G, exaggeration, mom, lr)
    Yr, Ur, Gr, g = R.step_csr(indptr, indices, v64, Y0, U0, G0, exaggeration, mom, float(lr), pairs=pairs)
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
    centre = np.abs(Y.cpu().numpy().astype(np.float64).mean(0)).max()
    print(f"    |mean Y| / max |Y| = {centre / np.abs(Yr).max():.2e} (bar 1e-6)")
    assert centre <= 1e-6 * np.abs(Yr).max()


def test_ten_steps_in_one_call_at_90_partials():
    from act_amd import kernels as K
    N = 1100
    indptr, indices, v32, _ = _csr(N)
    csr = (_dev(indptr), _dev(indices), _dev(v32))
    Y0, U0, G0 = _state(N, 1)[:3]
    lr = np.float32(R.learning_rate(N))
    one = [_dev(Y0), _dev(U0), _dev(G0)]
    for _ in range(10):
        K.tsne_step(csr, *one, 12.0, 0.5, lr)
    ten = [_dev(Y0), _dev(U0), _dev(G0)]
    K.tsne_steps(csr, *ten, 10, 12.0, 0.5, lr)
    assert not torch.equal(ten[0], _dev(Y0))
    for a, b in zip(one, ten):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 5. PCA initialisation ----------------------------------------------------------------------------------------------------------------------
# (N, D, seed): split-K 2 and two rounds of every loop of the eigenvector kernel; its LDS panels full; split-K 8 and one column past one round
@pytest.mark.parametrize("N,D,seed", [(1100, 384, 21), (600, 1024, 26), (4200, 257, 27)])
def test_pca_initialisation_past_one_round_of_features(N, D, seed):
    from act_amd import kernels as K
    X = R.make_lowrank(N, D, 8, seed, 1.0)[0]
    Yr, lam = R.pca_init(X)
    assert lam[1] / lam[0] <= 0.9 and lam[2] / lam[1] <= 0.9                                       # of the inputs: the two axes are determined
    Y, info = K.tsne_pca_init(_dev(X), want_info=True)
    Y, info = Y.cpu().numpy().astype(np.float64), info.cpu().numpy()
    err = np.abs(Y - Yr).max(0) / np.sqrt((Yr * Yr).sum(0))
    print(f"N, D = {N}, {D}: lambda2/lambda1 = {lam[1] / lam[0]:.4f}, lambda3/lambda2 = {lam[2] / lam[1]:.4f}, sweeps = {int(info[2])}, "
          f"last change = {info[3]:.1e}, max column error / column norm = {err.max():.2e} (bar 1e-4), eigenvalue errors = "
          f"{abs(info[0] / lam[0] - 1):.1e} {abs(info[1] / lam[1] - 1):.1e}, |std / 1e-4 - 1| = {abs(Y[:, 0].std() / 1e-4 - 1):.1e} (bar 1e-5)")
    assert np.all(err <= 1e-4)
    assert abs(Y[:, 0].std() / 1e-4 - 1) <= 1e-5


def test_pca_initialisation_refuses_a_width_past_its_panels():
    from act_amd import kernels as K
    from act_amd._C import ActHipError
    with pytest.raises(ActHipError):
        K.tsne_pca_init(torch.randn(64, 1025, device="cuda:0"))


# ---- 6. the runner's shape, end to end ----------------------------------------------------------------------------------------------------------
def test_fit_at_the_runner_shape():
    """2468 x 768 at the default perplexity (k = 90) through the public fit: finite, centred, better than where it started, the same twice.  (An
    element-wise comparison with a float64 trajectory is not made: it is chaotic, and test_gpu_tsne.py bounds it on problem A.)"""
    from act_amd import kernels as K
    from act_amd.utils.tsne import TSNE
    x = _dev(_knn_case(RUNNER)[0])
    fits = []
    for _ in range(2):
        t = TSNE(perplexity=30)
        fits.append((t.fit(x), t))
    Y, t = fits[0]
    assert Y.shape == (RUNNER[0], 2) and Y.dtype == torch.float32 and t.n_iter_ == 750
    assert t.affinities_[0].shape == (RUNNER[0] + 1,) and int(torch.diff(t.affinities_[0]).min()) >= RUNNER[2]
    Yh = Y.cpu().numpy().astype(np.float64)
    kl_start = float(K.tsne_kl(t.affinities_, K.tsne_pca_init(x)))
    print(f"KL {t.kl_divergence_:.4f} after the fit, {kl_start:.4f} at the PCA start; |mean Y| / max |Y| = "
          f"{np.abs(Yh.mean(0)).max() / np.abs(Yh).max():.2e} (bar 1e-6)")
    assert np.all(np.isfinite(Yh)) and np.isfinite(t.kl_divergence_)
    assert np.abs(Yh.mean(0)).max() <= 1e-6 * np.abs(Yh).max()
    assert t.kl_divergence_ < kl_start
    assert torch.equal(Y.view(torch.int32), fits[1][0].view(torch.int32)) and t.kl_divergence_ == fits[1][1].kl_divergence_
