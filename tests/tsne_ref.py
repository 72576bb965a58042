"""Shared pieces of the t-SNE tests: the generated problems and a float64 numpy restatement of every stage of csrc/tsne.hip -- cosine kNN by
stable argsort, the perplexity bisection, the dense symmetrisation and its CSR pattern, the gradient, one step, KL, the PCA initialisation by
numpy.linalg.eigh, a whole fit.  Everything is computed once per process.

The second half serves tests/test_gpu_tsne_edges.py: low-rank features for sizes at which isotropic data has no decidable neighbour sets, kNN of an
array, the gradient / KL / step along a CSR with the all-pairs part taken over row blocks (no N x N x 2 array), a random symmetric CSR and a
neighbour table with chosen in-degrees."""
import functools

import numpy as np


def make(N, D, K, seed, sep):
    """the draws of svm_ref.make, without its scale argument"""
    r = np.random.default_rng(seed)
    mu = r.normal(size=(K, D)) * sep
    y = r.integers(0, K, N)
    X = (mu[y] + r.normal(size=(N, D))).astype(np.float32)
    return X, y.astype(np.int64)


# label -> (N, D, K, seed, sep, perplexity); k = min(N - 1, 3 perplexity)
CASES = {"A": (257, 33, 5, 0, 1.0, 10), "B": (515, 48, 7, 1, 0.6, 10), "C": (40, 16, 3, 2, 1.0, 5)}
D_DUP, D_DUP_OF, D_ZERO = 5, 2, 13            # problem D: row 5 repeats row 2, row 13 is zero


def n_neighbors(N, perplexity):
    return min(N - 1, 3 * int(perplexity))


@functools.lru_cache(maxsize=None)
def problem(label):
    """-> (X float32 [N,D], labels, perplexity, k)"""
    if label == "D":
        X = np.random.default_rng(3).normal(size=(20, 8)).astype(np.float32)
        X[D_DUP] = X[D_DUP_OF]
        X[D_ZERO] = 0
        y, perp = np.zeros(20, np.int64), 10
    else:
        N, D, K, seed, sep, perp = CASES[label]
        X, y = make(N, D, K, seed, sep)
    X.setflags(write=False); y.setflags(write=False)
    return X, y, perp, n_neighbors(X.shape[0], perp)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def cosine_distances(X):
    """float64 [N,N] of 1 - x^_i . x^_j; a row of zero norm has x^ = 0 (distance 1 to every row); the diagonal is +inf"""
    X = np.asarray(X, np.float64)
    n = np.sqrt((X * X).sum(1))
    Xh = X * np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)[:, None]
    Dm = 1.0 - Xh @ Xh.T
    np.fill_diagonal(Dm, np.inf)
    return Dm


@functools.lru_cache(maxsize=None)
def knn(label):
    """-> (idx int32 [N,k], dist float64 [N,k], gap float64 [N] between the k-th and the (k+1)-th distance; +inf when k = N - 1)"""
    X, _, _, k = problem(label)
    Dm = cosine_distances(X)
    order = np.argsort(Dm, axis=1, kind="stable")               # ties towards the lower index
    srt = np.take_along_axis(Dm, order, axis=1)
    gap = srt[:, k] - srt[:, k - 1] if k < X.shape[0] - 1 else np.full(X.shape[0], np.inf)
    return _frozen(order[:, :k].astype(np.int32), srt[:, :k].copy(), gap)


def conditional_p(dist, perplexity, tol=1e-10, max_steps=200):
    """per row the beta with entropy(exp(-beta (d - d_min))) = log(perplexity): beta doubles while the upper bound is open, halves while the lower one
    is, else bisects.  The device stops at tol 1e-5 / 100 steps; the default here is the tight solution it is compared with.  -> (p [N,k], beta [N])"""
    dist = np.asarray(dist, np.float64)
    N, k = dist.shape
    target = np.log(float(perplexity))
    P, betas = np.empty((N, k)), np.empty(N)
    for i in range(N):
        dd = dist[i] - dist[i].min()
        beta, lo, hi = 1.0, -np.inf, np.inf
        for step in range(max_steps):
            pv = np.exp(-beta * dd)
            s = pv.sum()
            H = np.log(s) + beta * (dd * pv).sum() / s
            diff = H - target
            if abs(diff) < tol or step == max_steps - 1:
                break
            if diff > 0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else 0.5 * (beta + hi)
            else:
                hi = beta
                beta = beta * 0.5 if lo == -np.inf else 0.5 * (beta + lo)
        P[i], betas[i] = pv / s, beta
    return P, betas


def row_perplexity(p):
    p = np.asarray(p, np.float64)
    p = p / p.sum(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        H = -np.where(p > 0, p * np.log(p), 0.0).sum(1)
    return np.exp(H)


def symmetrize(idx, p):
    """-> (P float64 [N,N] = (P_cond + P_cond^T) / 2N, indptr, indices, values of its CSR form; the pattern is structural: j in nbr(i) or i in nbr(j))"""
    idx, p = np.asarray(idx), np.asarray(p, np.float64)
    N, k = idx.shape
    C, A = np.zeros((N, N)), np.zeros((N, N), bool)
    rows = np.repeat(np.arange(N), k)
    C[rows, idx.ravel()] = p.ravel()
    A[rows, idx.ravel()] = True
    P = (C + C.T) / (2.0 * N)
    A = A | A.T
    indptr = np.concatenate([[0], np.cumsum(A.sum(1))]).astype(np.int32)
    r, c = np.nonzero(A)                                        # row-major: ascending columns within a row
    return P, indptr, c.astype(np.int32), P[r, c]


def gradient(P, Y, exaggeration=1.0):
    """-> (g [N,2] = exaggeration sum_j P_ij w_ij (y_i - y_j) - (1/Z) sum_j w_ij^2 (y_i - y_j), Z): openTSNE's convention, a quarter of dKL/dy"""
    Y = np.asarray(Y, np.float64)
    diff = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + (diff * diff).sum(2))
    np.fill_diagonal(w, 0.0)
    Z = w.sum()
    attr = ((P * w)[:, :, None] * diff).sum(1)
    rep = ((w * w)[:, :, None] * diff).sum(1) / Z
    return exaggeration * attr - rep, Z


def kl(P, Y):
    Y = np.asarray(Y, np.float64)
    diff = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + (diff * diff).sum(2))
    np.fill_diagonal(w, 0.0)
    m = P > 0
    return float((P[m] * np.log(P[m] / (w[m] / w.sum()))).sum())


def step(P, Y, update, gains, exaggeration, momentum, lr):
    """one step on float64 copies -> (Y, update, gains, g)"""
    Y, update, gains = (np.asarray(a, np.float64) for a in (Y, update, gains))
    g, _ = gradient(P, Y, exaggeration)
    flip = np.sign(g) != np.sign(update)
    gains = np.maximum(np.where(flip, gains + 0.2, gains * 0.8), 0.01)
    update = momentum * update - lr * gains * g
    Y = Y + update
    return Y - Y.mean(0), update, gains, g


def learning_rate(N):
    return max(200.0, N / 12.0)


def run(P, Y0, schedule, lr):
    """schedule: [(iterations, exaggeration, momentum), ...] -> (Y, update, gains)"""
    Y = np.array(Y0, np.float64)
    update, gains = np.zeros_like(Y), np.ones_like(Y)
    for n, ex, mom in schedule:
        for _ in range(n):
            Y, update, gains, _ = step(P, Y, update, gains, ex, mom, lr)
    return Y, update, gains


def pca_init(X):
    """-> (Y0 float64 [N,2]: projection on the two leading eigenvectors of the covariance, each signed so that its largest-magnitude entry is positive,
    scaled so that column 0 has standard deviation 1e-4; the eigenvalues of X_c^T X_c in descending order)"""
    X = np.asarray(X, np.float64)
    Xc = X - X.mean(0)
    lam, vec = np.linalg.eigh(Xc.T @ Xc)
    V = vec[:, ::-1][:, :2].copy()
    for c in range(2):
        if V[np.argmax(np.abs(V[:, c])), c] < 0:
            V[:, c] = -V[:, c]
    Y = Xc @ V
    return Y * (1e-4 / Y[:, 0].std()), lam[::-1]


def knn_label_agreement(Y, labels, k=10):
    """mean over the points of the share of a point's k nearest embedding neighbours that carry its label"""
    Y = np.asarray(Y, np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float((labels[nn] == labels[:, None]).mean())


@functools.lru_cache(maxsize=None)
def affinities(label):
    """the reference chain of a problem -> (idx, dist, p, P dense, indptr, indices, values)"""
    _, _, perp, _ = problem(label)
    idx, dist, _ = knn(label)
    p, _ = conditional_p(dist, perp)
    return _frozen(idx, dist, p, *symmetrize(idx, p))


@functools.lru_cache(maxsize=None)
def embeddings(label):
    """the two states the step tests start from: N(0, 1e-4^2), and the reference's own state after 150 iterations (100 at exaggeration 12 and
    momentum 0.5, 50 at 1 and 0.8) -> ((Y, update, gains), (Y, update, gains))"""
    X = problem(label)[0]
    N = X.shape[0]
    P = affinities(label)[3]
    Y0 = np.random.default_rng(11).normal(size=(N, 2)) * 1e-4
    Y0 -= Y0.mean(0)
    late = run(P, Y0, [(100, 12.0, 0.5), (50, 1.0, 0.8)], learning_rate(N))
    return (_frozen(Y0, np.zeros((N, 2)), np.ones((N, 2))), _frozen(*late))


FIT_SCHEDULE = [(100, 12.0, 0.5), (150, 1.0, 0.8)]


def fit_init(N):
    return np.random.default_rng(5).normal(size=(N, 2)) * 1e-4


@functools.lru_cache(maxsize=None)
def fit_floor():
    """problem A under the identity and four point permutations (exact arithmetic is permutation-equivariant, floating point is not): the reference's
    final KL and 10-NN label agreement of each run -> (kls [5], agreements [5])"""
    X, y, perp, k = problem("A")
    N = X.shape[0]
    Y0 = fit_init(N)
    kls, agr = [], []
    for s in range(5):
        perm = np.arange(N) if s == 0 else np.random.default_rng(s).permutation(N)
        Dm = cosine_distances(X[perm])
        order = np.argsort(Dm, axis=1, kind="stable")[:, :k]
        p, _ = conditional_p(np.take_along_axis(Dm, order, axis=1), perp)
        P = symmetrize(order, p)[0]
        Y, _, _ = run(P, Y0[perm], FIT_SCHEDULE, learning_rate(N))
        kls.append(kl(P, Y))
        agr.append(knn_label_agreement(Y, y[perm]))
    return tuple(kls), tuple(agr)


# ---- sizes past one wave, one scan chunk and one repulsion chunk (tests/test_gpu_tsne_edges.py) ------------------------------------------------
def make_lowrank(N, D, K, seed, sep, r=12):
    """features of rank r: the latent clusters of make(N, r, ...) with axis a scaled by 1 / sqrt(a + 1), mixed into D columns by a fixed Gaussian
    matrix.  Isotropic Gaussian rows at D >= 260 concentrate the cosine distances until more than 2 % of the rows have a k-th / (k+1)-th gap under
    1e-5; these keep that share near 1 % and separate the leading eigenvalues of the covariance.  -> (X float32 [N,D], labels)"""
    Z, y = make(N, r, K, seed, sep)
    A = np.random.default_rng(seed + 1000).normal(size=(r, D)) / np.sqrt(r)
    X = (Z.astype(np.float64) * (1.0 / np.sqrt(np.arange(1, r + 1)))) @ A
    return X.astype(np.float32), y


def knn_of(X, k):
    """knn() of an array -> (idx int32 [N,k], dist float64 [N,k], gap float64 [N])"""
    N = X.shape[0]
    Dm = cosine_distances(X)
    order = np.argsort(Dm, axis=1, kind="stable")
    srt = np.take_along_axis(Dm, order, axis=1)
    gap = srt[:, k] - srt[:, k - 1] if k < N - 1 else np.full(N, np.inf)
    return order[:, :k].astype(np.int32), srt[:, :k].copy(), gap


PAIR_BLOCK = 512


def repulsion(Y):
    """the all-pairs part of a step over blocks of PAIR_BLOCK rows -> (R [N,2] = sum_j w_ij^2 (y_i - y_j), Z = sum_{i != j} w_ij)"""
    Y = np.asarray(Y, np.float64)
    N = Y.shape[0]
    R, Z = np.empty((N, 2)), 0.0
    for b in range(0, N, PAIR_BLOCK):
        e = min(N, b + PAIR_BLOCK)
        dx, dy = Y[b:e, None, 0] - Y[None, :, 0], Y[b:e, None, 1] - Y[None, :, 1]
        w = 1.0 / (1.0 + dx * dx + dy * dy)
        w[np.arange(e - b), np.arange(b, e)] = 0.0
        Z += w.sum()
        w *= w
        R[b:e, 0], R[b:e, 1] = (w * dx).sum(1), (w * dy).sum(1)
    return R, Z


def _csr_edges(indptr, indices, Y):
    """-> (row of every entry, y_row - y_column [nnz,2], w of the pair [nnz])"""
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    diff = Y[rows] - Y[np.asarray(indices)]
    return rows, diff, 1.0 / (1.0 + (diff * diff).sum(1))


def gradient_csr(indptr, indices, values, Y, exaggeration=1.0, pairs=None):
    """gradient() with P given as a CSR; pairs: repulsion(Y) where the caller already has it -> (g [N,2], Z)"""
    Y = np.asarray(Y, np.float64)
    N = Y.shape[0]
    R, Z = repulsion(Y) if pairs is None else pairs
    rows, diff, w = _csr_edges(indptr, indices, Y)
    pw = np.asarray(values, np.float64) * w
    attr = np.stack([np.bincount(rows, pw * diff[:, c], minlength=N) for c in range(2)], axis=1)
    return exaggeration * attr - R / Z, Z


def kl_csr(indptr, indices, values, Y, pairs=None):
    Y = np.asarray(Y, np.float64)
    _, Z = repulsion(Y) if pairs is None else pairs
    _, _, w = _csr_edges(indptr, indices, Y)
    v = np.asarray(values, np.float64)
    m = v > 0
    return float((v[m] * np.log(v[m] / (w[m] / Z))).sum())


def step_csr(indptr, indices, values, Y, update, gains, exaggeration, momentum, lr, pairs=None):
    """step() with P given as a CSR -> (Y, update, gains, g)"""
    Y, update, gains = (np.asarray(a, np.float64) for a in (Y, update, gains))
    g, _ = gradient_csr(indptr, indices, values, Y, exaggeration, pairs)
    flip = np.sign(g) != np.sign(update)
    gains = np.maximum(np.where(flip, gains + 0.2, gains * 0.8), 0.01)
    update = momentum * update - lr * gains * g
    Y = Y + update
    return Y - Y.mean(0), update, gains, g


def random_csr(N, deg, seed):
    """a symmetric P of about deg entries per row from a random edge list: unordered pairs i < j coded i N + j and made unique, one positive value per
    pair, both directions sorted by code (row-major, columns ascending); the values sum to 1 -> (indptr int32 [N+1], indices int32, values)"""
    r = np.random.default_rng(seed)
    a, b = r.integers(0, N, N * deg // 2), r.integers(0, N, N * deg // 2)
    keep = a != b
    lo, hi = np.minimum(a, b)[keep].astype(np.int64), np.maximum(a, b)[keep].astype(np.int64)
    code = np.unique(lo * N + hi)
    lo, hi = code // N, code % N
    v = r.uniform(0.2, 1.8, len(code))
    both, vals = np.concatenate([lo * N + hi, hi * N + lo]), np.concatenate([v, v])
    order = np.argsort(both, kind="stable")
    both, vals = both[order], vals[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(both // N, minlength=N))]).astype(np.int32)
    return indptr, (both % N).astype(np.int32), vals / vals.sum()


def hub_idx(N, k, hubs, seed=0):
    """a neighbour table int32 [N,k] of distinct non-self indices in which row h is named by exactly hubs[h] other rows (the hubs[h] lowest-numbered
    ones), for every h in hubs; the rest of every row is drawn from the rows that are not in hubs"""
    r = np.random.default_rng(seed)
    rows = [[] for _ in range(N)]
    for h, deg in hubs.items():
        assert 0 <= deg <= N - 1
        for s in [i for i in range(N) if i != h][:deg]:
            rows[s].append(h)
    free = np.array([i for i in range(N) if i not in hubs])
    out = np.empty((N, k), np.int32)
    for i in range(N):
        assert len(rows[i]) <= k
        pool = free[free != i]
        row = np.concatenate([np.array(rows[i], np.int64), r.choice(pool, k - len(rows[i]), replace=False)])
        out[i] = r.permutation(row)
    return out


def edge_state(N, which):
    """the states the large step tests start from -> (Y, update, gains), centred Y: 0 = N(0, 1e-4^2), no update, unit gains (the first iteration);
    1 = N(0, 3^2), so that w covers (0, 1], updates N(0, 0.05^2) of either sign and gains between the floor 0.01 and 4"""
    r = np.random.default_rng(100 + which)
    Y = r.normal(size=(N, 2)) * (1e-4 if which == 0 else 3.0)
    Y -= Y.mean(0)
    if which == 0:
        return Y, np.zeros((N, 2)), np.ones((N, 2))
    return Y, r.normal(size=(N, 2)) * 0.05, np.maximum(r.uniform(-0.2, 4.0, size=(N, 2)), 0.01)
