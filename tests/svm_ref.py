"""Shared pieces of the linear-SVM tests: the generated problems, the float64 objective of liblinear's L2-regularised L2-loss SVC (one-vs-rest, the
bias regularised as the appended constant feature) with its gradient, and the sklearn oracles.  Everything is computed once per process."""
import functools

import numpy as np


def make(N, D, K, seed, sep, scale):
    r = np.random.default_rng(seed)
    mu = r.normal(size=(K, D)) * sep
    y = r.integers(0, K, N)
    X = ((mu[y] + r.normal(size=(N, D))) * scale).astype(np.float32)
    return X, y.astype(np.int64)


# name -> (N, D, K, seed, sep, scale); the test split is make(400, ...) with the same seed, so its first draw reproduces mu
CASES = {"n257_d33_k5": (257, 33, 5, 0, 1.0, 1.0), "n515_d48_k7": (515, 48, 7, 1, 0.6, 1.0), "n1000_d64_k10_x3": (1000, 64, 10, 2, 0.5, 3.0),
         "n300_d40_k2": (300, 40, 2, 3, 0.5, 1.0), "n300_d24_skip": (300, 24, 5, 4, 0.8, 1.0)}
# wider than one 64-column tile, at the class limit, past 64 row blocks: device solver only (tests/test_gpu_svm_edges.py).  Kept out of CASES, which
# the host L-BFGS test walks class by class
WIDE_CASES = {"n1100_d132_k40": (1100, 132, 40, 5, 1.0, 1.0), "n700_d130_k64": (700, 130, 64, 7, 1.0, 1.0), "n4161_d70_k3": (4161, 70, 3, 6, 0.5, 1.0)}
G_ALLOW_MIN = 5e-3                                            # see g_allow
SKIP_IDS = np.array([0, 1, 3, 4, 5], dtype=np.int64)          # the 'skip' case draws 5 of the 6 ids 0..5: id 2 never occurs
N_TEST = 400


@functools.lru_cache(maxsize=None)
def problem(name):
    """-> (X train, labels train, X test, labels test, classes)"""
    N, D, K, seed, sep, scale = CASES[name] if name in CASES else WIDE_CASES[name]
    X, y = make(N, D, K, seed, sep, scale)
    Xt, yt = make(N_TEST, D, K, seed, sep, scale)
    if name.endswith("skip"):
        y, yt = SKIP_IDS[y], SKIP_IDS[yt]
    for a in (X, y, Xt, yt):
        a.setflags(write=False)
    return X, y, Xt, yt, np.unique(y)


def objective_and_gradient(W, b, X, labels, classes, C=1.0):
    """float64: f [K], dW [K,D], db [K] of f_c = 1/2 (|w|^2 + b^2) + C sum_i max(0, 1 - y_ic (x_i . w + b))^2"""
    W, b, X = np.asarray(W, np.float64), np.asarray(b, np.float64), np.asarray(X, np.float64)
    Y = np.where(np.asarray(labels)[:, None] == np.asarray(classes)[None, :], 1.0, -1.0)           # [N,K]
    H = np.maximum(0.0, 1.0 - Y * (X @ W.T + b[None, :]))
    f = 0.5 * ((W * W).sum(1) + b * b) + C * (H * H).sum(0)
    R = Y * H
    return f, W - 2.0 * C * (R.T @ X), b - 2.0 * C * R.sum(0)


def grad_norms(W, b, X, labels, classes, C=1.0):
    _, gW, gb = objective_and_gradient(W, b, X, labels, classes, C)
    return np.sqrt((gW * gW).sum(1) + gb * gb)


def _rows(clf, K):
    """coef_ [K,D], intercept_ [K] of a fitted sklearn LinearSVC; two classes: sklearn keeps the row of classes_[1], the other is its mirror image"""
    W, b = np.asarray(clf.coef_, np.float64), np.asarray(clf.intercept_, np.float64)
    if K == 2:
        W, b = np.concatenate([-W, W]), np.concatenate([-b, b])
    return W, b


@functools.lru_cache(maxsize=None)
def oracle(name, tight=True):
    """sklearn on the float64 copy of the features -> (W [K,D], b [K]).  tight: the primal Newton solver run to tol 1e-10; else LinearSVC()"""
    from sklearn.svm import LinearSVC
    X, y, _, _, classes = problem(name)
    clf = LinearSVC(dual=False, tol=1e-10, max_iter=100000) if tight else LinearSVC()
    clf.fit(X.astype(np.float64), y)
    assert np.array_equal(clf.classes_, classes)
    W, b = _rows(clf, len(classes))
    W.setflags(write=False); b.setflags(write=False)
    return W, b


@functools.lru_cache(maxsize=None)
def g_allow(name):
    """From the tight oracle alone: the 5th smallest of (top1 - top2) / (4 |[x, 1]|) over the N_TEST test rows.  The gap rule of the solver tests
    leaves a row out when its oracle gap is at most 2 |[x, 1]| * 2 g (a point within g of the minimiser moves a score by at most |[x, 1]| g), so a
    device gradient norm g below this figure leaves out at most 4 rows = 1 %: the cap on the rows left out then cannot hide a solver that stops early"""
    Xt = problem(name)[2].astype(np.float64)
    Wo, bo = oracle(name)
    top = np.sort(Xt @ Wo.T + bo, axis=1)
    return float(np.sort((top[:, -1] - top[:, -2]) / (4.0 * np.sqrt((Xt * Xt).sum(1) + 1.0)))[4])
