"""GPU: csrc/svm.hip past what tests/test_gpu_svm.py reaches -- more than one 64-column tile of the transposed product (d0 = 64, 128, ... with a last
tile of one float4 or of 1 - 3 ragged columns), more than two reduction chunks of the scores and W rows up to the class limit of 64, the scalar load
form on a base that is not 16-byte aligned, a mask holding -0.0, sums over more than 64 row blocks (N > 4096), the solver at D = 130 / 132 and
K = 40 / 64, the independence of the classes solved together, and the argument checks.

The products are checked for EQUALITY on integer lattices (X, W in [-4, 4], P in [-2, 2], b in [-8, 8]): every partial sum is an integer below 2^24,
so the fp32 FMA chains, the fp32 256-row partial tiles and the float64 sums over the splits are exact in any order and the result is the int64
numpy product, element for element.  On real values the bars are those of tests/test_gpu_svm.py, unchanged.  Every test prints what it measured
before it asserts."""
import functools

import numpy as np
import pytest
import torch

from tests import svm_ref as R
from tests.test_gpu_svm import DEV, EPS32, _dev, _fit, check_hinge, check_solver

pytestmark = pytest.mark.gpu

# (N, D, K).  scores: one tile of everything; three chunks and one class; vector loads, five chunks, the last holding one float4, three row blocks;
# scalar loads, the last chunk holding two columns, five row blocks, the class limit; the production width (24 chunks); the smallest
SCORES_SHAPES = [(64, 64, 64), (65, 68, 1), (130, 132, 40), (257, 130, 64), (70, 768, 40), (3, 4, 2)]
# tprod: one tile of everything; a second column tile of one column and a second split of one row; three column tiles (the last one float4), five
# splits; scalar loads, a last tile of two columns, a third split of one row; twelve column tiles; fewer rows than one 32-row chunk; one row
TPROD_SHAPES = [(256, 64, 64), (257, 65, 5), (1100, 132, 40), (513, 130, 64), (300, 768, 40), (31, 200, 3), (1, 70, 2)]
_ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]
MIS = (130, 132, 40)                                         # D % 4 == 0: only the base address can select the scalar loads
WIDE = "n1100_d132_k40"


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _lattice(N, D, K):
    """-> X [N,D], W [K,D], b [K], P [N,K] (about 40 % zeros), float32 holding integers"""
    r = np.random.default_rng(1000003 * N + 1009 * D + K)
    X, W = r.integers(-4, 5, (N, D)), r.integers(-4, 5, (K, D))
    b = r.integers(-8, 9, K)
    P = r.choice(np.array([-2, -1, 1, 2]), (N, K))
    P[r.random((N, K)) < 0.4] = 0
    return _frozen(*(a.astype(np.float32) for a in (X, W, b, P)))


@functools.lru_cache(maxsize=None)
def _gaussian(N, D, K):
    r = np.random.default_rng(7 + 1000003 * N + 1009 * D + K)
    X, W, b, P = (r.normal(size=s).astype(np.float32) for s in ((N, D), (K, D), (K,), (N, K)))
    P[r.random((N, K)) < 0.4] = 0                              # the sparsity of a hinge / an active mask
    return _frozen(X, W, b, P)


def _signed_zeros(P, seed):
    """P with its zeros made half +0.0 and half -0.0"""
    r = np.random.default_rng(seed)
    m = P.copy()
    z = np.flatnonzero(P == 0)
    neg = z[r.permutation(z.size)[: z.size // 2]]
    m.ravel()[neg] = np.copysign(np.float32(0), np.float32(-1))
    assert np.signbit(m.ravel()[z]).sum() == z.size // 2 and np.array_equal(m == 0, P == 0)
    return m


def _assert_exact(got, ref, what):
    """got (float32 from the device) == ref (int64) element for element; the message names the first element that differs"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere(~(got.astype(np.float64) == ref))
    print(f"{what}: {len(bad)} of {ref.size} elements differ from the int64 product")
    if len(bad):
        at = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{what}: {len(bad)} elements differ, the first at (row, column) = {at}: got {got[at]!r}, expected {ref[at]}")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _misaligned(a):
    """a contiguous device view of ``a``'s values whose base address is one float past a 16-byte boundary"""
    t = a if torch.is_tensor(a) else _dev(a)
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4       # the test cannot pass by not reaching the path
    return v


# ---- 1. the products -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,K", SCORES_SHAPES, ids=_ids(SCORES_SHAPES))
def test_scores_exact_on_a_lattice_and_masked_by_either_zero(N, D, K):
    from act_amd import kernels as Kn
    X, W, b, P = _lattice(N, D, K)
    Xi, Wi, bi = X.astype(np.int64), W.astype(np.int64), b.astype(np.int64)
    assert (np.abs(Xi) @ np.abs(Wi).T + np.abs(bi)).max() < 2 ** 24          # every partial sum is an exactly representable integer
    Xd, Wd, bd = _dev(X), _dev(W), _dev(b)
    got = Kn.svm_scores(Xd, Wd, bd).cpu().numpy()
    nob = Kn.svm_scores(Xd, Wd).cpu().numpy()
    _assert_exact(got, Xi @ Wi.T + bi, f"scores {N}x{D}x{K} with b")
    _assert_exact(nob, Xi @ Wi.T, f"scores {N}x{D}x{K} without b")
    mask = _signed_zeros(P, N + D)
    for m, what in ((mask, "both zeros"), (-mask, "both zeros, signs swapped")):
        masked = Kn.svm_scores(Xd, Wd, bd, mask=_dev(m)).cpu().numpy()
        zero = m == 0
        wrong_zero = int(((masked.view(np.int32) & 0x7FFFFFFF) != 0)[zero].sum())
        wrong_kept = int((masked.view(np.int32) != got.view(np.int32))[~zero].sum())
        print(f"scores {N}x{D}x{K} mask ({what}): {int(zero.sum())} masked, {int(np.signbit(m[zero]).sum())} of them by -0.0; "
              f"{wrong_zero} masked scores not zero, {wrong_kept} kept scores changed")
        assert wrong_zero == 0 and wrong_kept == 0


@pytest.mark.parametrize("N,D,K", TPROD_SHAPES, ids=_ids(TPROD_SHAPES))
def test_tprod_exact_on_a_lattice_and_deterministic(N, D, K):
    from act_amd import kernels as Kn
    X, _, _, P = _lattice(N, D, K)
    Xi, Pi = X.astype(np.int64), P.astype(np.int64)
    assert (np.abs(Pi).T @ np.abs(Xi)).max() < 2 ** 24 and np.abs(Pi).sum(0).max() < 2 ** 24
    out, colsum = Kn.svm_tprod(_dev(P), _dev(X))
    out2, colsum2 = Kn.svm_tprod(_dev(P), _dev(X))
    _assert_exact(out.cpu().numpy(), Pi.T @ Xi, f"tprod {N}x{D}x{K}")
    _assert_exact(colsum.cpu().numpy()[:, None], Pi.sum(0)[:, None], f"tprod {N}x{D}x{K} column sums")
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(colsum), _bits(colsum2))


@pytest.mark.parametrize("N,D,K", SCORES_SHAPES, ids=_ids(SCORES_SHAPES))
def test_scores_forward_bound(N, D, K):
    """X W^T + b against float64 numpy, bar (D + 1) x fp32 epsilon x (sum_d |x w| + |b|), as test_gpu_svm.test_scores_forward_bound_and_mask"""
    from act_amd import kernels as Kn
    X, W, b, P = _gaussian(N, D, K)
    X64, W64, b64 = X.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    bar = (D + 1) * EPS32 * (np.abs(X64) @ np.abs(W64).T + np.abs(b64))
    got = Kn.svm_scores(_dev(X), _dev(W), _dev(b)).cpu().numpy()
    nob = Kn.svm_scores(_dev(X), _dev(W)).cpu().numpy()
    masked = Kn.svm_scores(_dev(X), _dev(W), _dev(b), mask=_dev(P)).cpu().numpy()
    err, errn = np.abs(got - (X64 @ W64.T + b64)), np.abs(nob - X64 @ W64.T)
    print(f"scores {N}x{D}x{K}: max err / bar = {(err / bar).max():.3e} with b, {(errn / bar).max():.3e} without")
    assert bar.min() > 0 and (err <= bar).all() and (errn <= bar).all()
    assert np.array_equal(masked, np.where(P != 0, got, np.float32(0)))


@pytest.mark.parametrize("N,D,K", TPROD_SHAPES, ids=_ids(TPROD_SHAPES))
def test_tprod_forward_bound(N, D, K):
    """P^T X and the column sums of P against float64 numpy, bars N x fp32 epsilon x sum_i |p_ic x_id| and N x fp32 epsilon x sum_i |p_ic|, as
    test_gpu_svm.test_transposed_product_forward_bound"""
    from act_amd import kernels as Kn
    X, _, _, P = _gaussian(N, D, K)
    out, colsum = Kn.svm_tprod(_dev(P), _dev(X))
    P64, X64 = P.astype(np.float64), X.astype(np.float64)
    err = np.abs(out.cpu().numpy().astype(np.float64) - P64.T @ X64)
    bar = N * EPS32 * (np.abs(P64).T @ np.abs(X64))
    errb = np.abs(colsum.cpu().numpy().astype(np.float64) - P64.sum(0))
    barb = N * EPS32 * np.abs(P64).sum(0)
    ratio = lambda e, b: float(np.divide(e, b, out=np.zeros_like(e), where=b > 0).max())       # a column of P that is all zero has bar 0 and err 0
    print(f"tprod {N}x{D}x{K}: max err / bar = {ratio(err, bar):.3e}, column sums {ratio(errb, barb):.3e}")
    assert np.isfinite(out.cpu().numpy()).all() and (err <= bar).all() and (errb <= barb).all()


# ---- 2. the scalar loads on a misaligned base ------------------------------------------------------------------------------------------------
def test_misaligned_base_is_bit_identical():
    """D % 4 == 0 on a base one float past a 16-byte boundary: svm_vec_ok selects the scalar loads, which put the same values in the same LDS
    slots as the float4 loads, and the arithmetic is shared: any difference from the aligned call is a defect"""
    from act_amd import kernels as Kn
    N, D, K = MIS
    X, W, b, P = (_dev(a) for a in _gaussian(N, D, K))
    assert D % 4 == 0 and X.data_ptr() % 16 == 0 and W.data_ptr() % 16 == 0
    Xm, Wm, Pm = _misaligned(X), _misaligned(W), _misaligned(P)
    ref, ref_masked = Kn.svm_scores(X, W, b), Kn.svm_scores(X, W, b, mask=P)
    for x, w, what in ((Xm, W, "x"), (X, Wm, "w"), (Xm, Wm, "x and w")):
        got, got_masked = Kn.svm_scores(x, w, b), Kn.svm_scores(x, w, b, mask=Pm)
        n1, n2 = int((_bits(got) != _bits(ref)).sum()), int((_bits(got_masked) != _bits(ref_masked)).sum())
        print(f"scores {N}x{D}x{K}, misaligned {what}: {n1} elements differ from the aligned call, {n2} with a mask")
        assert n1 == 0 and n2 == 0
    out, colsum = Kn.svm_tprod(P, X)
    for p, what in ((P, "x"), (Pm, "x and p")):
        o, c = Kn.svm_tprod(p, Xm)
        n1, n2 = int((_bits(o) != _bits(out)).sum()), int((_bits(c) != _bits(colsum)).sum())
        print(f"tprod {N}x{D}x{K}, misaligned {what}: {n1} elements differ from the aligned call, {n2} column sums")
        assert n1 == 0 and n2 == 0


# ---- 3. sums over more than 64 row blocks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(4097, 3), (4161, 5), (4160, 64)])
def test_hinge_past_64_row_blocks(N, K):
    """65 blocks, the last of one row; 66 blocks; 65 full blocks at the class limit: svm_block_sum takes its second trip"""
    assert (N + 63) // 64 > 64
    check_hinge(N, K)


# ---- 4. the solver at wide shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.WIDE_CASES))
def test_solver_wide_against_liblinear(name):
    """the assertions of test_gpu_svm.test_solver_against_liblinear.  Its cap of 1 % on the rows left out depends on the device's own gradient
    norm, so the room the problem leaves is established first, from the oracle alone (svm_ref.g_allow): a run that ends above G_ALLOW_MIN is a
    solver failure, and the cap reports it"""
    ga = R.g_allow(name)
    print(f"{name}: g_allow = {ga:.3e} (bar {R.G_ALLOW_MIN:.0e})")
    assert ga >= R.G_ALLOW_MIN                                 # before the device is used
    check_solver(name, _fit(name))


def _newton_loop(Xd, yd):
    """LinearSVC().fit's loop with the state kept -> (classes, W, b, istate [3,K] on the host, dstate [2,K] on the host)"""
    from act_amd import kernels as Kn
    from act_amd.utils.svm import LinearSVC
    ref = LinearSVC()
    classes = torch.unique(yd)
    k = classes.numel()
    W, b = torch.zeros(k, Xd.shape[1], dtype=torch.float32, device=DEV), torch.zeros(k, dtype=torch.float32, device=DEV)
    istate, dstate = Kn.svm_state(k, DEV)
    for _ in range(ref.max_newton):
        Kn.svm_newton(Xd, yd, classes, W, b, istate, dstate, ref.C, ref.tol, ref.max_cg)
        if all(istate[0].tolist()):
            break
    return classes, W, b, istate.cpu().numpy(), dstate.cpu().numpy()


def test_fit_on_misaligned_features_is_bit_identical():
    from act_amd.utils.svm import LinearSVC
    X, y, _, _, _ = R.problem(WIDE)
    ref = _fit(WIDE)
    Xm = _misaligned(X)
    assert X.shape[1] % 4 == 0 and Xm.contiguous().data_ptr() == Xm.data_ptr()          # fit's .contiguous() keeps the view
    clf = LinearSVC().fit(Xm, _dev(y))
    nW, nb = int((_bits(clf.coef_) != _bits(ref.coef_)).sum()), int((_bits(clf.intercept_) != _bits(ref.intercept_)).sum())
    print(f"{WIDE} on a misaligned base: {nW} weights and {nb} intercepts differ; newton {clf.n_iter_} / {ref.n_iter_}, cg {clf.n_cg_} / {ref.n_cg_}, "
          f"status equal: {torch.equal(clf.status_, ref.status_)}")
    assert nW == 0 and nb == 0
    assert clf.n_iter_ == ref.n_iter_ and clf.n_cg_ == ref.n_cg_ and torch.equal(clf.status_, ref.status_)


def test_no_class_depends_on_the_classes_solved_beside_it():
    """Row c of the 40-class fit against row 1 of the two-class fit of ``labels == classes[c]`` (the same y, in column 1 of 2 instead of column c
    of 40).  Each class has its own wave in every per-class kernel, its own column in every tile and its own flags, a frozen class is never written
    again and the early return fires only when all classes are frozen: the weights, the exit flag, the Newton and CG counts and the recorded
    objective and gradient norm are bit-identical, or the classes are coupled"""
    X, y, _, _, classes = R.problem(WIDE)
    Xd = _dev(X)
    cls, W, b, ist, dst = _newton_loop(Xd, _dev(y))
    ref = _fit(WIDE)
    assert np.array_equal(cls.cpu().numpy(), classes) and len(classes) == 40
    assert torch.equal(_bits(W), _bits(ref.coef_)) and torch.equal(_bits(b), _bits(ref.intercept_))      # the loop above is fit's
    assert int(ist[1].max()) == ref.n_iter_ and int(ist[2].max()) == ref.n_cg_ and np.array_equal(ist[0], ref.status_.numpy())
    failures = []
    for c in (0, 17, 39):
        cls2, W2, b2, ist2, dst2 = _newton_loop(Xd, _dev((y == classes[c]).astype(np.int64)))
        assert cls2.tolist() == [0, 1]
        nW = int((_bits(W2[1]) != _bits(W[c])).sum())
        same_b = bool(torch.equal(_bits(b2[1:2]), _bits(b[c:c + 1])))
        same_d = np.array_equal(dst2[:, 1].view(np.int64), dst[:, c].view(np.int64))
        print(f"class {c} alone / among 40: {nW} of {W.shape[1]} weights differ, intercept equal: {same_b}; (flag, newton, cg) {ist2[:, 1].tolist()} / "
              f"{ist[:, c].tolist()}; (objective, gradient norm) {dst2[:, 1].tolist()} / {dst[:, c].tolist()}")
        if nW or not same_b or not same_d or not np.array_equal(ist2[:, 1], ist[:, c]):
            failures.append(c)
    assert not failures, f"classes {failures} depend on the classes solved beside them"


# ---- 5. arguments ----------------------------------------------------------------------------------------------------------------------------
def test_scores_refuses_bad_arguments():
    from act_amd import kernels as Kn
    from act_amd._C import ActHipError
    x, w, m = torch.zeros(8, 12, device=DEV), torch.zeros(5, 12, device=DEV), torch.ones(8, 5, device=DEV)
    assert Kn.SVM_MAX_CLASSES == 64
    assert Kn.svm_scores(x, torch.zeros(64, 12, device=DEV)).shape == (8, 64)        # the limit itself is served
    with pytest.raises(ActHipError):
        Kn.svm_scores(x, torch.zeros(65, 12, device=DEV))
    with pytest.raises(ActHipError):
        Kn.svm_scores(x, torch.zeros(5, 16, device=DEV))
    for bad in (torch.ones(5, 8, device=DEV), torch.ones(8, 6, device=DEV), torch.ones(40, device=DEV)):
        with pytest.raises(ActHipError):
            Kn.svm_scores(x, w, mask=bad)
    assert Kn.svm_scores(x, w, mask=m).shape == (8, 5)


@pytest.mark.parametrize("k", [65, 1])
def test_fit_names_an_unsupported_class_count(k):
    from act_amd._C import ActHipError
    from act_amd.utils.svm import LinearSVC
    y = (torch.arange(130, device=DEV) % k) * 3
    assert torch.unique(y).numel() == k
    with pytest.raises(ActHipError, match=rf"(?<!\d){k} classes"):
        LinearSVC().fit(torch.zeros(130, 8, device=DEV), y)


def test_predict_ties_at_64_classes_go_to_the_lowest_index():
    """a lattice score matrix (exact on the device) whose maximum is tied wherever it falls on one of three duplicated classes"""
    from act_amd.utils.svm import LinearSVC
    N, D, K = 200, 12, 64
    r = np.random.default_rng(64)
    X, W, b = r.integers(-4, 5, (N, D)), r.integers(-4, 5, (K, D)), r.integers(-8, 9, K)
    for lo, hi in ((7, 40), (0, 63), (12, 50)):
        W[hi], b[hi] = W[lo], b[lo]
    S = X @ W.T + b
    tied = (S == S.max(1, keepdims=True)).sum(1) > 1
    ids = np.sort(r.choice(1000, K, replace=False)).astype(np.int64)
    expect = ids[S.argmax(1)]                                  # numpy's argmax is the first of the maxima
    print(f"predict at K = 64: {int(tied.sum())} of {N} rows have a tied maximum, {len(set(S.argmax(1)[tied].tolist()))} different winners among them")
    assert tied.sum() >= 10 and len(set(S.argmax(1)[tied].tolist())) >= 3
    clf = LinearSVC()
    clf.classes_, clf.coef_, clf.intercept_ = _dev(ids), _dev(W.astype(np.float32)), _dev(b.astype(np.float32))
    Xd = _dev(X.astype(np.float32))
    _assert_exact(clf.decision_function(Xd).cpu().numpy(), S, "decision_function at K = 64")
    pred = clf.predict(Xd).cpu().numpy()
    print(f"predict at K = 64: {int((pred != expect).sum())} rows differ from classes_[first argmax], {int((pred != expect)[tied].sum())} of them tied")
    assert np.array_equal(pred, expect)
