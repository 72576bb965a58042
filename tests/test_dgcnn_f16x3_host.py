"""CPU checks of the range guard and the arithmetic of the frozen tokenizer's head product on split-f16 planes (composite.dgcnn_features,
ACT_TOKENIZER_F16X3): the weight-only bound on the head's A operand -- the concatenated GroupNorm + LeakyReLU + max_k tails of the four edge-conv layers --
really bounds it and is attained up to 1 %, the scale taken from it keeps every plane inside f16, and the numpy restatement of the kernel
(tests/f16x3_ref.py) is fp32-grade at the head's K = 2304 with the split at that scale."""
import math

import numpy as np

from tests import f16x3_ref as R

COUTS, GROUPS = (256, 512, 512, 1024), 4


def _tail(x, gamma, beta, groups=GROUPS, eps=1e-5, slope=0.2):
    """x [C, G, k] (one cloud) -> [C, G]: GroupNorm(groups) over (C / groups, G, k) with the biased variance, affine, LeakyReLU, max over k; float64"""
    C = x.shape[0]
    xg = x.reshape(groups, -1)
    xh = ((xg - xg.mean(1, keepdims=True)) / np.sqrt(xg.var(1, keepdims=True) + eps)).reshape(x.shape)
    y = xh * gamma[:, None, None] + beta[:, None, None]
    y = np.where(y >= 0, y, slope * y)
    assert y.shape[0] == C
    return y.max(axis=2)


def _bound_c(n, gamma, beta):
    return math.sqrt(n) * np.abs(gamma) + np.abs(beta)


def test_the_bound_holds_and_a_spike_attains_it():
    rng = np.random.default_rng(0)
    C, G, k = 32, 24, 4
    n = (C // GROUPS) * G * k
    gamma, beta = rng.standard_normal(C), rng.standard_normal(C)
    bc = _bound_c(n, gamma, beta)[:, None]
    for x in (rng.standard_normal((C, G, k)), 1e4 * rng.standard_normal((C, G, k)) + 3e4):
        assert np.all(np.abs(_tail(x, gamma, beta)) <= bc)
    # every group zero except one spike: its standardised value is sqrt(n - 1) up to eps
    for sign in (1.0, -1.0):
        for c in (0, 9, 31):
            x = np.zeros((C, G, k))
            x[c, 5, 2] = sign * 1e3
            g = gamma.copy()
            g[c] = sign * abs(g[c])                        # the spike lands on the positive side of LeakyReLU
            b = np.zeros(C)
            y = _tail(x, g, b)
            assert np.all(np.abs(y) <= _bound_c(n, g, b)[:, None])
            assert y[c, 5] >= 0.99 * math.sqrt(n - 1) * abs(g[c]), (y[c, 5], math.sqrt(n - 1) * abs(g[c]))
            assert np.all(np.abs(_tail(x, g, beta)) <= _bound_c(n, g, beta)[:, None])


def test_the_scale_keeps_the_bound_inside_f16_and_a_large_gamma_withholds_it():
    import act_amd.composite as CP
    rng = np.random.default_rng(1)
    gs = [1 + 0.1 * rng.standard_normal(c) for c in COUTS]
    bs = [0.1 * rng.standard_normal(c) for c in COUTS]
    for G, k in ((64, 4), (512, 4)):
        for gam in ([np.ones(c) for c in COUTS], gs):
            gmax, bmax = [float(np.abs(g).max()) for g in gam], [float(np.abs(b).max()) for b in bs]
            bound = CP.f16x3_dgcnn_bound(gmax, bmax, COUTS, [GROUPS] * 4, G, k)
            # (max|gamma| and max|beta| are taken apart: at or above the largest per-channel bound, and the formula of the layer that gives most)
            assert bound >= max(float(_bound_c((c // GROUPS) * G * k, g, b).max()) for c, g, b in zip(COUTS, gam, bs))
            assert bound == max(math.sqrt((c // GROUPS) * G * k) * gm + bm for c, gm, bm in zip(COUTS, gmax, bmax))
            s = CP.f16x3_act_scale(bound)
            assert s > 0 and s == R.act_scale(bound) and s * bound <= 32768.0 and 2 * s * bound > 32768.0
        # layer 4's gamma scaled until the bound passes 2^15: no scale, the head stays on the f32 kernel
        gmax = [1.0, 1.0, 1.0, 1.0]
        while CP.f16x3_dgcnn_bound(gmax, [0.0] * 4, COUTS, [GROUPS] * 4, G, k) <= 32768.0:
            gmax[3] *= 2
        assert CP.f16x3_act_scale(CP.f16x3_dgcnn_bound(gmax, [0.0] * 4, COUTS, [GROUPS] * 4, G, k)) == 0.0
    assert CP.f16x3_act_scale(CP.f16x3_dgcnn_bound([float("nan")] + [1.0] * 3, [0.0] * 4, COUTS, [GROUPS] * 4, 64, 4)) == 0.0


def test_the_head_product_is_fp32_grade_at_the_derived_scale():
    """K = 2304: the restatement with the split at the scale the guard derives (60-90 x above the real maximum of cat) against float64, next to an fp32
    matmul of the same operands -- the gate of tests/test_f16x3_host.py"""
    import act_amd.composite as CP
    rng = np.random.default_rng(2)
    k = 4
    for G in (64, 96):
        gam = [1 + 0.1 * rng.standard_normal(c) for c in COUTS]
        bet = [0.1 * rng.standard_normal(c) for c in COUTS]
        cat = np.concatenate([_tail(rng.standard_normal((c, G, k)), g, b) for c, g, b in zip(COUTS, gam, bet)]).T.astype(np.float32)      # [G, 2304]
        assert cat.shape == (G, 2304)
        w = (0.02 * rng.standard_normal((128, 2304))).astype(np.float32)
        bound = CP.f16x3_dgcnn_bound([float(np.abs(g).max()) for g in gam], [float(np.abs(b).max()) for b in bet], COUTS, [GROUPS] * 4, G, k)
        s = CP.f16x3_act_scale(bound)
        assert s > 0 and float(np.abs(cat).max()) <= bound
        h1, h2 = R.split(cat, s)
        assert np.isfinite(h1.astype(np.float32)).all() and np.isfinite(h2.astype(np.float32)).all()
        ref = cat.astype(np.float64) @ w.astype(np.float64).T
        e32 = float(np.linalg.norm((cat @ w.T).astype(np.float64) - ref) / np.linalg.norm(ref))
        e16 = float(np.linalg.norm(R.gemm(cat, w, s).astype(np.float64) - ref) / np.linalg.norm(ref))
        print(f"G {G} bound {bound:.1f} max|cat| {np.abs(cat).max():.2f} scale {s:g}: f32 matmul {e32:.2e}  split-f16 {e16:.2e}")
        assert e16 <= 1.5 * e32, (e16, e32)


def test_the_switch_defaults_to_on():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import act_amd.composite as CP; print(int(CP.TOKENIZER_F16X3))"
    env = {k: v for k, v in os.environ.items() if k != "ACT_TOKENIZER_F16X3"}
    run = lambda e: subprocess.run([sys.executable, "-c", code], cwd=root, env=e, capture_output=True, text=True, check=True).stdout.split()
    assert run(env) == ["1"] and run(dict(env, ACT_TOKENIZER_F16X3="0")) == ["0"]
