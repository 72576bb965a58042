"""CPU checks of the range guard and the arithmetic of the frozen tokenizer's last mini-PointNet product on split-f16 planes (composite.pointnet_forward,
ACT_TOKENIZER_PN_F16X3): the weight-only bound on relu(bn2(h3)) under training-mode statistics really bounds it and is attained up to 1 %, the scale taken
from it keeps every plane inside f16 at the Stage-II and the C5 row counts, a gamma past the limit withholds the scale, and the numpy restatement of the
kernel (tests/f16x3_ref.py) with the affine map, ReLU and split applied the kernel's way is fp32-grade at K = 512."""
import math

import numpy as np

from tests import f16x3_ref as R


def _bn_relu(x, gamma, beta, eps=1e-5):
    """x [R, C] -> relu(BatchNorm(x)) with the batch's biased variance; float64"""
    y = (x - x.mean(0, keepdims=True)) / np.sqrt(x.var(0, keepdims=True) + eps) * gamma[None, :] + beta[None, :]
    return np.maximum(y, 0.0)


def test_the_bound_holds_and_a_spike_attains_it():
    import act_amd.composite as CP
    rng = np.random.default_rng(0)
    Rr, C = 4096, 16
    gamma, beta = rng.standard_normal(C), rng.standard_normal(C)
    bc = math.sqrt(Rr) * np.abs(gamma) + np.abs(beta)
    bound = CP.f16x3_pointnet_bound(float(np.abs(gamma).max()), float(np.abs(beta).max()), Rr)
    assert bound >= bc.max()
    for x in (rng.standard_normal((Rr, C)), 1e4 * rng.standard_normal((Rr, C)) + 3e4):
        y = _bn_relu(x, gamma, beta)
        assert np.all(y <= bc[None, :]) and y.max() <= bound
    # a column that is zero except one spike: its standardised value is sqrt(R - 1) up to eps
    for sign in (1.0, -1.0):
        for c in (0, 7, 15):
            x = np.zeros((Rr, C))
            x[11, c] = sign * 1e3
            g = gamma.copy()
            g[c] = sign * abs(g[c])                        # the spike lands on the positive side of ReLU
            y = _bn_relu(x, g, np.zeros(C))
            assert np.all(y <= (math.sqrt(Rr) * np.abs(g))[None, :])
            assert y[11, c] >= 0.99 * math.sqrt(Rr - 1) * abs(g[c]), (y[11, c], math.sqrt(Rr - 1) * abs(g[c]))
            assert np.all(_bn_relu(x, g, beta) <= (math.sqrt(Rr) * np.abs(g) + np.abs(beta))[None, :])


def test_the_scale_keeps_the_bound_inside_f16_and_a_large_gamma_withholds_it():
    import act_amd.composite as CP
    rng = np.random.default_rng(1)
    for Rr in (262144, 2097152):                           # Stage II (B = 128, G = 64, n = 32) and the C5 geometry
        for gamma, beta in ((np.ones(512), np.zeros(512)), (1 + 0.1 * rng.standard_normal(512), 0.1 * rng.standard_normal(512))):
            bound = CP.f16x3_pointnet_bound(float(np.abs(gamma).max()), float(np.abs(beta).max()), Rr)
            assert bound == math.sqrt(Rr) * float(np.abs(gamma).max()) + float(np.abs(beta).max())
            s = CP.f16x3_act_scale(bound)
            assert s > 0 and s == R.act_scale(bound) and s * bound <= 32768.0 and 2 * s * bound > 32768.0
        g = 1.0
        while CP.f16x3_pointnet_bound(g, 0.0, Rr) <= 32768.0:
            g *= 2
        assert CP.f16x3_act_scale(CP.f16x3_pointnet_bound(g, 0.0, Rr)) == 0.0          # no scale: the f32 product
    assert CP.f16x3_act_scale(CP.f16x3_pointnet_bound(float("nan"), 0.0, 262144)) == 0.0


def test_the_on_load_product_is_fp32_grade_at_the_derived_scale():
    """K = 512: affine map with the scale folded in (one fp32 fma), ReLU, split, three products -- against float64 of the same fp32 inputs, next to an fp32
    matmul of the fp32 activation: the gate of tests/test_f16x3_host.py.  The scale is the one the guard derives for R = 262,144 rows."""
    import act_amd.composite as CP
    rng = np.random.default_rng(2)
    Rr, K, C = 256, 512, 128
    for shift in (0.0, 2.0):
        h = (rng.standard_normal((Rr, K)) + shift).astype(np.float32)
        gamma, beta = (1 + 0.1 * rng.standard_normal(K)), 0.1 * rng.standard_normal(K)
        sc = (gamma / np.sqrt(h.astype(np.float64).var(0) + 1e-5)).astype(np.float32)
        sh = (beta - h.astype(np.float64).mean(0) * sc).astype(np.float32)
        w = (0.05 * rng.standard_normal((C, K))).astype(np.float32)
        s = CP.f16x3_act_scale(CP.f16x3_pointnet_bound(float(np.abs(gamma).max()), float(np.abs(beta).max()), 262144))
        assert s > 0
        # the kernel's operand: fma(h, sc s, sh s) in fp32 (float64 product and sum of fp32 values, rounded once), ReLU; s is a power of two, so it is s a
        a_s = np.maximum((h.astype(np.float64) * (sc * np.float32(s)).astype(np.float64) + (sh * np.float32(s)).astype(np.float64)).astype(np.float32), 0)
        a = np.maximum((h.astype(np.float64) * sc.astype(np.float64) + sh.astype(np.float64)).astype(np.float32), 0)
        assert np.array_equal(a_s, a * np.float32(s))
        h1, h2 = R.split(a_s, 1.0)
        assert np.isfinite(h1.astype(np.float32)).all() and np.isfinite(h2.astype(np.float32)).all() and float(a_s.max()) <= 32768.0
        ref = a.astype(np.float64) @ w.astype(np.float64).T
        e32 = float(np.linalg.norm((a @ w.T).astype(np.float64) - ref) / np.linalg.norm(ref))
        e16 = float(np.linalg.norm(R.gemm(a, w, s).astype(np.float64) - ref) / np.linalg.norm(ref))
        print(f"shift {shift}: max|a| {a.max():.2f} scale {s:g}: f32 matmul {e32:.2e}  split-f16 {e16:.2e}")
        assert e16 <= 1.5 * e32, (e16, e32)


def test_the_switch_defaults_to_on():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import act_amd.composite as CP; print(int(CP.TOKENIZER_PN_F16X3))"
    env = {k: v for k, v in os.environ.items() if k != "ACT_TOKENIZER_PN_F16X3"}
    run = lambda e: subprocess.run([sys.executable, "-c", code], cwd=root, env=e, capture_output=True, text=True, check=True).stdout.split()
    assert run(env) == ["1"] and run(dict(env, ACT_TOKENIZER_PN_F16X3="0")) == ["0"]
