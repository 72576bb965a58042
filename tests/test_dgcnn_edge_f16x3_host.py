"""CPU checks of the range guard and the arithmetic of the frozen tokenizer's stacked edge-conv products on split-f16 planes (composite.dgcnn_features,
ACT_TOKENIZER_DGCNN_F16X3): the A operand of layers 2-4 is a column slice of the head's operand, split at the head's scale, so the head's weight-only bound
must hold for every slice on its own -- checked with the adversarial single-spike groups of tests/test_dgcnn_f16x3_host.py at each layer's own width -- the
scale keeps every plane inside f16 at the Stage-II and the C5 geometry, and the numpy restatement of the kernel (tests/f16x3_ref.py) is fp32-grade at K = 256
and K = 512 with the split at that (far too careful) scale."""
import math
import os
import subprocess
import sys

import numpy as np

from tests import f16x3_ref as R

COUTS, GROUPS = (256, 512, 512, 1024), 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tail(x, gamma, beta, groups=GROUPS, eps=1e-5, slope=0.2):
    """x [C, G, k] (one cloud) -> [C, G]: GroupNorm(groups) over (C / groups, G, k) with the biased variance, affine, LeakyReLU, max over k; float64"""
    xg = x.reshape(groups, -1)
    xh = ((xg - xg.mean(1, keepdims=True)) / np.sqrt(xg.var(1, keepdims=True) + eps)).reshape(x.shape)
    y = xh * gamma[:, None, None] + beta[:, None, None]
    return np.where(y >= 0, y, slope * y).max(axis=2)


def test_the_head_bound_holds_for_every_slice_under_single_spike_groups():
    """one spike per GroupNorm group standardises to sqrt(n - 1): the extreme of each layer's tail.  Every layer at its own width (G = 8, k = 4 keeps it
    small), gamma = 1 + noise, the spike on the channel with the largest |gamma|: the slice reaches 99 % of its own term of the bound and never passes it."""
    import act_amd.composite as CP
    rng = np.random.default_rng(0)
    G, k = 8, 4
    gam = [1 + 0.1 * rng.standard_normal(c) for c in COUTS]
    bet = [0.1 * rng.standard_normal(c) for c in COUTS]
    gmax, bmax = [float(np.abs(g).max()) for g in gam], [float(np.abs(b).max()) for b in bet]
    bound = CP.f16x3_dgcnn_bound(gmax, bmax, COUTS, [GROUPS] * 4, G, k)
    for c, g, b in zip(COUTS, gam, bet):
        n = (c // GROUPS) * G * k
        ch = int(np.abs(g).argmax())
        for sign in (1.0, -1.0):
            x = np.zeros((c, G, k))
            x[ch, 3, 1] = sign * 1e3
            g2 = g.copy()
            g2[ch] = sign * abs(g[ch])                      # the spike lands on the positive side of LeakyReLU
            top = float(np.abs(_tail(x, g2, np.zeros(c))).max())
            assert top <= math.sqrt(n) * abs(g[ch]) <= bound
            assert top >= 0.99 * math.sqrt(n - 1) * abs(g[ch]), (top, n)
            assert float(np.abs(_tail(x, g2, b)).max()) <= bound
        assert float(np.abs(_tail(1e4 * rng.standard_normal((c, G, k)) + 3e4, g, b)).max()) <= bound


def test_the_scale_keeps_the_bound_inside_f16_at_both_geometries():
    import act_amd.composite as CP
    rng = np.random.default_rng(1)
    for G, k in ((64, 4), (512, 4)):
        for gam, bet in (([np.ones(c) for c in COUTS], [np.zeros(c) for c in COUTS]),
                         ([1 + 0.1 * rng.standard_normal(c) for c in COUTS], [0.1 * rng.standard_normal(c) for c in COUTS])):
            bound = CP.f16x3_dgcnn_bound([float(np.abs(g).max()) for g in gam], [float(np.abs(b).max()) for b in bet], COUTS, [GROUPS] * 4, G, k)
            s = CP.f16x3_act_scale(bound)
            assert s > 0 and s == R.act_scale(bound) and bound * s <= 32768.0 and 2 * bound * s > 32768.0
            for c, g, b in zip(COUTS, gam, bet):            # ... hence every slice: its own term is below the maximum
                assert (math.sqrt((c // GROUPS) * G * k) * float(np.abs(g).max()) + float(np.abs(b).max())) * s <= 32768.0


def test_the_stacked_products_are_fp32_grade_at_the_head_scale():
    """K = 256 (layer 2) and K = 512 (layers 3, 4): the operand is a tail's output, split at the scale the guard derives for the whole cat at (G, k) = (64, 4)
    -- set by layer 4's width, 60-90 x above what the slice reaches -- against float64, next to an fp32 matmul: the gate of tests/test_f16x3_host.py"""
    import act_amd.composite as CP
    rng = np.random.default_rng(2)
    G, k = 64, 4
    gam = [1 + 0.1 * rng.standard_normal(c) for c in COUTS]
    bet = [0.1 * rng.standard_normal(c) for c in COUTS]
    s = CP.f16x3_act_scale(CP.f16x3_dgcnn_bound([float(np.abs(g).max()) for g in gam], [float(np.abs(b).max()) for b in bet], COUTS, [GROUPS] * 4, G, k))
    assert s > 0
    for layer, N in ((0, 256), (1, 256), (2, 512)):         # the slice that feeds layers 2, 3, 4 (K = 256, 512, 512); N kept small
        K = COUTS[layer]
        a = _tail(rng.standard_normal((K, G, k)), gam[layer], bet[layer]).T.astype(np.float32)          # [G, K]
        w = (rng.standard_normal((N, K)) / math.sqrt(K)).astype(np.float32)
        h1, h2 = R.split(a, s)
        assert np.isfinite(h1.astype(np.float32)).all() and np.isfinite(h2.astype(np.float32)).all()
        ref = a.astype(np.float64) @ w.astype(np.float64).T
        e32 = float(np.linalg.norm((a @ w.T).astype(np.float64) - ref) / np.linalg.norm(ref))
        e16 = float(np.linalg.norm(R.gemm(a, w, s).astype(np.float64) - ref) / np.linalg.norm(ref))
        print(f"K {K} max|a| {np.abs(a).max():.2f} scale {s:g}: f32 matmul {e32:.2e}  split-f16 {e16:.2e}")
        assert e16 <= 1.5 * e32, (e16, e32)


def test_the_switch_defaults_to_on():
    code = "import act_amd.composite as CP; print(int(CP.TOKENIZER_DGCNN_F16X3), CP.DGCNN_F16X3_MIN_T)"
    env = {k: v for k, v in os.environ.items() if k != "ACT_TOKENIZER_DGCNN_F16X3"}
    run = lambda e: subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, check=True).stdout.split()
    assert run(env) == ["1", "4096"] and run(dict(env, ACT_TOKENIZER_DGCNN_F16X3="0")) == ["0", "4096"]
