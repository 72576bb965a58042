"""CPU checks of the split-f16 teacher arithmetic, on the numpy restatement (tests/f16x3_ref.py): it is fp32-grade on the operand families of the teacher
(error against float64 no worse than an fp32 matmul's), its two known failure modes are the ones the scales close, and the weight-only range-guard bounds
really bound LayerNorm, GELU and attention outputs -- so bound * s_A <= 2^15 makes an f16 overflow impossible."""
import math

import numpy as np
import pytest

from tests import f16x3_ref as R


def _rel_l2(x, ref):
    return float(np.linalg.norm(x.astype(np.float64) - ref) / np.linalg.norm(ref))


def _ln_like(rng, m, k):
    x = rng.standard_normal((m, k))
    x = (x - x.mean(1, keepdims=True)) / x.std(1, keepdims=True)
    return (x * (1 + 0.1 * rng.standard_normal(k)) + 0.1 * rng.standard_normal(k)).astype(np.float32)


def _gelu(x):
    return 0.5 * x * (1 + np.vectorize(math.erf)(x / math.sqrt(2)))


def families(rng, m=96):
    """(name, A [m, K], W [128, K]): the operand families of the teacher's four products"""
    w768 = (0.02 * rng.standard_normal((128, 768))).astype(np.float32)
    w3072 = (0.02 * rng.standard_normal((128, 3072))).astype(np.float32)
    ln = _ln_like(rng, m, 768)
    big = ln * np.float32(3e4 / np.abs(ln).max())
    return [("layernorm", ln, w768), ("acts*1e-2", ln * np.float32(1e-2), w768),
            ("gelu", _gelu(rng.standard_normal((m, 3072))).astype(np.float32), w3072), ("acts<=3e4", big, w768)]


@pytest.mark.parametrize("loose", [1.0, 64.0])
def test_split_f16_products_are_fp32_grade(loose):
    """the three-product form with fp32 accumulation against float64, next to a plain fp32 matmul of the same operands: no worse than 1.5 x (the margin is
    the spread between two fp32 summation orders).  ``loose``: how far the guard's bound sits above the real maximum (the l1 bounds are loose by 10-100 x)"""
    rng = np.random.default_rng(0)
    for name, a, w in families(rng):
        ref = a.astype(np.float64) @ w.astype(np.float64).T
        s_a = R.act_scale(loose * float(np.abs(a).max()))
        if loose * float(np.abs(a).max()) > 32768.0:         # (3e4 under a 64 x loose bound: the guard keeps that Linear on the f32 kernel)
            assert s_a == 0.0
            continue
        assert s_a > 0
        e32, e16 = _rel_l2(a @ w.T, ref), _rel_l2(R.gemm(a, w, s_a), ref)
        print(f"{name:10s} loose {loose:4.0f}: f32 matmul {e32:.2e}  split-f16 {e16:.2e}")
        assert e16 <= 1.5 * e32, (name, e16, e32)
        assert e16 <= 6e-7                                   # absolute: an order of magnitude under the bf16x3 planes' 4.4e-6


def test_what_is_dropped_is_the_2_pow_minus_22_term_only():
    """in exact (float64) accumulation the three products differ from the true product by the h2.h2 term and the planes' own 2^-22 tails"""
    rng = np.random.default_rng(1)
    _, a, w = families(rng)[0]
    ref = a.astype(np.float64) @ w.astype(np.float64).T
    s_a = R.act_scale(float(np.abs(a).max()))
    assert _rel_l2(R.gemm(a, w, s_a, np.float64), ref) <= 2.0 ** -21
    assert _rel_l2(R.gemm(a, w, s_a, np.float64, drop_lolo=False), ref) <= 2.0 ** -22


def test_the_scales_close_the_two_failure_modes():
    rng = np.random.default_rng(2)
    w = (0.02 * rng.standard_normal((128, 768))).astype(np.float32)
    tiny = (1e-6 * (1 + 0.1 * rng.standard_normal((64, 768)))).astype(np.float32)
    ref = tiny.astype(np.float64) @ w.astype(np.float64).T
    assert _rel_l2(R.gemm(tiny, w, 1.0), ref) > 1e-4                         # unscaled: h1 is flushed, h2 alone carries 11 bits
    assert _rel_l2(R.gemm(tiny, w, R.act_scale(float(np.abs(tiny).max()))), ref) <= 6e-7
    huge = np.full((4, 64), 1e5, dtype=np.float32)
    with np.errstate(over="ignore"):
        assert np.isinf(R.split(huge, 1.0)[0].astype(np.float32)).all()      # unscaled: above 65504
    h1, h2 = R.split(huge, R.act_scale(1e5))
    assert np.isfinite(h1.astype(np.float32)).all() and np.abs(h2.astype(np.float32)).max() <= np.abs(h1.astype(np.float32)).max()
    assert R.act_scale(32768.0) == 1.0 and R.act_scale(32769.0) == 0.0 and R.act_scale(float("inf")) == 0.0 and R.act_scale(float("nan")) == 0.0
    assert R.act_scale(1.0) == 32768.0 and R.act_scale(1.5) == 16384.0


def test_split_rule_at_the_edges():
    x = np.array([0.0, -0.0, 2.0 ** -14, -2.0 ** -14, np.nextafter(np.float32(2.0 ** -14), np.float32(0)), 2.0 ** -15, 3e-6, 1.0, -1.0 - 2.0 ** -12, 65504.0],
                 dtype=np.float32)
    h1, h2 = R.split(x)
    f1, f2 = h1.astype(np.float64), h2.astype(np.float64)
    assert np.all((f1 == 0) | (np.abs(f1) >= 2.0 ** -14)) and np.all((f2 == 0) | (np.abs(f2) >= 2.0 ** -14))
    assert f1[5] == 0 and f2[5] == 2.0 ** -4                                 # 2^-15: h1 flushed, h2 = 2^-15 * 2^11 picks the whole value up
    assert f1[8] == -1.0 and f2[8] == -0.5                                   # -(1 + 2^-12): residual -2^-12 * 2^11
    assert not np.signbit(h1[1]) and not np.signbit(h2[0])                   # flushed elements are +0
    rec, xd = f1 + f2 / 2048, x.astype(np.float64)
    top = np.abs(xd) >= 2.0 ** -3                                            # both planes normal: 22 bits + sign
    assert np.all(np.abs(rec - xd)[top] <= np.abs(xd)[top] * 2.0 ** -22)
    assert np.all(np.abs(rec - xd) <= np.abs(xd) * 2.0 ** -11)              # a flushed h1 leaves h2's 11 bits


def test_guard_bounds_hold_on_random_and_adversarial_inputs():
    rng = np.random.default_rng(3)
    D, Hd, eps = 64, 256, 1e-6
    n1w, n1b, n2w, n2b = (rng.standard_normal(D) for _ in range(4))
    wqkv, bqkv = 0.3 * rng.standard_normal((3 * D, D)), rng.standard_normal(3 * D)
    w1, b1 = 0.3 * rng.standard_normal((Hd, D)), rng.standard_normal(Hd)
    b_ln1, b_att, b_ln2, b_gelu = R.block_bounds(n1w, n1b, wqkv, bqkv, n2w, n2b, w1, b1)

    def ln(x, g, b):
        mu = x.mean(1, keepdims=True)
        return (x - mu) / np.sqrt(x.var(1, keepdims=True) + eps) * g + b

    spikes = np.zeros((2 * D, D))
    spikes[np.arange(D), np.arange(D)] = 1e6                                 # one channel carries the row: |xhat| -> sqrt(D - 1)
    spikes[D + np.arange(D), np.arange(D)] = -1e6
    signs = 1e3 * np.sign(rng.standard_normal((64, D)))                      # +-1 rows: every |xhat| ~ 1 with the worst sign pattern for the l1 bound
    rows = np.concatenate([rng.standard_normal((256, D)), 1e4 * rng.standard_normal((64, D)), spikes, signs, np.ones((1, D))])
    y1, y2 = ln(rows, n1w, n1b), ln(rows, n2w, n2b)
    assert np.abs(y1).max() <= b_ln1 and np.abs(y2).max() <= b_ln2
    assert np.abs(y1).max() >= 0.5 * b_ln1                                   # the spikes come close: the bound is not vacuous
    # V rows and attention outputs (any softmax weights, peaked ones included)
    v = y1 @ wqkv[2 * D:].T + bqkv[2 * D:]
    assert np.abs(v).max() <= b_att
    logits = np.concatenate([rng.standard_normal((32, v.shape[0])), 50.0 * rng.standard_normal((32, v.shape[0]))])
    p = np.exp(logits - logits.max(1, keepdims=True)); p /= p.sum(1, keepdims=True)
    assert np.abs(p @ v).max() <= b_att
    # fc1 pre-activation and its GELU
    h = y2 @ w1.T + b1
    assert np.abs(h).max() <= b_gelu and np.abs(_gelu(h)).max() <= b_gelu
    # the l1 bound is attained by the sign pattern of a row
    u2 = R.ln_bound(n2w, n2b)
    n = int(np.argmax(R.l1_bound(w1, b1, u2)))
    worst = np.sign(w1[n]) * u2 * np.sign(b1[n])
    assert abs(worst @ w1[n] + b1[n]) == pytest.approx(b_gelu, rel=1e-12)
    # and with the scale taken from the bound nothing reaches the f16 limit
    for bound, vals in ((b_ln1, y1), (b_att, p @ v), (b_ln2, y2), (b_gelu, _gelu(h))):
        s = R.act_scale(bound)
        assert s > 0 and np.abs(vals).max() * s <= 32768.0
        h1, h2 = R.split(vals.astype(np.float32), s)
        assert np.isfinite(h1.astype(np.float32)).all() and np.isfinite(h2.astype(np.float32)).all()


def test_python_guard_matches_the_restatement():
    """composite.f16x3_act_scale (what the teacher uses) == the restatement's rule, over bounds across the range"""
    import act_amd.composite as CP
    rng = np.random.default_rng(4)
    for b in list(np.exp(rng.uniform(math.log(1e-9), math.log(1e6), 400))) + [2.0 ** k for k in range(-20, 18)] + [0.0, float("inf"), float("nan"), 32768.0]:
        assert CP.f16x3_act_scale(b) == R.act_scale(b), b


def test_default_is_on_and_the_opt_in_is_off():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import act_amd.composite as CP; print(int(CP.TEACHER_F16X3), int(CP.TEACHER_BF16X3))"
    env = {k: v for k, v in os.environ.items() if k not in ("ACT_TEACHER_F16X3", "ACT_TEACHER_BF16X3")}
    run = lambda e: subprocess.run([sys.executable, "-c", code], cwd=root, env=e, capture_output=True, text=True, check=True).stdout.split()
    assert run(env) == ["1", "0"] and run(dict(env, ACT_TEACHER_F16X3="0")) == ["0", "0"]
