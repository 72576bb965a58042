"""CPU: the arithmetic of the default teacher's prompt keys / values (act_prompt_kv_fwd_f16x3_f32) restated in numpy -- LayerNorm rows of dropout(tok) + ppos,
split at the qkv Linear's static scale act_scale(max ln_bound(gamma, beta)), multiplied the split-f16 kernel's way (tests/f16x3_ref.py) -- against float64.
The gate is the one of the project's split-f16 tests: relative L2 error at most 1.5 x that of an fp32 matmul of the same rows."""
import numpy as np
import pytest

from tests import f16x3_ref as R

EPS = 1e-6


def _inputs(P, D, N, offset=0.0, seed=0):
    g = np.random.default_rng(1000 + 7 * P + D + N + seed)
    r = lambda *s: g.standard_normal(s).astype(np.float32)
    tok, ppos = r(P, D), r(P, D) * np.float32(0.5) + np.float32(offset)
    gamma, beta = np.float32(1) + np.float32(0.2) * r(D), np.float32(0.1) * r(D)
    w = r(N, D) / np.float32(D ** 0.5)
    return tok, ppos, gamma, beta, w, g


def _ln_rows(v, gamma, beta):
    """fp32 LayerNorm rows (statistics in float64, rounded once: the kernel's rows to within an fp32 rounding)"""
    v = v.astype(np.float64)
    mean = v.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(v.var(axis=1, keepdims=True) + EPS)
    return ((v - mean) * rstd * gamma.astype(np.float64) + beta.astype(np.float64)).astype(np.float32)


def _rel_l2(x, ref):
    return float(np.linalg.norm(x.astype(np.float64) - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("drop_p,offset", [(0.0, 0.0), (0.1, 0.0), (0.5, 0.0), (0.1, 3.0)])
def test_error_against_float64_is_that_of_an_fp32_product(drop_p, offset):
    rows, D, N = 128, 768, 1536
    P = 64
    tok, ppos, gamma, beta, w, g = _inputs(P, D, N, offset)
    keep = (g.random((rows, D)) >= drop_p).astype(np.float32)
    v = np.tile(tok, (rows // P, 1)) * keep * np.float32(1.0 / (1.0 - drop_p)) + np.tile(ppos, (rows // P, 1))
    n1p = _ln_rows(v, gamma, beta)
    s_a = R.act_scale(R.ln_bound(gamma, beta).max())
    assert s_a > 0 and np.abs(n1p).max() * s_a <= 2.0 ** 15
    ref = n1p.astype(np.float64) @ w.astype(np.float64).T
    e32 = _rel_l2(n1p @ w.T, ref)
    e16 = _rel_l2(R.gemm(n1p, w, s_a), ref)
    print(f"rows {rows} D {D} N {N} drop {drop_p} offset {offset}: fp32 {e32:.3e}  split-f16 {e16:.3e}  ratio {e16 / e32:.2f}")
    assert e16 <= 1.5 * e32, (e16, e32)


def test_a_spike_row_stays_inside_the_f16_range():
    """one channel carries the whole row: |xhat| reaches sqrt(D - 1), the extreme the bound sqrt(D) |gamma| + |beta| is written for"""
    D = 768
    g = np.random.default_rng(5)
    gamma = (1 + 0.2 * g.standard_normal(D)).astype(np.float32)
    beta = (0.1 * g.standard_normal(D)).astype(np.float32)
    j = int(np.abs(gamma).argmax())
    v = np.zeros((2, D), dtype=np.float32)
    v[0, j], v[1, j] = 1e4, -1e4
    n1p = _ln_rows(v, gamma, beta)
    assert np.abs(n1p).max() > 0.99 * np.sqrt(D - 1) * np.abs(gamma[j]) - np.abs(beta[j])          # the spike really is at the extreme
    s_a = R.act_scale(R.ln_bound(gamma, beta).max())
    h1, h2 = R.split(n1p, s_a)
    assert np.abs(n1p.astype(np.float64) * s_a).max() <= 2.0 ** 15
    assert np.isfinite(h1.astype(np.float32)).all() and np.isfinite(h2.astype(np.float32)).all()
    back = (h1.astype(np.float64) + h2.astype(np.float64) / 2048.0) / s_a
    assert np.abs(back - n1p).max() <= 2.0 ** -21 * np.abs(n1p).max()                              # 22 bits of the largest element survive the split
