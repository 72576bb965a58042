"""GPU: the row kernels of csrc/norm.hip -- LayerNorm forward and backward, act_colsum_f32, cross-entropy, mse / smooth-l1, the cosine loss,
act_scale_rows_f32, act_add_f32 and the prompt rows -- where tests/test_gpu_dense.py and tests/test_gpu_finetune.py do not reach them: a row of one
float4, one live lane in the second chunk, either side of both MAXV switches, every NULL-able pointer, the argument checks, a last LayerNorm-backward
workgroup that is not full, rows_per_block past 16, accumulate_params = 1, every stride tail of the dgamma / dbeta fold, the ACT_LN_BWD_WAVES /
ACT_LN_BWD_RPB forms (fresh child processes: both are read once), ld > C, the 1,024-part cap of the column sums, C < 64 and ties and infinite logits
in the cross-entropy, mean_kernel with two and three elements per thread, the knee of smooth-l1, the clamp region and scaled rows of the cosine, and
the second trip of every grid-stride loop.

Sums are checked for EQUALITY on integer lattices (every partial sum a multiple of 1/2 or of 1/8 below 2^24: float32 adds them exactly in any
order).  On real values the bars are those of tests/test_gpu_dense.py and tests/test_gpu_finetune.py, unchanged: LayerNorm 2e-5 forward and 5e-5
backward, cosine 1e-5, regression 2e-6, cross-entropy 1e-5 (loss) and 1e-6 (dz), bias gradient 2e-5, all as max|err| / max(1, max|ref|) against
float64.  The references are tests/norm_rows_ref.py (checked on the CPU by tests/test_norm_rows_host.py).  Every test prints what it measured
before it asserts.

Out of scope: labels outside [0, C) of the cross-entropy.  The kernel does not check them (it reads logits[row, label]); no case here has one."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import norm_rows_ref as N
from tests.test_gpu_dense import _rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_E_BADARG, ACT_E_NULLPTR = -1, -2
LN_FWD, LN_BWD, COS, REG, XENT_LOSS, XENT_DZ, BIAS = 2e-5, 5e-5, 1e-5, 2e-6, 1e-5, 1e-6, 2e-5
SENT = 7.0
GUARD = 64                                                   # sentinel floats behind a workspace
_ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available()
    import act_amd.kernels as K
    return K


def _kernels():
    import act_amd.kernels as K
    return K


def _st():
    return torch.cuda.current_stream().cuda_stream


def _d(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a, order="C")).to(dtype).cuda()


def _n(t):
    return t.detach().cpu().numpy()


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sent(*shape):
    return torch.full(shape, SENT, device="cuda")


def _untouched(*ts):
    return all(bool((t == SENT).all()) for t in ts)


def _p(t):
    return t.data_ptr() if t is not None else None


def _ordered(a):
    """float32 -> int64 that increases with the value: differences count ulps"""
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _assert_exact(got, ref, what):
    """got (float32 from the device) == ref (int64 or float64) element for element; the message names the first element that differs"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere(~(got == ref))
    print(f"{what}: {len(bad)} of {ref.size} elements differ from the exact result")
    if len(bad):
        at = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{what}: {len(bad)} elements differ, the first at {at}: got {got[at]!r}, expected {ref[at]!r}")


class _Workspace:
    """exactly ``nbytes`` bytes (checked against the restated size) followed by sentinel floats that must survive the call"""

    def __init__(self, nbytes, floats):
        assert nbytes == 4 * floats, (nbytes, floats)
        self.bytes = nbytes
        self.t = _sent(nbytes // 4 + GUARD)

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        assert (self.t[self.bytes // 4:] == SENT).all(), "the kernel wrote past its workspace"


# ---- LayerNorm forward -------------------------------------------------------------------------------------------------------------------------
def _ln_fwd(K, x, pos, g, b, eps=N.LN_EPS, want_xin=True, want_stats=True):
    """act_layernorm_fwd_f32 into sentinel-filled outputs -> rc, y, xin_out, mean, rstd (None where the pointer was NULL)"""
    T, D = x.shape
    y = _sent(T, D)
    xin = _sent(T, D) if want_xin else None
    mean, rstd = (_sent(T), _sent(T)) if want_stats else (None, None)
    rc = K.lib.act_layernorm_fwd_f32(_p(x), _p(pos), _p(g), _p(b), _p(xin), _p(y), _p(mean), _p(rstd), T, D, eps, _st())
    return rc, y, xin, mean, rstd


@pytest.mark.parametrize("D", N.LN_D)
def test_layernorm_forward_shapes_and_optional_pointers(K, D):
    g, b = N.ln_params(D)
    gd, bd = _d(g), _d(b)
    for T in N.LN_FWD_T:
        x, pos, _, _ = N.ln_real(T, D)
        xd, pd = _d(x), _d(pos)
        xin_ref = x + pos                                                                 # one float32 addition per element
        y_ref, m_ref, r_ref = N.layernorm_fwd(xin_ref, g, b)
        rc, y, xin, mean, rstd = _ln_fwd(K, xd, pd, gd, bd)
        e = _rel(y, _t64(y_ref)), _rel(mean, _t64(m_ref)), _rel(rstd, _t64(r_ref))
        print(f"[T={T} D={D}] y, mean, rstd rel err = {e[0]:.2e}, {e[1]:.2e}, {e[2]:.2e} (bar {LN_FWD:.0e})")
        assert rc == 0 and max(e) <= LN_FWD
        assert np.array_equal(_n(xin).view(np.int32), xin_ref.view(np.int32)), "xin_out != x + pos bit for bit"
        rc, y2, xin2, _, _ = _ln_fwd(K, xd, pd, gd, bd, want_xin=False)                   # xin_out = NULL
        assert rc == 0 and xin2 is None and torch.equal(_bits(y2), _bits(y))
        rc, y3, xin3, m3, _ = _ln_fwd(K, xd, pd, gd, bd, want_stats=False)                # mean = rstd = NULL
        assert rc == 0 and m3 is None and torch.equal(_bits(y3), _bits(y)) and torch.equal(_bits(xin3), _bits(xin))
        rc, y4, xin4, m4, r4 = _ln_fwd(K, xd, None, gd, bd)                               # pos = NULL
        y4_ref = N.layernorm_fwd(x, g, b)[0]
        e4 = _rel(y4, _t64(y4_ref))
        print(f"[T={T} D={D}] pos = NULL: y rel err = {e4:.2e}")
        assert rc == 0 and e4 <= LN_FWD and torch.equal(_bits(xin4), _bits(xd))


@pytest.mark.parametrize("D,M", N.FAR_MEAN, ids=[f"{d}@{int(m)}" for d, m in N.FAR_MEAN])
def test_layernorm_forward_far_mean_lattice(K, D, M):
    """rows M + k / 8 summing to D M exactly: the mean must be M, and y stays at the forward bar only with a centred second moment (a float32
    E[x^2] - mean^2 is off by 2e-3 to 8e-2 on these rows: test_norm_rows_host.py)"""
    x = N.far_mean_rows(N.FAR_T, D, M)
    g, b = N.ln_params(D)
    y_ref, _, r_ref = N.layernorm_fwd(x, g, b)
    rc, y, _, mean, rstd = _ln_fwd(K, _d(x), None, _d(g), _d(b))
    e, er = _rel(y, _t64(y_ref)), _rel(rstd, _t64(r_ref))
    print(f"[D={D} M={M}] mean in [{_n(mean).min()!r}, {_n(mean).max()!r}], y rel err = {e:.2e}, rstd rel err = {er:.2e} (bar {LN_FWD:.0e})")
    assert rc == 0 and (_n(mean) == M).all() and e <= LN_FWD and er <= LN_FWD


@pytest.mark.parametrize("D", [4, 260, 2048])
def test_layernorm_forward_constant_rows(K, D):
    """variance 0: rstd = 1 / sqrt(eps) to one ulp and y = beta.  The constants are multiples of a power of two with few digits, so a row's sum and
    its mean are exact"""
    c = np.array([0.0, 1.5, -1024.0, 30000.0, -0.375], np.float32)
    x = np.repeat(c[:, None], D, axis=1)
    g, b = N.ln_params(D)
    for eps in (1e-5, 1e-6):
        rc, y, _, mean, rstd = _ln_fwd(K, _d(x), None, _d(g), _d(b), eps=eps)
        want = np.float32(1.0 / np.sqrt(np.float64(np.float32(eps))))
        ulps = np.abs(_ordered(_n(rstd)) - _ordered(np.full(len(c), want))).max()
        print(f"[D={D} eps={eps}] rstd = {_n(rstd)!r}, 1/sqrt(eps) = {want!r}: {ulps} ulp; y == beta: {bool((_n(y) == b).all())}")
        assert rc == 0 and (_n(mean) == c).all() and ulps <= 1 and (_n(y) == b[None, :]).all()


def test_layernorm_forward_refusals(K):
    D = 8
    x, g, b = _d(np.ones((3, 2052), np.float32)), _d(np.ones(2052, np.float32)), _d(np.zeros(2052, np.float32))
    outs = [_sent(3, 2052), _sent(3, 2052), _sent(3), _sent(3)]                           # xin_out, y, mean, rstd

    def call(xp, gp, bp, yp, T, D):
        return K.lib.act_layernorm_fwd_f32(xp, _p(x), gp, bp, _p(outs[0]), yp, _p(outs[2]), _p(outs[3]), T, D, N.LN_EPS, _st())
    full = (_p(x), _p(g), _p(b), _p(outs[1]))
    got = {"D % 4": call(*full, 3, 6), "D = 0": call(*full, 3, 0), "D = 2052": call(*full, 3, 2052), "T < 0": call(*full, -1, D),
           "x NULL": call(None, *full[1:], 3, D), "gamma NULL": call(full[0], None, *full[2:], 3, D), "beta NULL": call(*full[:2], None, full[3], 3, D),
           "y NULL": call(*full[:3], None, 3, D), "T = 0": call(*full, 0, D)}
    torch.cuda.synchronize()
    print(got, "outputs untouched:", _untouched(*outs))
    assert [got[k] for k in ("D % 4", "D = 0", "D = 2052", "T < 0")] == [ACT_E_BADARG] * 4
    assert [got[k] for k in ("x NULL", "gamma NULL", "beta NULL", "y NULL")] == [ACT_E_NULLPTR] * 4 and got["T = 0"] == 0
    assert _untouched(*outs)
    assert call(*full, 3, 2048) == 0                                                      # the widest row that is accepted


# ---- LayerNorm backward ------------------------------------------------------------------------------------------------------------------------
def _ln_bwd(K, dy, xin, g, mean, rstd, dres=None, params=True, accumulate=0, dg0=None, db0=None, short=0, rpb_env=0):
    """act_layernorm_bwd_f32 with a workspace of exactly act_layernorm_bwd_workspace bytes (``short`` floats less) -> rc, dx, dgamma, dbeta"""
    T, D = dy.shape
    dx = _sent(T, D)
    dg = dg0.clone() if dg0 is not None else (_sent(D) if params else None)
    db = db0.clone() if db0 is not None else (_sent(D) if params else None)
    ws = _Workspace(K.lib.act_layernorm_bwd_workspace(T, D), N.ln_bwd_workspace_floats(T, D, rpb_env))
    rc = K.lib.act_layernorm_bwd_f32(_p(dy), _p(xin), _p(g), _p(mean), _p(rstd), _p(dres), _p(dx), _p(dg), _p(db), accumulate, ws.ptr(),
                                     ws.bytes - 4 * short, T, D, _st())
    ws.check()
    return rc, dx, dg, db


def _ln_bwd_real(K, T, D, rpb_env=0):
    """Gaussian rows through the forward and the backward -> the errors of dx (with dres), dx (without), dgamma, dbeta, and whether dx without
    parameter gradients equals dx with them bit for bit"""
    x, pos, dy, dres = N.ln_real(T, D)
    g, b = N.ln_params(D)
    xin = x + pos
    _, mean, rstd = N.layernorm_fwd(xin, g, b)
    dx_ref, dg_ref, db_ref = N.layernorm_bwd(dy, xin, g, mean, rstd, dres)
    dyd, xd, gd, rd = _d(dy), _d(xin), _d(g), _d(dres)
    rc0, _, _, md, sd = _ln_fwd(K, xd, None, gd, _d(b))
    rc1, dx, dg, db = _ln_bwd(K, dyd, xd, gd, md, sd, rd, rpb_env=rpb_env)
    rc2, dx_plain, dg2, db2 = _ln_bwd(K, dyd, xd, gd, md, sd, None, rpb_env=rpb_env)
    rc3, dx_np, _, _ = _ln_bwd(K, dyd, xd, gd, md, sd, rd, params=False, rpb_env=rpb_env)
    assert (rc0, rc1, rc2, rc3) == (0, 0, 0, 0)
    return {"dx": _rel(dx, _t64(dx_ref)), "dx_nodres": _rel(dx_plain, _t64(dx_ref - dres.astype(np.float64))), "dgamma": _rel(dg, _t64(dg_ref)),
            "dbeta": _rel(db, _t64(db_ref)), "noparams_same_bits": bool(torch.equal(_bits(dx_np), _bits(dx))),
            "params_same_bits": bool(torch.equal(_bits(dg), _bits(dg2)) and torch.equal(_bits(db), _bits(db2)))}


def _ln_bwd_exact(K, T, D, rpb_env=0):
    """the lattice -> the number of dgamma / dbeta elements that differ from the int64 sums, plain and accumulated onto integers, and dx's error"""
    xin, dy, mean, rstd, gamma = N.ln_bwd_lattice(T, D)
    ig, ib = N.ln_bwd_lattice_sums(T, D)
    dx_ref = N.layernorm_bwd(dy, xin, gamma, mean, rstd)[0]
    args = [_d(a) for a in (dy, xin, gamma, mean, rstd)]
    rc, dx, dg, db = _ln_bwd(K, *args, rpb_env=rpb_env)
    base_g, base_b = np.arange(D, dtype=np.float32) - 30, np.float32(1000) - 3 * np.arange(D, dtype=np.float32)
    rc2, dx2, ag, ab = _ln_bwd(K, *args, accumulate=1, dg0=_d(base_g), db0=_d(base_b), rpb_env=rpb_env)
    assert rc == 0 and rc2 == 0
    return {"dgamma": (_n(dg).astype(np.float64), ig), "dbeta": (_n(db).astype(np.float64), ib),
            "dgamma accumulated": (_n(ag).astype(np.float64), ig + base_g), "dbeta accumulated": (_n(ab).astype(np.float64), ib + base_b),
            "dx": _rel(dx, _t64(dx_ref)), "dx_same_bits": bool(torch.equal(_bits(dx), _bits(dx2)))}


def _check_real(tag, e):
    print(f"{tag}: dx {e['dx']:.2e}, dx without dres {e['dx_nodres']:.2e}, dgamma {e['dgamma']:.2e}, dbeta {e['dbeta']:.2e} (bar {LN_BWD:.0e}); "
          f"dx without dgamma / dbeta bit-identical: {e['noparams_same_bits']}; dgamma / dbeta independent of dres: {e['params_same_bits']}")
    assert max(e["dx"], e["dx_nodres"], e["dgamma"], e["dbeta"]) <= LN_BWD and e["noparams_same_bits"] and e["params_same_bits"]


@pytest.mark.parametrize("D", N.LN_D)
def test_layernorm_backward_shapes(K, D):
    for T in N.LN_BWD_T:
        _check_real(f"[T={T} D={D}]", _ln_bwd_real(K, T, D))


def test_layernorm_backward_rows_per_block_grows_and_the_last_workgroup_is_ragged(K):
    T, D = N.LN_BWD_BIG
    assert N.ln_bwd_blocks(T) == (20, 821, 11)
    _check_real(f"[T={T} D={D}] rows_per_block 20, last workgroup 11 rows", _ln_bwd_real(K, T, D))


@pytest.mark.parametrize("T", list(N.LN_EXACT_T))
def test_layernorm_backward_parameter_gradients_are_the_exact_sums(K, T):
    D = N.LN_EXACT_D
    r = _ln_bwd_exact(K, T, D)
    print(f"[T={T} D={D}] nblk = {N.LN_EXACT_T[T]}: dx rel err = {r['dx']:.2e}; dx the same with accumulate_params = 1: {r['dx_same_bits']}")
    for what in ("dgamma", "dbeta", "dgamma accumulated", "dbeta accumulated"):
        _assert_exact(*r[what], f"[T={T}] {what}")
    assert r["dx"] <= LN_BWD and r["dx_same_bits"]


def test_layernorm_backward_workspace_and_refusals(K):
    T, D = 70, N.LN_EXACT_D
    xin, dy, mean, rstd, gamma = (_d(a) for a in N.ln_bwd_lattice(T, D))
    rc, dx, dg, db = _ln_bwd(K, dy, xin, gamma, mean, rstd, short=1)                      # one float less than act_layernorm_bwd_workspace
    torch.cuda.synchronize()
    print(f"workspace one float short: rc = {rc}, outputs untouched: {_untouched(dx, dg, db)}")
    assert rc == ACT_E_BADARG and _untouched(dx, dg, db)
    rc, dx2, _, _ = _ln_bwd(K, dy, xin, gamma, mean, rstd, params=False, short=1)         # without parameter gradients no workspace is needed
    assert rc == 0 and not _untouched(dx2)
    ws = _sent(2 * D * 8)
    for bad in ((T, 6), (T, 0), (T, 2052), (-1, D)):
        assert K.lib.act_layernorm_bwd_f32(_p(dy), _p(xin), _p(gamma), _p(mean), _p(rstd), None, _p(dx), _p(dg), _p(db), 0, _p(ws), ws.numel() * 4,
                                           *bad, _st()) == ACT_E_BADARG, bad
    for i in (0, 1, 2, 3, 4, 6):
        a = [_p(dy), _p(xin), _p(gamma), _p(mean), _p(rstd), None, _p(dx), _p(dg), _p(db)]
        a[i] = None
        assert K.lib.act_layernorm_bwd_f32(*a, 0, _p(ws), ws.numel() * 4, T, D, _st()) == ACT_E_NULLPTR, i
    assert K.lib.act_layernorm_bwd_f32(_p(dy), _p(xin), _p(gamma), _p(mean), _p(rstd), None, _p(dx), _p(dg), _p(db), 0, _p(ws), ws.numel() * 4, 0, D,
                                       _st()) == 0
    torch.cuda.synchronize()
    assert _untouched(dx, dg, db)


# ---- the ACT_LN_BWD_WAVES / ACT_LN_BWD_RPB forms -----------------------------------------------------------------------------------------------
# (waves, rows per block or None, D): 16 waves on 32-row workgroups -> <16, 2>; ACT_LN_BWD_RPB = 4 -> four-row workgroups, which fall back to four
# waves whatever ACT_LN_BWD_WAVES says (25 partial rows at T = 100); 8 waves on the default 16-row workgroups -> <8, 2> and, at D = 1024, <8, 4>
CHILDREN = [(16, 32, (260, 512)), (8, 4, (260, 512, 1024)), (8, None, (260, 512, 1024))]
CHILD_T = (1, 33, 100)


def _child():
    """run by test_layernorm_backward_wave_forms in a fresh interpreter with ACT_LN_BWD_WAVES / ACT_LN_BWD_RPB set: prints one JSON line"""
    K = _kernels()
    rpb = int(os.environ.get("ACT_LN_BWD_RPB", "0"))
    out = []
    for D in json.loads(os.environ["NORM_ROWS_CHILD_D"]):
        for T in CHILD_T:
            rec = {"D": D, "T": T, "blocks": N.ln_bwd_blocks(T, rpb), "real": _ln_bwd_real(K, T, D, rpb)}
            ex = _ln_bwd_exact(K, T, D, rpb)
            rec["exact"] = {k: (int((~(v[0] == v[1])).sum()) if isinstance(v, tuple) else v) for k, v in ex.items()}
            out.append(rec)
    torch.cuda.synchronize()
    print("child-json " + json.dumps(out))


@pytest.mark.parametrize("waves,rpb,Ds", CHILDREN, ids=[f"waves{w}-rpb{r}" for w, r, _ in CHILDREN])
def test_layernorm_backward_wave_forms(waves, rpb, Ds):
    env = dict(os.environ, ACT_LN_BWD_WAVES=str(waves), NORM_ROWS_CHILD_D=json.dumps(list(Ds)))
    env.pop("ACT_LN_BWD_RPB", None)
    if rpb is not None:
        env["ACT_LN_BWD_RPB"] = str(rpb)
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_norm_rows_edges as T; T._child()"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith("child-json ")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-4000:] + r.stderr[-4000:]
    recs = json.loads(lines[0][len("child-json "):])
    assert [(c["D"], c["T"]) for c in recs] == [(D, T) for D in Ds for T in CHILD_T]
    for c in recs:
        tag = f"[waves={waves} rpb={rpb} T={c['T']} D={c['D']}] (rows per block, nblk, last) = {tuple(c['blocks'])}"
        ex = c["exact"]
        print(f"{tag}: elements off the exact sums: dgamma {ex['dgamma']}, dbeta {ex['dbeta']}, accumulated {ex['dgamma accumulated']}, "
              f"{ex['dbeta accumulated']}; lattice dx {ex['dx']:.2e}")
    for c in recs:
        _check_real(f"[waves={waves} rpb={rpb} T={c['T']} D={c['D']}]", c["real"])
        ex = c["exact"]
        assert (ex["dgamma"], ex["dbeta"], ex["dgamma accumulated"], ex["dbeta accumulated"]) == (0, 0, 0, 0) and ex["dx"] <= LN_BWD and ex["dx_same_bits"]


# ---- act_colsum_f32 ----------------------------------------------------------------------------------------------------------------------------
def _colsum(K, x, R, C, ld, accumulate=0, out0=None, short=0):
    out = out0.clone() if out0 is not None else _sent(C)
    ws = _Workspace(K.lib.act_colsum_workspace(R, C), N.colsum_workspace_floats(R, C))
    rc = K.lib.act_colsum_f32(_p(x), R, C, ld, _p(out), accumulate, ws.ptr(), ws.bytes - 4 * short, _st())
    ws.check()
    return rc, out


def _padded(x, pad):
    """x [R,C] -> a device buffer [max(R, 1), C + pad] with NaN in the padding columns (a NaN in a sum: they were read)"""
    R, C = x.shape
    buf = np.full((max(R, 1), C + pad), np.nan, np.float32)
    buf[:R, :C] = x
    if R == 0:
        buf[:] = np.nan                                                                   # no row may be read at all
    return _d(buf)


@pytest.mark.parametrize("R,C", N.COLSUM_SHAPES, ids=_ids(N.COLSUM_SHAPES))
def test_colsum_on_the_lattice(K, R, C):
    x = N.colsum_lattice(R, C)
    ref = x.astype(np.int64).sum(0)
    base = (np.arange(C) % 17 - 8).astype(np.float32)
    print(f"[{R}x{C}] (parts, rows per block, nparts, rows of the last part) = {N.COLSUM[(R, C)]}")
    for pad in (0, 3):
        xd = _padded(x, pad)
        rc, out = _colsum(K, xd, R, C, C + pad)
        assert rc == 0
        _assert_exact(_n(out), ref, f"[{R}x{C} ld={C + pad}] column sums")
        rc, acc = _colsum(K, xd, R, C, C + pad, accumulate=1, out0=_d(base))
        assert rc == 0
        _assert_exact(_n(acc), ref + base.astype(np.int64), f"[{R}x{C} ld={C + pad}] accumulated column sums")


def test_colsum_real_values_workspace_and_refusals(K):
    R, C = 1000, 130
    x = N.ln_real(R, C)[0]
    rc, out = _colsum(K, _d(x), R, C, C)
    e = _rel(out, _t64(N.colsum(x)))
    print(f"[{R}x{C}] Gaussian rows: column sums rel err = {e:.2e} (bar {BIAS:.0e})")
    assert rc == 0 and e <= BIAS
    assert torch.equal(_kernels().colsum(_d(x)), out)                                     # the wrapper: the same launch
    rc, out = _colsum(K, _d(x), R, C, C, short=1)
    torch.cuda.synchronize()
    print(f"workspace one float short: rc = {rc}, output untouched: {_untouched(out)}")
    assert rc == ACT_E_BADARG and _untouched(out)
    ws = _sent(1024 * C)
    assert K.lib.act_colsum_f32(_p(out), -1, C, C, _p(out), 0, _p(ws), ws.numel() * 4, _st()) == ACT_E_BADARG
    assert K.lib.act_colsum_f32(_p(out), R, 0, C, _p(out), 0, _p(ws), ws.numel() * 4, _st()) == ACT_E_BADARG
    assert K.lib.act_colsum_f32(None, R, C, C, _p(out), 0, _p(ws), ws.numel() * 4, _st()) == ACT_E_NULLPTR
    assert K.lib.act_colsum_f32(_p(ws), R, C, C, None, 0, _p(ws), ws.numel() * 4, _st()) == ACT_E_NULLPTR
    assert K.lib.act_colsum_f32(_p(ws), R, C, C, _p(out), 0, None, ws.numel() * 4, _st()) == ACT_E_NULLPTR
    torch.cuda.synchronize()
    assert _untouched(out)


# ---- cross-entropy -----------------------------------------------------------------------------------------------------------------------------
def _xent(K, z, lab, g=1.0, want_acc=True):
    """the C entries -> loss, acc (or None), row_buf [3,R] = {row maximum, row loss, log sum exp(z - maximum), sign bit: arg-max == label}, dz"""
    R, C = z.shape
    zd, ld = _d(z), _d(lab, torch.int64)
    loss, acc, buf, dz = _sent(1), (_sent(1) if want_acc else None), _sent(3, R), _sent(R, C)
    assert K.lib.act_softmax_xent_fwd_f32(_p(zd), _p(ld), R, C, _p(loss), _p(buf), _p(acc), _st()) == 0
    assert K.lib.act_softmax_xent_bwd_f32(_p(zd), _p(ld), _p(buf), _p(_d(np.array([g], np.float32))), R, C, _p(dz), _st()) == 0
    return loss, acc, buf, dz


def _flags(buf):
    """per row: arg-max == label (the sign bit of row 2 of row_buf)"""
    return np.signbit(_n(buf[2])).astype(np.float32)


def _check_xent(K, tag, z, lab, g=2.5):
    R = z.shape[0]
    l_ref, lse_ref, top1, dz_ref = N.xent(z, lab, g)
    loss, acc, buf, dz = _xent(K, z, lab, g)
    lse = _n(buf[0]).astype(np.float64) + np.abs(_n(buf[2]).astype(np.float64))
    el, es, ed = abs(loss.item() - l_ref) / max(1.0, abs(l_ref)), N.rel(lse, lse_ref), _rel(dz, _t64(dz_ref))
    hits = int(round(top1 * R))
    print(f"{tag}: loss {loss.item()!r} vs {l_ref!r}: {el:.2e} (bar {XENT_LOSS:.0e}), lse {es:.2e}, dz {ed:.2e} (bar {XENT_DZ:.0e}), "
          f"top-1 {acc.item()!r} vs {hits} / {R}")
    assert np.isfinite(loss.item()) and el <= XENT_LOSS and es <= XENT_LOSS and ed <= XENT_DZ
    assert acc.item() == float(np.float32(hits) / np.float32(R)) and int(_flags(buf).sum()) == hits
    return loss, acc, buf, dz


@pytest.mark.parametrize("R,C", N.XENT_SHAPES, ids=_ids(N.XENT_SHAPES))
def test_cross_entropy_shapes(K, R, C):
    z, lab = N.xent_input(R, C)
    loss, acc, buf, dz = _check_xent(K, f"[{R}x{C}]", z, lab)
    zd = _d(z).requires_grad_(True)
    l2, a2 = K.softmax_xent(zd, _d(lab, torch.int64))                                     # the autograd wrapper: the same launches
    (l2 * 2.5).backward()
    assert torch.equal(l2.reshape(1), loss) and torch.equal(a2.reshape(1), acc) and torch.equal(_bits(zd.grad), _bits(dz))
    l3, a3, _, _ = _xent(K, z, lab, want_acc=False)                                       # acc_out = NULL
    assert a3 is None and torch.equal(l3, loss)


@pytest.mark.parametrize("C", [3, 65, 130])
def test_cross_entropy_ties_go_to_the_lowest_index(K, C):
    """the row maximum at {c, c + 64} (two columns of one lane), at {c, c + 1} (two lanes) and in every column; labels on the lower and on the
    higher of the two, so that a wrong arg-max changes the fraction"""
    r = np.random.default_rng(C)
    rows, first, labs = [], [], []
    pairs = [(c, c + 64) for c in (0, 1, 63, C - 65) if 0 <= c and c + 64 < C] + [(c, c + 1) for c in (0, 62, 63, 64, C - 2) if 0 <= c and c + 1 < C]
    for lo, hi in pairs:
        for lab in (lo, hi):
            row = r.standard_normal(C).astype(np.float32)
            row[[lo, hi]] = 9.0
            rows.append(row); first.append(lo); labs.append(lab)
    for lab in (0, C - 1):
        rows.append(np.full(C, -1.25, np.float32)); first.append(0); labs.append(lab)     # an all-equal row: index 0
    z, lab = np.stack(rows), np.array(labs)
    loss, acc, buf, dz = _check_xent(K, f"[ties, C={C}, {len(rows)} rows]", z, lab)
    flags = _flags(buf)
    print(f"[ties, C={C}] per-row arg-max == label: {flags.astype(int).tolist()}, expected {(np.array(first) == lab).astype(int).tolist()}")
    assert np.array_equal(flags, (np.array(first) == lab).astype(np.float32))


@pytest.mark.parametrize("R,C", [(5, 63), (9, 65)])
def test_cross_entropy_large_logits(K, R, C):
    z = (1e4 * np.resize(np.array([-1.0, 0.0, 1.0], np.float32), (R, C))).astype(np.float32)
    lab = (np.arange(R) * 7) % C                                                          # labels on all three values
    _check_xent(K, f"[1e4 {{-1, 0, 1}}, {R}x{C}]", z, lab, g=1.0)


def test_cross_entropy_minus_infinity_logits(K):
    R, C = 9, 65
    z, lab = (a.copy() for a in N.xent_input(R, C))
    off = np.ones(C, bool)
    off[[3, 64]] = False                                                                  # classes 3 and 64 do not exist
    lab[lab == 3] = 4; lab[lab == 64] = 5
    zi = z.copy(); zi[:, ~off] = -np.inf
    loss, acc, buf, dz = _check_xent(K, "[-inf off the label]", zi, lab)
    small = _xent(K, z[:, off], (np.cumsum(off) - 1)[lab])[0]
    print(f"loss {loss.item()!r}, without those classes {small.item()!r}; dz there: {_n(dz)[:, ~off].tolist()}")
    assert abs(loss.item() - small.item()) <= XENT_LOSS * max(1.0, abs(small.item())) and (_n(dz)[:, ~off] == 0).all()
    zi[2, lab[2]] = -np.inf                                                               # -inf on the label: +inf, as torch gives
    loss = _xent(K, zi, lab)[0]
    print(f"-inf on the label: loss = {loss.item()!r}")
    assert loss.item() == float("inf") == N.xent(zi, lab)[0]


def test_cross_entropy_refusals(K):
    z, lab, out = _d(np.zeros((2, 3), np.float32)), _d(np.zeros(2), torch.int64), [_sent(1), _sent(3, 2), _sent(1), _sent(2, 3)]
    fwd = lambda zp, lp, R, C, lo, bp: K.lib.act_softmax_xent_fwd_f32(zp, lp, R, C, lo, bp, _p(out[2]), _st())
    bwd = lambda zp, lp, bp, gp, R, C, dp: K.lib.act_softmax_xent_bwd_f32(zp, lp, bp, gp, R, C, dp, _st())
    assert fwd(_p(z), _p(lab), 0, 3, _p(out[0]), _p(out[1])) == ACT_E_BADARG and fwd(_p(z), _p(lab), 2, 0, _p(out[0]), _p(out[1])) == ACT_E_BADARG
    for i in range(4):
        a = [_p(z), _p(lab), 2, 3, _p(out[0]), _p(out[1])]
        a[i if i < 2 else i + 2] = None
        assert fwd(*a) == ACT_E_NULLPTR, i
    g = _d(np.ones(1, np.float32))
    assert bwd(_p(z), _p(lab), _p(out[1]), _p(g), 0, 3, _p(out[3])) == ACT_E_BADARG and bwd(_p(z), _p(lab), _p(out[1]), _p(g), 2, 0, _p(out[3])) == ACT_E_BADARG
    for i in (0, 1, 2, 3, 6):
        a = [_p(z), _p(lab), _p(out[1]), _p(g), 2, 3, _p(out[3])]
        a[i] = None
        assert bwd(*a) == ACT_E_NULLPTR, i
    torch.cuda.synchronize()
    assert _untouched(*out)


# ---- l2 / smoothl1 -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reg_input(R, D):
    r = np.random.default_rng(3 * R + D)
    return (2 * r.standard_normal((R, D))).astype(np.float32), r.standard_normal((R, D)).astype(np.float32)


def _check_regression(K, tag, s, t, kind):
    loss_ref, ds_ref = N.regression(s, t, kind, 3.0)
    sg = _d(s).requires_grad_(True)
    loss = K.regression_distill_loss(sg, _d(t), ("l2", "smoothl1")[kind])
    (loss * 3.0).backward()
    el, ed = abs(loss.item() - loss_ref) / max(1.0, abs(loss_ref)), _rel(sg.grad, _t64(ds_ref))
    print(f"{tag} kind {kind}: loss {loss.item()!r} vs {loss_ref!r}: {el:.2e}, ds {ed:.2e} (bar {REG:.0e})")
    assert el <= REG and ed <= REG
    return sg.grad


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("R,D", N.REG_SHAPES, ids=_ids(N.REG_SHAPES))
def test_regression_losses_shapes(K, R, D, kind):
    _check_regression(K, f"[{R}x{D}]", *_reg_input(R, D), kind)


@pytest.mark.parametrize("kind", [0, 1])
def test_regression_losses_at_the_knee(K, kind):
    """d = s - t exactly at +-1, one ulp inside, one ulp outside, 0 and +-3, a row of nothing else (so the row's loss is not drowned) and a row of
    Gaussians around them"""
    n = len(N.KNEE)
    s, t = (a[:2, :n + 4].copy() for a in _reg_input(5, 63))
    s[:, :n] = np.array(N.KNEE, np.float32); t[:, :n] = 0
    s[0, n:] = 0; t[0, n:] = 0
    ds = _n(_check_regression(K, "[knee]", s, t, kind))
    want = N.regression(s, t, kind, 3.0)[1][0, :n]
    print(f"[knee] kind {kind}: ds at d = {N.KNEE}: {ds[0, :n].tolist()}")
    assert np.abs(ds[0, :n] - want).max() <= REG


def test_regression_losses_refuse_an_unknown_kind(K):
    s, out = _d(np.zeros((2, 4), np.float32)), [_sent(1), _sent(2), _sent(2, 4)]
    g = _d(np.ones(1, np.float32))
    for kind in (-1, 2):
        assert K.lib.act_regression_loss_fwd_f32(_p(s), _p(s), 2, 4, kind, _p(out[0]), _p(out[1]), _st()) == ACT_E_BADARG
        assert K.lib.act_regression_loss_bwd_f32(_p(s), _p(s), _p(g), 2, 4, kind, _p(out[2]), _st()) == ACT_E_BADARG
    assert K.lib.act_regression_loss_fwd_f32(_p(s), _p(s), 0, 4, 0, _p(out[0]), _p(out[1]), _st()) == ACT_E_BADARG
    assert K.lib.act_regression_loss_fwd_f32(None, _p(s), 2, 4, 0, _p(out[0]), _p(out[1]), _st()) == ACT_E_NULLPTR
    torch.cuda.synchronize()
    assert _untouched(*out)


# ---- cosine ------------------------------------------------------------------------------------------------------------------------------------
def _cosine(K, s, t, g=3.0):
    """K.cosine_distill_loss -> loss (float), ds (numpy), and the row losses through the C entry"""
    sg = _d(s).requires_grad_(True)
    td = _d(t)
    loss = K.cosine_distill_loss(sg, td)
    (loss * g).backward()
    R, D = s.shape
    out = [_sent(1), _sent(R), _sent(R, 3)]
    assert K.lib.act_cosine_loss_fwd_f32(_p(sg.detach()), _p(td), R, D, N.COS_EPS, *(_p(o) for o in out), _st()) == 0
    assert torch.equal(out[0], loss.reshape(1))
    return loss.item(), _n(sg.grad), _n(out[1])


def _check_cosine(K, tag, s, t, g=3.0):
    loss_ref, row_ref, ds_ref = N.cosine(s, t, g=g)
    loss, ds, row = _cosine(K, s, t, g)
    el, er, ed = abs(loss - loss_ref), N.rel(row, row_ref), N.rel(ds, ds_ref)
    print(f"{tag}: loss {loss!r} vs {loss_ref!r}: {el:.2e}, row loss {er:.2e}, ds {ed:.2e} (max|ds| = {np.abs(ds_ref).max():.3e}; bar {COS:.0e})")
    assert el <= COS and er <= COS and ed <= COS
    return loss, ds, row


@pytest.mark.parametrize("R,D", N.COS_SHAPES, ids=_ids(N.COS_SHAPES))
def test_cosine_loss_shapes(K, R, D):
    _check_cosine(K, f"[{R}x{D}]", *N.cos_input(R, D))


@pytest.mark.parametrize("ks,kt", [(-20, 0), (0, -20), (-20, -20), (40, 0), (0, 40), (40, 40), (40, -20)],
                         ids=lambda k: f"2^{k}")
def test_cosine_loss_scaled_rows(K, ks, kt):
    """s 2^ks, t 2^kt: a power of two changes exponents only, so cos is the same and ds is 2^-ks times the unscaled one, at the unscaled bar"""
    s, t = N.cos_input(204, 384)
    s2, t2 = (s * np.float32(2.0 ** ks)).astype(np.float32), (t * np.float32(2.0 ** kt)).astype(np.float32)
    loss0, ds0, row0 = _cosine(K, s, t)
    loss_ref, row_ref, ds_ref = N.cosine(s2, t2, g=3.0)
    loss, ds, row = _cosine(K, s2, t2)
    back = ds.astype(np.float64) * 2.0 ** ks                                              # exact: a power of two
    el, er, ed = abs(loss - loss_ref), N.rel(row, row_ref), N.rel(back, ds_ref * 2.0 ** ks)
    print(f"[s 2^{ks}, t 2^{kt}] loss {loss!r} vs {loss_ref!r}: {el:.2e}, row loss {er:.2e}, ds 2^{ks} {ed:.2e} (bar {COS:.0e}); "
          f"bit-identical to the unscaled run: row loss {np.array_equal(row, row0)}, ds {np.array_equal(back.astype(np.float32), ds0)}")
    assert np.isfinite(ds).all() and el <= COS and er <= COS and ed <= COS


def test_cosine_loss_clamp_region(K):
    """a zero student row, a zero teacher row, both zero, a student and a teacher row of norm 1e-10 (eps = 1e-8), against F.cosine_similarity's
    definition: every norm clamped on its own.  ds is compared row by row, each relative to its own largest element"""
    s, t, names = N.cos_clamp_input()
    g, R = 3.0, len(names)
    loss_ref, row_ref, ds_ref = N.cosine(s, t, g=g)
    loss, ds, row = _cosine(K, s, t, g)
    errs = [N.rel(ds[i] / max(1.0, np.abs(ds_ref[i]).max()), ds_ref[i] / max(1.0, np.abs(ds_ref[i]).max())) for i in range(R)]
    for i, name in enumerate(names):
        print(f"[{name}] row loss {row[i]!r} vs {row_ref[i]!r}; max|ds| {np.abs(ds[i]).max():.6e} vs {np.abs(ds_ref[i]).max():.6e}, rel err {errs[i]:.2e}")
    print(f"loss {loss!r} vs {loss_ref!r} (bar {COS:.0e})")
    assert abs(loss - loss_ref) <= COS and N.rel(row, row_ref) <= COS and max(errs) <= COS
    assert row[1] == 1.0 and row[2] == 1.0 and row[3] == 1.0 and (ds[3] == 0).all() and (ds[2] == 0).all()
    tn = np.linalg.norm(t[1].astype(np.float64))
    assert N.rel(ds[1] * 1e-7, -g / R * t[1].astype(np.float64) / (tn * N.COS_EPS) * 1e-7) <= COS          # -g / R t / (|t| eps)


# ---- row gate, add, prompt rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,D,rps", N.SCALE_ROWS, ids=_ids(N.SCALE_ROWS))
def test_scale_rows(K, T, D, rps):
    r = np.random.default_rng(T + D)
    x = r.standard_normal((T, D)).astype(np.float32)
    gate = r.choice(np.array([0.0, 1.0 / (1 - 0.1), 1.0 / (1 - 0.25), 1.0], np.float32), (T + rps - 1) // rps)
    gate[:2] = np.array([1.0 / (1 - 0.1), 0.0], np.float32)[:len(gate)]
    ref = N.scale_rows(x, gate, rps)
    xd, gd, y = _d(x), _d(gate), _sent(T, D)
    assert K.lib.act_scale_rows_f32(_p(xd), _p(gd), T, D, rps, _p(y), _st()) == 0
    same = np.array_equal(_n(y).view(np.int32), ref.view(np.int32))
    assert K.lib.act_scale_rows_f32(_p(xd), _p(gd), T, D, rps, _p(xd), _st()) == 0       # y == x: in place
    inplace = np.array_equal(_n(xd).view(np.int32), ref.view(np.int32))
    print(f"[T={T} D={D} rows per gate {rps}] {T * D // 4} float4, gates {sorted(set(gate.tolist()))}: bit-identical {same}, in place {inplace}")
    assert same and inplace
    if T == 7:
        out = _sent(T, D)
        bad = [K.lib.act_scale_rows_f32(_p(xd), _p(gd), T, 6, rps, _p(out), _st()), K.lib.act_scale_rows_f32(_p(xd), _p(gd), T, D, 0, _p(out), _st()),
               K.lib.act_scale_rows_f32(_p(xd), _p(gd), -1, D, rps, _p(out), _st()), K.lib.act_scale_rows_f32(_p(xd), _p(gd), 0, D, rps, _p(out), _st()),
               K.lib.act_scale_rows_f32(None, _p(gd), T, D, rps, _p(out), _st())]
        torch.cuda.synchronize()
        assert bad == [ACT_E_BADARG] * 3 + [0, ACT_E_NULLPTR] and _untouched(out)


@pytest.mark.parametrize("n", N.ADD_N)
def test_add(K, n):
    r = np.random.default_rng(n + 1)
    a, b = r.standard_normal(n + 4).astype(np.float32), r.standard_normal(n + 4).astype(np.float32)
    a[n:] = SENT                                                                          # four sentinels behind the n elements
    ref = N.add(a[:n], b[:n])
    ad, bd, out = _d(a), _d(b), _sent(n + 4)
    assert K.lib.act_add_f32(_p(ad), _p(bd), _p(out), n, _st()) == 0
    plain = np.array_equal(_n(out[:n]).view(np.int32), ref.view(np.int32)) and _untouched(out[n:])
    a2 = ad.clone()
    assert K.lib.act_add_f32(_p(a2), _p(bd), _p(a2), n, _st()) == 0                       # out aliases a
    b2 = bd.clone()
    assert K.lib.act_add_f32(_p(ad), _p(b2), _p(b2), n, _st()) == 0                       # out aliases b
    alias_a = np.array_equal(_n(a2[:n]).view(np.int32), ref.view(np.int32)) and _untouched(a2[n:])
    alias_b = np.array_equal(_n(b2[:n]).view(np.int32), ref.view(np.int32)) and torch.equal(b2[n:], bd[n:])
    print(f"[n={n}] {n // 4} float4: bit-identical {plain}, out = a {alias_a}, out = b {alias_b}")
    assert plain and alias_a and alias_b


def test_add_refusals(K):
    a, b, out = _d(np.ones(16, np.float32)), _d(np.ones(16, np.float32)), _sent(16)
    got = [K.lib.act_add_f32(_p(a), _p(b), _p(out), 6, _st()), K.lib.act_add_f32(_p(a), _p(b), _p(out), -4, _st()),
           K.lib.act_add_f32(_p(a) + 4, _p(b), _p(out), 8, _st()), K.lib.act_add_f32(_p(a), _p(b) + 4, _p(out), 8, _st()),
           K.lib.act_add_f32(_p(a), _p(b), _p(out) + 4, 8, _st()), K.lib.act_add_f32(None, _p(b), _p(out), 8, _st()),
           K.lib.act_add_f32(_p(a), _p(b), None, 8, _st())]
    torch.cuda.synchronize()
    print(got, "output untouched:", _untouched(out))
    assert got == [ACT_E_BADARG] * 5 + [ACT_E_NULLPTR] * 2 and _untouched(out)


def test_prompt_rows_past_the_grid_cap(K):
    """B P D / 4 > 8192 * 256 with an injected mask and p = 0.5 (inv_keep = 2: every product exact).  Forward: tok mask 2 + ppos, one rounding
    per element; backward on integers: dtok and dppos are the int64 sums over the B clouds"""
    B, P, D = N.PROMPT
    r = np.random.default_rng(B)
    tok, ppos = r.standard_normal((P, D)).astype(np.float32), r.standard_normal((P, D)).astype(np.float32)
    mask = (r.random((B * P, D)) < 0.5).astype(np.float32)
    dy = r.integers(-2, 3, (B * P, D)).astype(np.float32)
    y_ref = (np.tile(tok, (B, 1)) * mask * np.float32(2) + np.tile(ppos, (B, 1))).astype(np.float32)
    assert np.array_equal(y_ref, N.prompt_rows_fwd(tok, ppos, mask, B, 2.0).astype(np.float32))
    td, pd, md = _d(tok).requires_grad_(True), _d(ppos).requires_grad_(True), _d(mask)
    y = K.prompt_rows(td, pd, B, drop_p=0.5, seed=0, mask=md.view(B, P, D))
    same = np.array_equal(_n(y).view(np.int32), y_ref.view(np.int32))
    print(f"[B={B} P={P} D={D}] {B * P * D // 4} float4 (grid cap {N.GRID_CAP}): forward bit-identical {same}")
    assert same
    y.backward(_d(dy))
    dtok, dppos = N.prompt_rows_bwd(dy, mask, B, P, 2.0)
    _assert_exact(_n(td.grad), dtok, "dtok")
    _assert_exact(_n(pd.grad), dppos, "dppos")
