"""Host restatement of csrc/augment.hip (test infrastructure, the role of tests/philox_ref.py): the seven ops of the fused augmentation chain in
numpy float32 -- one rounding per product and sum, as the kernel is built without contraction -- and the Philox draw layout, written from the
text of include/act_hip.h: key = seed ^ (counter * 0x9E3779B97F4A7C15), counter words (slot, cloud, 3, position + 8 sub), a uniform is
(word >> 8) * 2^-24, Box-Muller with its first uniform ((word >> 8) + 1) * 2^-24.  The Box-Muller and the rotation's sine / cosine are evaluated
in float64 here; the kernel's fp32 functions are held to the bars of tests/test_gpu_augment.py.

ops: [(kind, p0, p1, p2), ...]; draws: per op a tuple in the order of act_augment_op_t.draws / draws2 (what kernels.augment takes)."""
import os

import numpy as np

from tests.philox_ref import philox4x32_10, _fold_counter, PHILOX_DOMAIN_AUGMENT

SCALE, TRANSLATE, SCALE_TRANSLATE, ROTATE_Y, JITTER, DROPOUT, FLIP = 1, 2, 3, 4, 5, 6, 7
F = np.float32
_U = F(2.0 ** -24)


def _u01(words):
    return (words >> np.uint64(8)).astype(np.float32) * _U                   # exact: 24 bits times a power of two


def _words(slot, cloud, pos, sub, seed, ctr, log=None):
    slot, cloud = np.broadcast_arrays(np.asarray(slot), np.asarray(cloud))
    if log is not None:
        log.extend((int(s), int(c), PHILOX_DOMAIN_AUGMENT, pos + 8 * sub) for s, c in zip(slot.ravel(), cloud.ravel()))
    return philox4x32_10(slot, cloud, PHILOX_DOMAIN_AUGMENT, pos + 8 * sub, _fold_counter(seed, ctr))


def philox_draws(ops, B, N, seed, ctr=None, log=None):
    """the draws the kernel takes from Philox for this chain, in the injectable form; ``log`` (a list) receives every counter used"""
    out = []
    b = np.arange(B)
    for pos, (kind, p0, p1, p2) in enumerate(ops):
        cloud = lambda slot: _u01(_words(slot, b, pos, 0, seed, ctr, log))                    # [B, 4] uniforms of one per-cloud counter
        point = lambda: _words(np.arange(N)[None, :], b[:, None], pos, 1, seed, ctr, log)     # [B, N, 4] words of the per-point counters
        scale = lambda u: F(p0) + (F(p1) - F(p0)) * u
        shift = lambda u, r: -F(r) + (F(2.0) * F(r)) * u
        if kind == SCALE:
            out.append((scale(cloud(0)[:, :3]),))
        elif kind == TRANSLATE:
            out.append((shift(cloud(0)[:, :3], p0),))
        elif kind == SCALE_TRANSLATE:
            out.append((scale(cloud(0)[:, :3]), shift(cloud(1)[:, :3], p2)))
        elif kind == ROTATE_Y:
            out.append((cloud(0)[:, 0],))
        elif kind == JITTER:
            w = point()
            top = (w >> np.uint64(8)).astype(np.float64)
            r01, r23 = np.sqrt(-2.0 * np.log((top[..., 0] + 1.0) * 2.0 ** -24)), np.sqrt(-2.0 * np.log((top[..., 2] + 1.0) * 2.0 ** -24))
            a1, a3 = 2.0 * np.pi * top[..., 1] * 2.0 ** -24, 2.0 * np.pi * top[..., 3] * 2.0 ** -24
            out.append((np.stack((r01 * np.cos(a1), r01 * np.sin(a1), r23 * np.cos(a3)), axis=-1).astype(np.float32),))
        elif kind == DROPOUT:
            out.append((cloud(0)[:, 0], _u01(point()[..., 0])))
        elif kind == FLIP:
            out.append((cloud(0)[:, :3],))
        else:
            raise ValueError(kind)
    return out


def rotation(u):
    """(cos, sin) of the angle 2 pi u, evaluated in float64 and rounded to float32"""
    ang = 2.0 * np.pi * np.asarray(u, dtype=np.float64)
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def apply(pc, ops, draws):
    """the chain on a copy of pc float32 [B, N, 3]; every op sees the cloud as the earlier ops left it"""
    p = np.array(pc, dtype=np.float32, copy=True)
    B, N, _ = p.shape
    for (kind, p0, p1, p2), d in zip(ops, draws):
        d = [None if t is None else np.asarray(t) for t in d]
        if kind == SCALE:
            p = p * d[0].astype(np.float32)[:, None, :]
        elif kind == TRANSLATE:
            p = p + d[0].astype(np.float32)[:, None, :]
        elif kind == SCALE_TRANSLATE:
            p = (p * d[0].astype(np.float32)[:, None, :]) + d[1].astype(np.float32)[:, None, :]
        elif kind == ROTATE_Y:
            c, s = rotation(d[0])
            c, s, z, o = c[:, None], s[:, None], F(0.0), F(1.0)
            x, y, w = p[..., 0], p[..., 1], p[..., 2]
            p = np.stack(((x * c + y * z) + w * (-s), (x * z + y * o) + w * z, (x * s + y * z) + w * c), axis=-1).astype(np.float32)
        elif kind == JITTER:
            p = p + np.clip(F(p0) * d[0].astype(np.float32), -F(p1), F(p1))
        elif kind == DROPOUT:
            ratio = d[0].astype(np.float32) * F(p0)
            drop = d[1].astype(np.float32) <= ratio[:, None]
            p = np.where(drop[..., None], p[:, :1, :], p)
        elif kind == FLIP:
            u = d[0].astype(np.float32)
            horz = [a for a in range(3) if a != int(p0)]
            for i in range(B):
                if u[i, 0] < F(0.95):
                    for slot, ax in enumerate(horz, start=1):
                        if u[i, slot] < F(0.5):
                            p[i, :, ax] = p[i, :, ax].max() - p[i, :, ax]
        else:
            raise ValueError(kind)
        assert p.dtype == np.float32
    return p


# ---- the reference's recorded outputs (tests/golden/g22_transforms.npz) and the bars they are held to, shared by the host and the GPU tests ----
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_transforms.npz")
D3 = (0., 0., 0.)
# op name in the golden -> (op, the golden's draw keys in the order of the op's draw pointers); parameters are the reference's defaults
GOLDEN_OPS = {
    "scale": ((SCALE, 2. / 3., 3. / 2., 0.), ("scale_scale",)),
    "translate": ((TRANSLATE, 0.2, 0., 0.), ("translate_shift",)),
    "st": ((SCALE_TRANSLATE, 2. / 3., 3. / 2., 0.2), ("st_scale", "st_shift")),
    "rotate": ((ROTATE_Y,) + D3, ("rotate_u",)),
    "jitter": ((JITTER, 0.01, 0.05, 0.), ("jitter_noise",)),
    "dropout": ((DROPOUT, 0.5, 0., 0.), ("dropout_ratio", "dropout_drop_u")),
    "flip": ((FLIP, 2., 0., 0.), ("flip_u",)),
}
ROTATE_ATOL = 2e-6      # the reference multiplies by a float32-cast matrix in torch's summation order; |coordinates| <= 2, two products of ~1.2e-7 relative error each


def check_against_golden(name, got, want):
    """the bars of the issue: bit-exact for scale, translate, scale-and-translate, dropout and flip; 1 ulp of the sum for jitter; 2e-6 for rotate"""
    if name == "rotate":
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"{name}: max abs error {err:.3e} (bar {ROTATE_ATOL})")
        assert err <= ROTATE_ATOL
    elif name == "jitter":
        ulp = np.maximum(np.spacing(np.abs(want)), np.spacing(np.abs(got)))
        worst = (np.abs(got.astype(np.float64) - want) / ulp).max()
        print(f"{name}: worst error {worst:.2f} ulp of the sum (bar 1)")
        assert worst <= 1.0
    else:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
