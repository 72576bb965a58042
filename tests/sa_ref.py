"""numpy restatement of the set-abstraction kernels (act_amd/csrc/sa.hip): the radius search, the grouped rows and their adjoint.
Test infrastructure only; every float32 chain is written out operation by operation so that it rounds where the kernel rounds."""
import numpy as np

F = np.float32


def sqdist(q, p):
    """q [S,3], p [N,3] float32 -> [S,N] float32, the difference form (dx*dx + dy*dy) + dz*dz with every product and sum rounded"""
    q, p = np.asarray(q, F), np.asarray(p, F)
    d = (q[:, None, :] - p[None, :, :]).astype(F)
    return ((d[..., 0] * d[..., 0]).astype(F) + (d[..., 1] * d[..., 1]).astype(F)).astype(F) + (d[..., 2] * d[..., 2]).astype(F)


def ball_query(xyz, new_xyz, radius, nsample, inclusive):
    """xyz [B,N,3], new_xyz [B,S,3] -> (idx int32 [B,S,nsample], cnt int32 [B,S]): the lowest nsample indices with d2 < r2 (d2 <= r2 when
    inclusive) in ascending order, the rest of the row the first hit, zeros without a hit; r2 = fl32(fl32(radius) * fl32(radius))"""
    xyz, new_xyz = np.asarray(xyz, F), np.asarray(new_xyz, F)
    B, S = new_xyz.shape[:2]
    r2 = F(F(radius) * F(radius))
    idx = np.zeros((B, S, nsample), np.int32)
    cnt = np.zeros((B, S), np.int32)
    for b in range(B):
        d2 = sqdist(new_xyz[b], xyz[b])
        hit = d2 <= r2 if inclusive else d2 < r2
        for s in range(S):
            h = np.flatnonzero(hit[s])[:nsample]
            cnt[b, s] = len(h)
            if len(h):
                idx[b, s, :len(h)] = h
                idx[b, s, len(h):] = h[0]
    return idx, cnt


def group_rows(xyz, new_xyz, feat, idx, use_xyz=True):
    """-> rows [B*S*ns, (3 if use_xyz) + D]: xyz[b, i] - new_xyz[b, s] | feat[b, i]"""
    B, S, ns = idx.shape
    parts = []
    bi = np.arange(B)[:, None, None]
    if use_xyz:
        parts.append((np.asarray(xyz, F)[bi, idx] - np.asarray(new_xyz, F)[:, :, None, :]).astype(F))
    if feat is not None:
        parts.append(np.asarray(feat, F)[bi, idx])
    return np.concatenate(parts, axis=-1).reshape(B * S * ns, -1)


def group_rows_bwd(drows, idx, N, D, use_xyz=True, dtype=F):
    """adjoint of group_rows in ``feat``: dfeat [B,N,D], every point summing its rows in ascending (s, j) order in ``dtype``"""
    B, S, ns = idx.shape
    X = 3 if use_xyz else 0
    g = np.asarray(drows).reshape(B, S * ns, X + D)[:, :, X:].astype(dtype)
    out = np.zeros((B, N, D), dtype)
    for b in range(B):
        flat = idx[b].reshape(-1)
        for e in range(S * ns):                                         # ascending e: the kernel's order
            out[b, flat[e]] = (out[b, flat[e]] + g[b, e]).astype(dtype)
    return out


def grouping_operation(features, idx):
    """features [B,C,N], idx [B,S,ns] -> [B,C,S,ns]"""
    B = features.shape[0]
    return np.stack([features[b][:, idx[b]] for b in range(B)])


def lattice_cloud(rs, B, N, lo=-2.0, hi=2.0):
    """coordinates that are multiples of 1/8 in [lo, hi]: every squared distance is exact in float32, in the expanded and the difference form"""
    return (rs.randint(int(lo * 8), int(hi * 8) + 1, size=(B, N, 3)) / 8.0).astype(F)
