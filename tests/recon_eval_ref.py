"""Independent statement of the Stage-I reconstruction metrics (helper of test_recon_eval_host.py / test_gpu_recon_eval.py).

Brute-force float64 numpy, written from the reference's definitions -- utils/metrics.py:57-95 (F-Score through nearest-neighbour distances,
CDL1 / CDL2 through ChamferDistanceL1 / L2(ignore_zeros=True) at batch size 1) and extensions/chamfer_dist/__init__.py:28-84
(L2 = mean d1 + mean d2 over squared distances, L1 = (mean sqrt d1 + mean sqrt d2) / 2, zero points = rows whose fp32 sum is 0, removed from
both clouds) -- not from the kernel.  Inputs are float32 arrays, promoted exactly."""
import numpy as np

SIGMAS = (0.002, 0.004, 0.006, 0.01)
BORDER_REL = 1e-5           # a query is borderline when its float64 nearest-neighbour distance is within this relative band of th


def pc_norm(pc):
    pc = pc - pc.mean(axis=0)
    return pc / np.max(np.sqrt((pc ** 2).sum(axis=1)))


def make_clouds(seed=0, B=64, N=1024, nc=512):
    """clouds for which every metric is informative: gt = pc_norm of N gaussian points, dense = every gt point twice plus gaussian noise of
    sigma 0.002 / 0.004 / 0.006 / 0.01 by cloud, coarse = an nc-subset plus the same noise"""
    rs = np.random.RandomState(seed)
    gt = np.stack([pc_norm(rs.standard_normal((N, 3))) for _ in range(B)]).astype(np.float32)
    dense = np.empty((B, 2 * N, 3), np.float32)
    coarse = np.empty((B, nc, 3), np.float32)
    for b in range(B):
        s = SIGMAS[b % len(SIGMAS)]
        dense[b] = np.concatenate([gt[b], gt[b]]) + s * rs.standard_normal((2 * N, 3))
        coarse[b] = gt[b][rs.permutation(N)[:nc]] + s * rs.standard_normal((nc, 3))
    return coarse, dense, gt


def nn_sq(a, b, chunk=256):
    """squared distance of every row of a to its nearest row of b, float64 brute force"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty(a.shape[0], np.float64)
    for i in range(0, a.shape[0], chunk):
        d = a[i:i + chunk, None, :] - b[None, :, :]
        out[i:i + chunk] = (d * d).sum(-1).min(axis=1)
    return out


def nonzero_mask(x):
    """torch.sum(xyz, dim=2).ne(0) for float32 points: (x + y) + z in fp32"""
    x = np.asarray(x, np.float32)
    return ((x[:, 0] + x[:, 1]) + x[:, 2]) != 0


def chamfer(a, b):
    """(L1, L2) of one pair of clouds; NaN when either is empty (torch.mean of an empty tensor)"""
    if a.shape[0] == 0 or b.shape[0] == 0:
        return float("nan"), float("nan")
    d1, d2 = nn_sq(a, b), nn_sq(b, a)
    return (np.sqrt(d1).mean() + np.sqrt(d2).mean()) / 2, d1.mean() + d2.mean()


def ref_row(coarse, dense, gt, th=0.01):
    """one cloud -> dict of the reference's values (unscaled) and the borderline counts of the two threshold decisions"""
    r = {}
    r["sparse_l1"], r["sparse_l2"] = chamfer(coarse, gt)
    r["dense_l1"], r["dense_l2"] = chamfer(dense, gt)
    r["cdl1"], r["cdl2"] = chamfer(dense[nonzero_mask(dense)], gt[nonzero_mask(gt)])
    dp, dr = np.sqrt(nn_sq(dense, gt)), np.sqrt(nn_sq(gt, dense))        # compute_point_cloud_distance: pred -> gt, gt -> pred
    r["hits_p"], r["hits_r"] = int((dp < th).sum()), int((dr < th).sum())
    r["border_p"] = int((np.abs(dp - th) <= BORDER_REL * th).sum())
    r["border_r"] = int((np.abs(dr - th) <= BORDER_REL * th).sum())
    p, q = r["hits_p"] / dense.shape[0], r["hits_r"] / gt.shape[0]
    r["fscore"] = 2 * q * p / (q + p) if q + p else 0.0
    return r


CHAMFER_KEYS = ("sparse_l1", "sparse_l2", "dense_l1", "dense_l2", "cdl1", "cdl2")      # the kernel's fields 0..5 in order


def fscore_from_counts(hp, hr, nd, N):
    p, r = hp / nd, hr / N
    return 2 * r * p / (r + p) if r + p else 0.0
