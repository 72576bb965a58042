"""Inputs that TIE for the grouping front end (act_amd/csrc/point_ops.hip): lattice clouds, the case tables of the FPS / kNN-group edge tests and
the maps from a point index to the lane / wave that holds it in each dispatch row of act_knn_group_f32 / act_fps_f32.
Test infrastructure only, no GPU: tests/test_point_ops_cases_host.py proves on the numpy oracle that these inputs tie where the kernels can go
wrong; tests/test_gpu_point_ops_edges.py and its child processes run the same tables on the device."""
import functools

import numpy as np

from oracle import point_ops as OP

F = np.float32

# ------------------------------------------------------------------------------------------------ case tables
KNN_B, KNN_Q = 2, 13                   # 26 queries: not a multiple of the 4 waves of a workgroup; cloud 1 starts 12 * N bytes in (4-byte aligned for odd N)
KNN_CASES = [
    (63, 63),                          # K = N at 1 point per lane
    (127, 16),                         # 2 points per lane
    (254, 32),                         # 4 points per lane
    (257, 9),                          # first N of 8 per lane: point 256 is alone in register row 1
    (390, 32),                         # 8 per lane
    (511, 32),                         # 8 per lane, N % 4 = 3
    (1022, 32),                        # 16 per lane, N % 4 = 2
    (2047, 32),                        # 32 per lane
    (2049, 64),                        # 64 per lane
    (4095, 64),                        # 64 per lane, K at the one-winner-per-lane limit
    (4097, 64),                        # 128 per lane
    (8190, 64),                        # 128 per lane
    (8193, 8),                         # rescan kernel by N
    (130, 65),                         # rescan kernel by K
    (130, 64),                         # register kernel: must give the first 64 columns of the K = 65 run
    (1, 1), (2, 2),                    # all points identical
]
KNN_KINDS = ("member", "offset")
KNN_SEEDS = {130: 1131}                # N -> seed where RandomState(N) leaves a condition of the host test short (130: the K = 64 cut, 0.46 of the queries)

FPS_B = 2
FPS_CASES = [
    (200, 24),                         # <1 wave, 4 points per lane>
    (1000, 24),                        # <4, 4>
    (2047, 24),                        # <4, 8>
    (4001, 40),                        # <8, 8>: candidates reduced by DPP
    (8190, 40),                        # <16, 8>
    (10922, 40),                       # <16, 16>, last N whose cloud fits the LDS
    (10923, 40),                       # <16, 16>, first N read from global memory
    (16383, 40),                       # <16, 16>
    (16390, 24),                       # fps_big_kernel
]
FPS_OVERSAMPLE = (70, 80)              # G > N with dead points (skip_near_origin on)
# one cloud each; the G indices crowd the cloud out of the LDS.  Gaussian clouds: on the lattice every running distance is 0 after 729 steps
FPS_CROWDED = [(10922, 8131), (10500, 10500)]
FPS_CFG_N = (300, 1000)                # ACT_FPS_CFG = 1..4 applies to 256 < N <= 1024


# ------------------------------------------------------------------------------------------------ generators
def lattice_cloud(seed, B, N):
    """[B,N,3] float32, coordinates drawn with replacement from {-4..4}/4: 729 sites, so many exact duplicates, and every squared distance
    between two points (or a point and a cell centre, see queries) is a small multiple of 1/64 -- exact in fp32 whatever the order of the sums"""
    return (np.random.RandomState(seed).randint(-4, 5, (B, N, 3)) / 4.0).astype(F)


def queries(kind, pts, Q, seed=0):
    """[B,Q,3] float32.  "member": the first Q points of each cloud (cyclically when N < Q).  "offset": centres of lattice cells, a site of
    {-4..3}/4 shifted by +1/8 on each axis -- equidistant from the 8 corners of its cell"""
    B, N, _ = pts.shape
    if kind == "member":
        return np.ascontiguousarray(pts[:, np.arange(Q) % N])
    if kind == "offset":
        return (np.random.RandomState(seed + 7919).randint(-4, 4, (B, Q, 3)) / 4.0 + 0.125).astype(F)
    raise ValueError(kind)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def knn_case(N, K, kind):
    """-> (pts [B,N,3], query [B,Q,3], dist [B,Q,K], idx int64 [B,Q,K]) with the numpy oracle's answer; computed once, read-only"""
    seed = KNN_SEEDS.get(N, N)
    pts = lattice_cloud(seed, KNN_B, N)
    if N <= 2:
        pts[:, 1:] = pts[:, :1]
    q = queries(kind, pts, KNN_Q, seed)
    d, i = OP.knn_ref(pts, q, K)
    return _frozen(pts, q, d, i)


def fps_cloud(N, B=FPS_B):
    """lattice cloud of the FPS cases.  Dead under skip_near_origin: every point the lattice put at the origin, in cloud 0 also the middle
    point (a small cloud may have drawn none), and in cloud 1 the START point itself"""
    pts = lattice_cloud(N, B, N)
    pts[0, N // 2] = 0.0
    pts[1, 0] = 0.0
    return pts


@functools.lru_cache(maxsize=None)
def fps_case(N, G, skip):
    """-> (pts [B,N,3], idx int32 [B,G]) with the numpy oracle's answer; computed once, read-only"""
    pts = fps_cloud(N)
    return _frozen(pts, OP.fps_ref(pts, G, skip_near_origin=skip))


@functools.lru_cache(maxsize=None)
def fps_crowded_case(N, G):
    from tests.golden.fill import clouds
    pts = clouds(N, 1, N)
    return _frozen(pts, OP.fps_ref(pts, G))


# ------------------------------------------------------------------------------------------------ who holds a point
def knn_ppl(N, K):
    """points per lane of the register kernel act_knn_group_f32 picks, None for the rescan kernel"""
    if K > 64 or N > 8192:
        return None
    return next(p for p in (1, 2, 4, 8, 16, 32, 64, 128) if N <= 64 * p)


def knn_interleaved(N, K):
    return (knn_ppl(N, K) or 0) >= 8


def knn_lane(idx, N, K):
    """the lane that owns point ``idx``: contiguous chunks up to 4 points per lane and in the rescan kernel; from 8 per lane on, register element
    e of lane l is point (e / 4) * 256 + 4 * l + e % 4"""
    idx = np.asarray(idx)
    ppl = knn_ppl(N, K)
    if ppl is None:
        return idx // ((N + 63) // 64)
    if ppl <= 4:
        return idx // ppl
    return (idx % 256) // 4


FPS_ROWS = ((256, 1, 4), (1024, 4, 4), (2048, 4, 8), (4096, 8, 8), (8192, 16, 8), (16384, 16, 16))    # (largest N, waves, points per lane)


def fps_waves(N):
    return next((w for n, w, _ in FPS_ROWS if N <= n), 16)


def fps_wave(idx, N):
    """the wave that owns point ``idx``: a thread holds a contiguous chunk (points-per-lane of its dispatch row; ceil(N / 1024) in fps_big_kernel)"""
    per = next((p for n, _, p in FPS_ROWS if N <= n), (N + 1023) // 1024)
    return np.asarray(idx) // per // 64


# ------------------------------------------------------------------------------------------------ the device side, shared with the child processes
def to_device(a, dev):
    """a (read-only, shared) case array as a device tensor"""
    import torch
    return torch.from_numpy(a.copy()).to(dev)


def check_knn_case(dev, N, K, kind):
    """act_knn_group_f32 through the public wrapper against the numpy oracle, bit for bit: indices, distances, centred neighbourhoods"""
    import torch
    from act_amd.knn_cuda import knn_group
    pts, q, d_ref, i_ref = knn_case(N, K, kind)
    idx, nbr, dist = knn_group(to_device(pts, dev), to_device(q, dev), K, want_nbr=True, want_dist=True)
    torch.cuda.synchronize()
    idx, nbr, dist = idx.cpu().numpy(), nbr.cpu().numpy(), dist.cpu().numpy()
    bad = np.flatnonzero((idx != i_ref).any(-1).ravel())
    assert idx.dtype == np.int64 and bad.size == 0, f"kNN N={N} K={K} {kind}: {bad.size} of {KNN_B * KNN_Q} queries differ, first {bad[:4].tolist()}"
    assert np.array_equal(dist, d_ref), f"kNN N={N} K={K} {kind}: distances differ"
    want = pts[np.arange(KNN_B)[:, None, None], i_ref] - q[:, :, None, :]
    assert np.array_equal(nbr, want), f"kNN N={N} K={K} {kind}: neighbourhoods differ"
