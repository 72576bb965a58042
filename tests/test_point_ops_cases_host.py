"""The inputs of tests/test_gpu_point_ops_edges.py TIE where act_amd/csrc/point_ops.hip can go wrong -- proven here on the numpy oracle alone, so
that a passing device test means the tie-breaking code ran, not that the inputs happened to avoid it.  Conditions on the inputs, no GPU."""
import ctypes

import numpy as np
import pytest

from oracle import point_ops as OP
from tests import point_ops_cases as PC

HALF = 0.5                                                           # the bar of every condition: at least half of the queries / steps
KNN_TIED = [c for c in PC.KNN_CASES if c[0] >= 63]
KNN_NONMONOTONE = [c for c in PC.KNN_CASES if PC.knn_interleaved(*c) and c[0] >= 390]
KNN_CUT = [c for c in PC.KNN_CASES if c[1] < c[0]]
FPS_MULTIWAVE = [c for c in PC.FPS_CASES if PC.fps_waves(c[0]) > 1]


def _winner_pairs(N, K, kind):
    """consecutive winners (j, j + 1) of every query: equal distance?, lanes of both, indices of both"""
    _, _, d, i = PC.knn_case(N, K, kind)
    lane = PC.knn_lane(i, N, K)
    return d[..., :-1] == d[..., 1:], lane[..., :-1], lane[..., 1:], i[..., :-1], i[..., 1:]


def test_lane_and_wave_maps():
    """the maps restate the kernels' layouts: spot values, and every lane / wave holds no more points than its registers"""
    assert PC.knn_ppl(64, 8) == 1 and PC.knn_ppl(65, 8) == 2 and PC.knn_ppl(256, 64) == 4 and PC.knn_ppl(257, 9) == 8
    assert PC.knn_ppl(8192, 64) == 128 and PC.knn_ppl(8193, 8) is None and PC.knn_ppl(130, 65) is None
    assert PC.knn_lane([0, 3, 4, 255, 256, 259, 260, 511], 511, 32).tolist() == [0, 0, 1, 63, 0, 0, 1, 63]
    assert PC.knn_lane([0, 1, 2, 126], 127, 16).tolist() == [0, 0, 1, 63]
    assert PC.knn_lane([0, 128, 129, 8192], 8193, 8).tolist() == [0, 0, 1, 63]            # ceil(8193 / 64) = 129 per lane
    for N, K in PC.KNN_CASES:
        ppl = PC.knn_ppl(N, K) or (N + 63) // 64
        count = np.bincount(PC.knn_lane(np.arange(N), N, K), minlength=64)
        assert len(count) == 64 and count.max() <= ppl
    assert PC.fps_wave([0, 255, 256, 999], 1000).tolist() == [0, 0, 1, 3]
    assert PC.fps_wave([0, 1023, 1024, 16382], 16383).tolist() == [0, 0, 1, 15]
    assert PC.fps_wave([0, 1087, 1088, 16389], 16390).tolist() == [0, 0, 1, 15]           # ceil(16390 / 1024) = 17 per thread
    for N, _ in PC.FPS_CASES:
        w = PC.fps_wave(np.arange(N), N)
        assert w.max() < PC.fps_waves(N) and (w.max() > 0) == (N > 256) and (np.diff(w) >= 0).all()


@pytest.mark.parametrize("kind", PC.KNN_KINDS)
@pytest.mark.parametrize("N,K", KNN_TIED)
def test_knn_inputs_tie_across_lanes(N, K, kind):
    eq, la, lb, _, _ = _winner_pairs(N, K, kind)
    frac = (eq & (la != lb)).any(-1).mean()
    print(f"cross-lane ties N={N} K={K} {kind}: {frac:.2f} of the queries")
    assert frac >= HALF


@pytest.mark.parametrize("kind", PC.KNN_KINDS)
@pytest.mark.parametrize("N,K", KNN_NONMONOTONE)
def test_knn_inputs_tie_with_the_lower_index_in_the_higher_lane(N, K, kind):
    """the pair the second wave reduction exists for: both lanes hold the round's minimum, and the lowest lane does not hold the lowest index"""
    eq, la, lb, ia, ib = _winner_pairs(N, K, kind)
    assert (ia[eq] < ib[eq]).all()                                   # the oracle's order inside a tie
    frac = (eq & (la > lb)).any(-1).mean()
    print(f"non-monotone ties N={N} K={K} {kind}: {frac:.2f} of the queries")
    assert frac >= HALF


@pytest.mark.parametrize("kind", PC.KNN_KINDS)
@pytest.mark.parametrize("N,K", KNN_CUT)
def test_knn_cut_falls_inside_a_tie(N, K, kind):
    pts, q, _, _ = PC.knn_case(N, K, kind)
    d = np.sort(OP._sqdist(q[:, :, None, :], pts[:, None, :, :]), axis=-1)
    frac = (d[..., K - 1] == d[..., K]).mean()
    print(f"boundary ties N={N} K={K} {kind}: {frac:.2f} of the queries")
    assert frac >= HALF


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("N,G", FPS_MULTIWAVE)
def test_fps_inputs_tie_across_waves(N, G, skip):
    """replay the oracle's chain: at each step, is the maximum running distance attained in two different waves?"""
    pts, idx = PC.fps_case(N, G, skip)
    for b in range(PC.FPS_B):
        p = pts[b]
        live = OP._sqdist(p, np.zeros(3, np.float32)) > np.float32(1e-3) if skip else np.ones(N, bool)
        temp = np.where(live, np.float32(1e10), np.float32(-1.0))
        tied = 0
        for j in range(1, G):
            temp = np.where(live, np.minimum(temp, OP._sqdist(p, p[idx[b, j - 1]][None, :])), temp)
            top = np.flatnonzero(temp == temp.max())
            assert top[0] == idx[b, j]                               # the replay follows the oracle
            tied += len(set(PC.fps_wave(top, N).tolist())) > 1
        print(f"cross-wave ties N={N} G={G} skip={skip} cloud {b}: {tied} of {G - 1} steps")
        assert tied >= HALF * (G - 1)


def test_fps_dead_points_are_where_the_cases_say():
    for N, _ in PC.FPS_CASES + [PC.FPS_OVERSAMPLE]:
        pts = PC.fps_cloud(N)
        dead = (pts == 0).all(-1)
        assert dead[1, 0] and not dead[0, 0] and dead[0].any()       # cloud 1 starts on a dead point, cloud 0 on a live one and has a dead one
        assert np.array_equal(dead, (pts.astype(np.float64) ** 2).sum(-1) <= 1e-3)        # and nothing else is within the ball
    N, G = PC.FPS_OVERSAMPLE
    _, idx = PC.fps_case(N, G, True)
    dead = (PC.fps_cloud(N) == 0).all(-1)
    assert dead[0].any() and not dead[0, 0]                          # cloud 0: some dead points, a live start
    pts = PC.fps_cloud(N)
    for b in range(PC.FPS_B):
        assert not dead[b, idx[b, 1:]].any()                         # never a dead point after the start ...
        sites = lambda k: set(map(tuple, pts[b, k].tolist()))
        assert sites(idx[b, 1:]) == sites(np.flatnonzero(~dead[b]))  # ... every live site (a duplicate of a picked point stays at distance 0) ...
        assert (idx[b, N:] == np.flatnonzero(~dead[b])[0]).all()     # ... and then the lowest live index for ever


P = lambda a: a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("kind", PC.KNN_KINDS)
def test_c_oracle_agrees_on_knn(oracle_c, kind):
    for N, K in PC.KNN_CASES:
        pts, q, d, i = PC.knn_case(N, K, kind)
        ci = np.empty((PC.KNN_B, PC.KNN_Q, K), np.int64); cd = np.empty((PC.KNN_B, PC.KNN_Q, K), np.float32)
        assert oracle_c.oracle_knn_f32(P(pts), P(q), PC.KNN_B, N, PC.KNN_Q, K, P(ci), P(cd)) == 0
        assert np.array_equal(ci, i) and np.array_equal(cd, d), (N, K)


def test_c_oracle_agrees_on_fps(oracle_c):
    for skip in (False, True):
        for N, G in PC.FPS_CASES + [PC.FPS_OVERSAMPLE]:
            pts, idx = PC.fps_case(N, G, skip)
            ci = np.empty((PC.FPS_B, G), np.int32)
            assert oracle_c.oracle_fps_f32(P(pts), PC.FPS_B, N, G, P(ci), int(skip)) == 0
            assert np.array_equal(ci, idx), (N, G, skip)
    for N, G in PC.FPS_CROWDED:
        pts, idx = PC.fps_crowded_case(N, G)
        ci = np.empty((1, G), np.int32)
        assert oracle_c.oracle_fps_f32(P(pts), 1, N, G, P(ci), 0) == 0
        assert np.array_equal(ci, idx), (N, G)
        if G == N:
            assert sorted(idx[0].tolist()) == list(range(N))        # a Gaussian cloud has no duplicates: G = N visits every point
