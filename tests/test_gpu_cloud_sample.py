"""GPU: csrc/cloud_sample.hip (K.cloud_sample) against its numpy restatement (tests/cloud_sample_ref.py) and numpy's pc_norm, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cloud_sample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NS = [1, 2, 7, 257, 1024, 1200, 8192]


def _i32(a):
    return torch.tensor(list(a), dtype=torch.int32, device=DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _pc_norm(pc):
    from act_amd.datasets.SyntheticDataset import pc_norm
    with np.errstate(invalid="ignore", divide="ignore"):
        return pc_norm(pc)


def _clouds(M, N, C, offset, seed):
    g = np.random.default_rng(seed)
    c = (g.standard_normal((M, N, C)) * ([1.0, 0.5, 2.0, 1.0, 1.0, 1.0][:C])).astype(np.float32)
    c[:, :, :3] += np.float32(offset)
    return c


# ---- selection ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 5, 64, 100, 1000, 8192])
def test_src_rows_equal_the_restatement(N):
    import act_amd.kernels as K
    clouds = torch.zeros(2, N, 3, device=DEV)
    items, draws = [1, 0, 1, 0], [0, 5, 9, 123456]
    for n in sorted({1, N, -(-N // 4)}):
        out, rows = K.cloud_sample(clouds, _i32(items), _i32(draws), n, 11, 3, permute=True, normalize=False, want_rows=True)
        rows = rows.cpu().numpy()
        assert rows.shape == (4, n) and rows.dtype == np.int32 and tuple(out.shape) == (4, n, 3)
        for b, d in enumerate(draws):
            assert np.array_equal(rows[b], R.subset_rows(N, n, 11, 3, d)), (N, n, d)
        _, plain = K.cloud_sample(clouds, _i32(items), _i32(draws), n, 11, 3, permute=False, normalize=False, want_rows=True)
        assert np.array_equal(plain.cpu().numpy(), np.tile(np.arange(n), (4, 1)))


# ---- gather --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 6])
def test_plain_gather_is_the_source_rows(C):
    import act_amd.kernels as K
    clouds = _clouds(3, 100, C, 0.0, C)
    items, draws = [2, 0, 2, 1, 0], [4, 3, 2, 1, 0]                          # out of order, repeated
    for n in (100, 25):
        out, rows = K.cloud_sample(torch.from_numpy(clouds).to(DEV), _i32(items), _i32(draws), n, 0, 0, permute=True, normalize=False,
                                   want_rows=True)
        out, rows = out.cpu().numpy(), rows.cpu().numpy()
        for b, it in enumerate(items):
            assert np.array_equal(rows[b], R.subset_rows(100, n, 0, 0, draws[b]))
            assert np.array_equal(_bits(out[b]), _bits(clouds[it, rows[b]]))
    alone = K.cloud_sample(torch.from_numpy(clouds).to(DEV), _i32(items), _i32(draws), 25, 0, 0, permute=True, normalize=False)
    assert torch.is_tensor(alone) and np.array_equal(_bits(alone.cpu().numpy()), _bits(out))      # want_rows off: the points alone


# ---- normalisation -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """clouds [2, 8192, C] for C = 3 and 6, around the origin and offset by 1000, resident once"""
    return {(C, off): _clouds(2, 8192, C, off, 17 + C) for C in (3, 6) for off in (0.0, 1000.0)}


@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("C", [3, 6])
def test_normalised_output_is_numpys_pc_norm(big, C, offset):
    import act_amd.kernels as K
    clouds = big[(C, offset)]
    dev = torch.from_numpy(clouds).to(DEV)
    items, draws = [1, 0, 1], [7, 8, 9]
    for n in NS:
        for permute in (True, False):
            out, rows = K.cloud_sample(dev, _i32(items), _i32(draws), n, 2, 5, permute=permute, normalize=True, want_rows=True)
            out, rows = out.cpu().numpy(), rows.cpu().numpy()
            for b, it in enumerate(items):
                src = clouds[it, rows[b]]
                assert np.array_equal(_bits(out[b, :, 0:3]), _bits(_pc_norm(src[:, 0:3]))), (n, permute, b)
                if C == 6:
                    assert np.array_equal(_bits(out[b, :, 3:6]), _bits(src[:, 3:6]))             # the normals come through untouched
            if n == 257 and permute:                                                              # and the whole item is the restatement's
                want, wrows = R.sample(clouds, 1, 7, n, 2, 5)
                assert np.array_equal(rows[0], wrows) and np.array_equal(_bits(out[0]), _bits(want))


def test_degenerate_clouds_give_numpys_nans():
    import act_amd.kernels as K
    one = _clouds(2, 64, 3, 3.0, 1)
    out = K.cloud_sample(torch.from_numpy(one).to(DEV), _i32([0, 1]), _i32([0, 1]), 1, 0, 0).cpu().numpy()
    assert np.isnan(out).all() and np.isnan(_pc_norm(one[0, :1])).all()                          # one point: 0 / 0
    same = np.broadcast_to(np.array([0.25, -1.5, 3.0], np.float32), (1, 32, 3)).copy()             # all points equal: the mean is exact
    want = _pc_norm(same[0])
    got = K.cloud_sample(torch.from_numpy(same).to(DEV), _i32([0]), _i32([0]), 32, 0, 0).cpu().numpy()[0]
    assert np.isnan(want).all() and np.array_equal(np.isnan(got), np.isnan(want))
    near = np.broadcast_to(np.array([0.1, 0.2, 0.3], np.float32), (1, 33, 3)).copy()               # all equal, the mean rounds: numpy decides
    want = _pc_norm(near[0])
    got = K.cloud_sample(torch.from_numpy(near).to(DEV), _i32([0]), _i32([0]), 33, 0, 0, permute=False).cpu().numpy()[0]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(_bits(got)[~np.isnan(want)], _bits(want)[~np.isnan(want)])


# ---- batches, determinism, frequencies -----------------------------------------------------------------------------------------------------------
def test_batch_independence_and_determinism():
    import act_amd.kernels as K
    clouds = torch.from_numpy(_clouds(5, 300, 6, 10.0, 3)).to(DEV)
    items = _i32(np.arange(48) % 5)
    draws = _i32(np.arange(48) * 3 + 1)
    whole, wrows = K.cloud_sample(clouds, items, draws, 75, 9, 4, want_rows=True)
    again, arows = K.cloud_sample(clouds, items, draws, 75, 9, 4, want_rows=True)
    assert torch.equal(whole.view(torch.int32), again.view(torch.int32)) and torch.equal(wrows, arows)            # two runs: the same bits
    parts = [K.cloud_sample(clouds, items[s:s + 8], draws[s:s + 8], 75, 9, 4, want_rows=True) for s in range(0, 48, 8)]
    assert torch.equal(torch.cat([p[0] for p in parts]).view(torch.int32), whole.view(torch.int32))               # one batch of 48 = six of 8
    assert torch.equal(torch.cat([p[1] for p in parts]), wrows)
    for seed, epoch in ((9, 5), (10, 4)):
        _, other = K.cloud_sample(clouds, items, draws, 75, seed, epoch, want_rows=True)
        assert not torch.equal(other, wrows) and bool((other != wrows).any(dim=1).all())                            # every item draws anew


def test_selection_frequencies_on_the_device():
    """the band of tests/test_cloud_loader_host.py (mean 1,024 +- 6 binomial standard deviations of 27.7), from the device's src_rows"""
    import act_amd.kernels as K
    clouds = torch.zeros(1, 64, 3, device=DEV)
    ids = torch.arange(4096, dtype=torch.int32, device=DEV)
    _, rows = K.cloud_sample(clouds, torch.zeros_like(ids), ids, 16, 0, 0, permute=True, normalize=False, want_rows=True)
    counts = torch.bincount(rows.reshape(-1).long(), minlength=64).cpu().numpy()
    print("selection counts: min %d max %d" % (counts.min(), counts.max()))
    assert counts.sum() == 4096 * 16 and counts.min() >= 858 and counts.max() <= 1190


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import act_amd.kernels as K
    import act_amd._C as C
    clouds = torch.zeros(3, 16, 3, device=DEV)
    ids = _i32([0, 1])
    ok = dict(clouds=clouds, item_ids=ids, draw_ids=ids, n=8, seed=0, epoch=0)
    K.cloud_sample(**ok)
    bad = [dict(n=17), dict(n=0), dict(n=-1), dict(clouds=torch.zeros(3, 16, 4, device=DEV)), dict(clouds=torch.zeros(3, 16, 2, device=DEV)),
           dict(clouds=torch.zeros(3, 9000, 3, device=DEV), n=8193), dict(item_ids=_i32([]), draw_ids=_i32([])),
           dict(clouds=clouds.double()), dict(clouds=clouds.cpu()), dict(clouds=torch.zeros(16, 3, device=DEV)),
           dict(item_ids=ids.long()), dict(draw_ids=ids.long()), dict(item_ids=ids.cpu()), dict(draw_ids=ids.cpu()), dict(draw_ids=_i32([0])),
           dict(item_ids=_i32([0, 3])), dict(item_ids=_i32([-1, 0]))]
    for kw in bad:
        with pytest.raises(ValueError):
            K.cloud_sample(**dict(ok, **kw))
    assert K.cloud_sample(**dict(ok, clouds=torch.zeros(3, 9000, 3, device=DEV), n=8192)).shape == (2, 8192, 3)
    # the C entry point: the error code, nothing launched
    assert C.lib.act_cloud_sample_max_points() == 8192
    out = torch.full((2, 8, 3), 7.0, device=DEV)

    def call(M=3, N=16, Cc=3, B=2, n=8, flags=3, o=out):
        return C.lib.act_cloud_sample_f32(C.ptr(clouds), M, N, Cc, C.ptr(ids), C.ptr(ids), B, n, 0, 0, flags, C.ptr(o), None, C.stream())
    assert call(n=17) == -1 and call(n=0) == -1 and call(N=9000, n=8193) == -1 and call(Cc=4) == -1 and call(B=0) == -1 and call(flags=4) == -1
    assert call(o=None) == -2
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # without validate an item id outside [0, M) reads nothing: NaN points, rows -1
    o2, rows = K.cloud_sample(clouds, _i32([0, 3]), ids, 8, 0, 0, want_rows=True, validate=False)
    assert bool(torch.isnan(o2[1]).all()) and bool((rows[1] == -1).all()) and bool((rows[0] >= 0).all())
