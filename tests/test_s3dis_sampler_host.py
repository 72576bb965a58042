"""CPU: the grid index of the device S3DIS block sampler built on CPU tensors, the numpy restatement of the sampler (tests/s3dis_sample_ref.py)
against S3DISDataset.sample_block's np.where, the two selection rules, and the epoch iterator's plan."""
import numpy as np
import pytest
import torch

from act_amd.datasets import DeviceS3DISBlocks
from act_amd.datasets.S3DISDataset import sample_block, SyntheticS3DIS
from tests import s3dis_sample_ref as R


@pytest.fixture(scope="module")
def rooms():
    e = R.room_e()
    return {"a": R.room_a(), "b": R.room_b(), "c": R.room_c(), "d": R.room_d(), "e": e, "e32": (e[0].astype(np.float32), e[1])}


@pytest.fixture(scope="module")
def built(rooms):
    names = list(rooms)
    blocks = DeviceS3DISBlocks([rooms[n][0] for n in names], [rooms[n][1] for n in names], 2048, device="cpu")
    return names, blocks, R.RefSampler([rooms[n] for n in names], 2048)


def _room_csr(ix, r):
    gx, gy, base = (int(v) for v in ix.grid_dims[r])
    off = ix.cell_off[base:base + gx * gy + 1].numpy()
    a = int(ix.room_off[r])
    return gx, gy, off - a, ix.cell_pts[a:int(ix.room_off[r + 1])].numpy()


def test_index_puts_every_point_in_exactly_one_cell_in_ascending_order(built):
    names, blocks, ref = built
    ix = blocks.index
    assert ix.xyz.dtype == torch.float64 and ix.labels.dtype == torch.int32 and ix.room_off.dtype == torch.int64
    assert ix.cell_off.dtype == torch.int64 and ix.cell_pts.dtype == torch.int32 and ix.cell == 0.25
    for r, name in enumerate(names):
        gx, gy, off, pts = _room_csr(ix, r)
        P = ref.pts[r].shape[0]
        assert (gx, gy) == tuple(ref.dims[r]) and off[0] == 0 and off[-1] == P and np.all(np.diff(off) >= 0), name
        assert np.array_equal(np.sort(pts), np.arange(P)), name                                   # every point once
        cell = np.repeat(np.arange(gx * gy), np.diff(off))
        assert np.array_equal(ref.cells(r)[pts], cell), name                                      # ... in the cell the cell function names
        same = cell[1:] == cell[:-1]
        assert np.all(np.diff(pts.astype(np.int64))[same] > 0), name                              # ascending inside every cell
    assert ix.grid_dims[names.index("d"), :2].tolist() == [1, 1]                                  # room D: one cell


def test_overlapped_cells_contain_np_where(built):
    names, blocks, ref = built
    ix = blocks.index
    rng = np.random.default_rng(0)
    for r, name in enumerate(names):
        gx, gy, off, pts = _room_csr(ix, r)
        p = ref.pts[r]
        most = 0
        for ci in rng.integers(0, p.shape[0], 500):
            ix0, ix1, iy0, iy1 = ref.window(r, ci)
            assert ix1 - ix0 <= 5 and iy1 - iy0 <= 5
            cand = np.concatenate([pts[off[iy * gx + ix0]:off[iy * gx + ix1 + 1]] for iy in range(iy0, iy1 + 1)])
            cx, cy = p[ci, 0], p[ci, 1]
            want = np.where((p[:, 0] >= cx - 0.5) & (p[:, 0] <= cx + 0.5) & (p[:, 1] >= cy - 0.5) & (p[:, 1] <= cy + 0.5))[0]
            assert np.isin(want, cand).all(), (name, ci)
            # the candidates that pass the test, in candidate order, are the restatement's member list
            m = cand[np.isin(cand, want)]
            assert np.array_equal(m, ref.members(r, ci)), (name, ci)
            most = max(most, cand.size)
        assert most <= ix.max_window, name
    assert ix.max_window <= max(q.shape[0] for q in ref.pts)


class _InjectedRng:
    """sample_block's two draws: the centre is injected, the selection records np.where's index set"""

    def __init__(self, ci):
        self.ci, self.idx = ci, None

    def choice(self, a, size=None, replace=True):
        if size is None:
            assert self.idx is None, "column rejected: the test picked a centre with too few points"
            return self.ci
        self.idx = np.array(a)
        return self.idx[np.arange(size) % self.idx.size]


@pytest.mark.parametrize("name", ["a", "b", "e", "e32"])
def test_restatement_members_equal_sample_block(rooms, name):
    pts, lab = rooms[name]
    ref = R.RefSampler([rooms[name]], 256)
    done = 0
    for ci in np.random.default_rng(1).integers(0, pts.shape[0], 60):
        mem = ref.members(0, ci)
        if mem.size <= 1024:
            continue
        rng = _InjectedRng(int(ci))
        xyz, _ = sample_block(pts, lab, 256, 1.0, rng)                                           # (in the room's own dtype)
        assert np.array_equal(np.sort(mem), rng.idx), (name, ci)
        sel = rng.idx[np.arange(256)]
        want = np.stack([(ref.pts[0][sel, 0] - ref.pts[0][ci, 0]).astype(np.float32), (ref.pts[0][sel, 1] - ref.pts[0][ci, 1]).astype(np.float32),
                         ref.pts[0][sel, 2].astype(np.float32)], axis=1)
        assert np.array_equal(xyz, want), (name, ci)                                             # float64 difference rounded once == the file dtype's
        done += 1
    assert done >= 20


def test_selection_rules():
    ref = R.RefSampler([R.room_d()], 2048)
    for k0 in (0, 1, 0xdeadbeef):
        for count in (2048, 2049, 2312, 4096, 5000):
            s = ref.select(k0, count)
            assert s.shape == (2048,) and s.min() >= 0 and s.max() < count and np.unique(s).size == 2048
        assert np.array_equal(np.sort(ref.select(k0, 2048)), np.arange(2048))                    # count == num_point: a permutation
        for count in (1, 2, 648, 2047):
            s = ref.select(k0, count)
            assert s.shape == (2048,) and s.min() >= 0 and s.max() < count
    assert not np.array_equal(ref.select(0, 2312), ref.select(1, 2312))


def test_centre_draw_is_in_range_and_spread():
    for P in (1, 2, 12936, (1 << 27) + 12345):
        c = np.array([R.center_draw(R.item_key(3, 1, i), t, P) for i in range(200) for t in range(4)])
        assert c.min() >= 0 and c.max() < P
        if P > 1000:
            assert np.unique(c).size > 700 and abs(c.mean() / P - 0.5) < 0.05


def test_restatement_accepts_and_falls_back():
    ref = R.RefSampler([R.room_b(), R.room_c()], 64, max_tries=8)
    outs = [ref.item(0, i, 0, 0) for i in range(64)]
    assert any(o["info"] > 1 for o in outs)
    for o in outs:
        assert o["info"] == len(o["counts"]) and o["count"] > 1024 and all(c <= 1024 for c in o["counts"][:-1])
    o = ref.item(1, 5, 0, 0)
    assert o["info"] == -8 and len(o["counts"]) == 8 and o["count"] == max(o["counts"])
    assert o["center_idx"] == R.center_draw(R.item_key(0, 0, 5), o["counts"].index(max(o["counts"])), 600)


@pytest.mark.parametrize("drop_last", [True, False])
def test_epoch_plan_covers_every_item_once(drop_last):
    ds = SyntheticS3DIS("train", 2048, num_rooms=2, points_per_room=4000)
    blocks = DeviceS3DISBlocks.from_dataset(ds, device="cpu")
    assert np.array_equal(blocks.room_idxs, ds.room_idxs) and blocks.labelweights is ds.labelweights and len(blocks) == len(ds)
    seen = []

    def fake(room_ids, item_ids, seed, epoch, center_idx=None, validate=True):
        seen.append((room_ids.numpy().copy(), item_ids.numpy().copy(), seed, epoch))
        return R_SAMPLE(room_ids, item_ids)
    from act_amd.datasets.S3DISDevice import S3DISSample

    def R_SAMPLE(r, i):
        return S3DISSample(r, i, None, None, None, None)
    blocks.sample = fake
    n, B = len(ds), 3
    assert n % B != 0                                                                             # a last partial batch exists
    got = list(blocks.epoch(B, 4, 9, drop_last=drop_last))
    assert len(got) == (n // B if drop_last else n // B + 1) and len(seen) == len(got)
    items = np.concatenate([s[1] for s in seen])
    assert np.array_equal(items, np.arange(n if not drop_last else n // B * B))                   # every item id once, ids = positions
    assert all(s[0].size == B for s in seen[:n // B]) and (drop_last or seen[-1][0].size == n % B)
    order = np.random.default_rng((9, 4)).permutation(n)
    assert np.array_equal(np.concatenate([s[0] for s in seen]), ds.room_idxs[order][:items.size])
    assert all(s[2:] == (9, 4) for s in seen)
    seen.clear()
    list(blocks.epoch(B, 0, 9, shuffle=False, drop_last=drop_last))
    assert np.array_equal(np.concatenate([s[0] for s in seen]), ds.room_idxs[:items.size])


def test_construction_refuses_non_finite_coordinates():
    p, l = R.room_c()
    for bad in (np.nan, np.inf):
        q = p.copy()
        q[17, 1] = bad
        with pytest.raises(ValueError):
            DeviceS3DISBlocks([q], [l], 64, device="cpu")
    with pytest.raises(ValueError):
        DeviceS3DISBlocks([p], [l], 0, device="cpu")
