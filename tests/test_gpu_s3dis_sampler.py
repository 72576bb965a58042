"""GPU: S3DIS training blocks sampled on the device from resident rooms (csrc/s3dis_sample.hip, act_amd/datasets/S3DISDevice.py) against np.where
and the numpy restatement of the whole sampler (tests/s3dis_sample_ref.py), bit for bit."""
import copy
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests import s3dis_sample_ref as R

pytestmark = pytest.mark.gpu

NAMES = ["a", "b", "c", "d", "e", "e32"]
A, B_, C, D, E, E32 = range(6)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rooms():
    e = R.room_e()
    return [R.room_a(), R.room_b(), R.room_c(), R.room_d(), e, (e[0].astype(np.float32), e[1])]


@pytest.fixture(scope="module")
def blocks(dev, rooms):
    from act_amd.datasets import DeviceS3DISBlocks
    return DeviceS3DISBlocks([p for p, _ in rooms], [l for _, l in rooms], 2048, device=dev)


def variant(blocks, num_point=None, max_tries=None):
    """the same resident rooms with another num_point / max_tries"""
    v = copy.copy(blocks)
    v.index = copy.copy(blocks.index)
    if num_point is not None:
        v.num_point = num_point
    if max_tries is not None:
        v.max_tries = v.index.max_tries = max_tries
    return v


def i32(dev, a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32, device=dev)


def run(blocks, dev, room_ids, item_ids, seed=0, epoch=0, center_idx=None):
    """-> the outputs as numpy arrays + the member lists the launch left in the workspace"""
    out = blocks.sample(i32(dev, room_ids), i32(dev, item_ids), seed, epoch, None if center_idx is None else i32(dev, center_idx))
    B, mw = len(room_ids), blocks.index.max_window
    ws = blocks._ws[:B * mw].view(B, mw).cpu().numpy()
    o = {k: getattr(out, k).cpu().numpy() for k in out._fields}
    o["members"] = [ws[b, :min(int(c), mw)] for b, c in enumerate(o["count"])]
    assert o["xyz"].dtype == np.float32 and o["labels"].dtype == np.int64 and all(o[k].dtype == np.int32 for k in ("rows", "count", "center_idx", "info"))
    assert o["xyz"].shape == (B, blocks.num_point, 3) and o["labels"].shape == o["rows"].shape == (B, blocks.num_point)
    return o


def member_mask(p, centres):
    """[len(centres), P] bool: the reference's np.where test of every centre's column"""
    cx, cy = p[centres, 0][:, None], p[centres, 1][:, None]
    return (p[None, :, 0] >= cx - 0.5) & (p[None, :, 0] <= cx + 0.5) & (p[None, :, 1] >= cy - 0.5) & (p[None, :, 1] <= cy + 0.5)


def check_injected(blocks, dev, rooms, room, centres, chunk=2048):
    """count == np.where's, every row a member, xyz / labels those of the rows (centred exactly), member list == the restatement's order"""
    p = np.asarray(rooms[room][0])[:, :3].astype(np.float64)
    lab = rooms[room][1].astype(np.int64)
    ref = R.RefSampler([rooms[room]], blocks.num_point)
    counts = []
    for s in range(0, len(centres), chunk):
        c = np.asarray(centres[s:s + chunk])
        o = run(blocks, dev, [room] * len(c), np.arange(s, s + len(c)), center_idx=c)
        mask = member_mask(p, c)
        assert np.array_equal(o["count"], mask.sum(axis=1))
        assert np.array_equal(o["center_idx"], c) and np.all(o["info"] == 1)
        rows = o["rows"].astype(np.int64)
        assert rows.min() >= 0 and np.take_along_axis(mask, rows, axis=1).all()
        assert np.array_equal(o["labels"], lab[rows])
        want = np.stack([(p[rows, 0] - p[c, 0][:, None]).astype(np.float32), (p[rows, 1] - p[c, 1][:, None]).astype(np.float32),
                         p[rows, 2].astype(np.float32)], axis=2)
        assert np.array_equal(o["xyz"], want)
        for b in range(0, len(c), 37):                                        # the compacted list: cells row-major, ascending inside a cell
            assert np.array_equal(o["members"][b], ref.members(0, c[b])), (room, c[b])
        counts.append(o["count"])
    return np.concatenate(counts)


def test_counts_and_members_room_a(blocks, dev, rooms):
    p = rooms[A][0]
    centres = np.where(p[:, 2] == 0)[0]
    assert centres.size == 1617
    counts = check_injected(blocks, dev, rooms, A, centres)
    assert counts.min() == 648 and counts.max() == 2312 and (counts == 2048).any() and (counts <= 1024).any()


def test_counts_and_members_room_b_every_point(blocks, dev, rooms):
    counts = check_injected(variant(blocks, num_point=256), dev, rooms, B_, np.arange(rooms[B_][0].shape[0]))
    assert counts.min() == 486 and counts.max() == 1734


@pytest.fixture(scope="module")
def whole(rooms):
    """the restatement of 256 items over rooms A and B for two seeds and two epochs, computed once"""
    ref = R.RefSampler(rooms[:2], 2048)
    room_ids = np.arange(256) % 2
    item_ids = np.arange(256) * 3 + 1
    return room_ids, item_ids, {(s, e): [ref.item(int(r), int(i), s, e) for r, i in zip(room_ids, item_ids)] for s in (0, 7) for e in (0, 3)}


def test_whole_sampler_equals_restatement(blocks, dev, whole):
    room_ids, item_ids, refs = whole
    firsts = []
    for (seed, epoch), ref in refs.items():
        o = run(blocks, dev, room_ids, item_ids, seed, epoch)
        for k in ("center_idx", "info", "count"):
            assert np.array_equal(o[k], np.array([r[k] for r in ref])), (k, seed, epoch)
        for k in ("rows", "xyz", "labels"):
            assert np.array_equal(o[k], np.stack([r[k] for r in ref])), (k, seed, epoch)
        assert all(np.array_equal(m, r["members"]) for m, r in zip(o["members"], ref))
        firsts.append(o["center_idx"])
    assert not any(np.array_equal(firsts[0], f) for f in firsts[1:])         # seed and epoch both move the draws


def test_retry_path(blocks, dev, whole):
    room_ids, item_ids, refs = whole
    ref = refs[(0, 0)]
    retried = np.array([r["counts"][0] <= 1024 for r in ref])
    assert retried.sum() >= 5, "mis-specified: too few items whose first attempt is rejected"
    o = run(blocks, dev, room_ids, item_ids, 0, 0)
    assert np.all(o["info"][retried] > 1) and np.all(o["count"][retried] > 1024)
    assert np.all(o["info"][~retried] == 1) and np.all(o["count"] > 1024)


def test_fallback_takes_the_fullest_attempt(blocks, dev, rooms):
    v = variant(blocks, max_tries=8)
    ref = R.RefSampler(rooms[:3], 2048, max_tries=8)
    items = np.arange(40)
    o = run(v, dev, [C] * 40, items, 5, 2)
    want = [ref.item(C, int(i), 5, 2) for i in items]
    assert np.all(o["info"] == -8)
    tie = 0
    for b, w in enumerate(want):
        best = int(np.argmax(w["counts"]))                                   # the largest count, the earliest on ties
        assert w["counts"][best] == max(w["counts"]) and w["center_idx"] == R.center_draw(R.item_key(5, 2, b), best, 600)
        tie += w["counts"].count(max(w["counts"])) > 1
        assert o["center_idx"][b] == w["center_idx"] and o["count"][b] == w["count"] <= 216
        assert np.array_equal(o["rows"][b], w["rows"]) and np.array_equal(o["xyz"][b], w["xyz"]) and np.array_equal(o["labels"][b], w["labels"])
        assert np.isin(o["rows"][b], w["members"]).all() and np.unique(o["rows"][b]).size <= w["count"] < 2048      # with replacement
    assert tie >= 1, "mis-specified: no item with tied attempts"
    assert len({w["counts"].index(max(w["counts"])) for w in want}) > 2      # ... and not always the first or the last attempt


def test_without_replacement(blocks, dev, rooms):
    p = rooms[A][0]
    ref = R.RefSampler(rooms[:1], 2048)
    level0 = np.where(p[:, 2] == 0)[0]                                       # (a column's count depends on x and y only)
    counts = member_mask(p, level0).sum(axis=1)
    exact, full = level0[counts == 2048], level0[counts == 2312]
    assert exact.size == 4 and full.size > 0                                 # 16 x 16 columns: one clipped column each way, four places
    o = run(blocks, dev, [A] * exact.size, np.arange(exact.size), 1, 0, center_idx=exact)
    for b, c in enumerate(exact):
        assert np.array_equal(np.sort(o["rows"][b]), np.sort(ref.members(0, c)))                   # a permutation of the member list
        assert not np.array_equal(o["rows"][b], ref.members(0, c))
    c = int(full[0])
    mem = ref.members(0, c)
    o = run(blocks, dev, [A] * 400, np.arange(400), 1, 0, center_idx=[c] * 400)
    assert np.all(o["count"] == 2312)
    taken = np.zeros((400, p.shape[0]), bool)
    np.put_along_axis(taken, o["rows"].astype(np.int64), True, axis=1)
    assert np.all(taken.sum(axis=1) == 2048) and not taken[:, np.setdiff1d(np.arange(p.shape[0]), mem)].any()     # 2,048 distinct members
    # over 400 item ids every member is selected at least once and left out at least once (a proper draw misses this with p < 1e-20: 0.886^400)
    assert taken[:, mem].any(axis=0).all() and (~taken[:, mem]).any(axis=0).all()


def test_batch_independence_and_determinism(blocks, dev):
    room_ids = np.array([A, B_, D, E, E32, A, B_, E] * 6)
    item_ids = np.arange(48) * 11 + 5
    one = run(blocks, dev, room_ids, item_ids, 3, 1)
    again = run(blocks, dev, room_ids, item_ids, 3, 1)
    parts = [run(blocks, dev, room_ids[s:s + 8], item_ids[s:s + 8], 3, 1) for s in range(0, 48, 8)]
    for k in ("xyz", "labels", "rows", "count", "center_idx", "info"):
        assert np.array_equal(one[k], again[k]), k
        assert np.array_equal(one[k].view(np.uint32 if k == "xyz" else one[k].dtype), np.concatenate([q[k] for q in parts]).view(
            np.uint32 if k == "xyz" else one[k].dtype)), k


@pytest.mark.parametrize("room", [E, E32])
def test_random_coordinates(blocks, dev, rooms, room):
    p = np.asarray(rooms[room][0]).astype(np.float64)
    centres = np.random.default_rng(8).integers(0, p.shape[0], 128)
    o = run(blocks, dev, [room] * 128, np.arange(128), center_idx=centres)
    mask = member_mask(p, centres)
    assert np.array_equal(o["count"], mask.sum(axis=1))
    for b in range(128):
        assert np.array_equal(np.sort(o["members"][b]), np.where(mask[b])[0]), b                   # the member set is float64 np.where's
    rows = o["rows"].astype(np.int64)
    want = np.stack([(p[rows, 0] - p[centres, 0][:, None]).astype(np.float32), (p[rows, 1] - p[centres, 1][:, None]).astype(np.float32),
                     p[rows, 2].astype(np.float32)], axis=2)
    assert np.array_equal(o["xyz"], want) and np.take_along_axis(mask, rows, axis=1).all()
    if room == E32:                                                          # the float32 room really differs from the float64 one
        assert not np.array_equal(p, rooms[E][0])


def test_edge_rooms_and_sizes(blocks, dev, rooms):
    ref = R.RefSampler(rooms, 2048)
    o = run(blocks, dev, [D] * 4, [0, 1, 2, 3], 2, 0)
    assert np.all(o["count"] == 1500) and np.all(o["info"] == 1)             # one cell, accepted at attempt 0
    for b in range(4):
        w = ref.item(D, b, 2, 0)
        assert np.array_equal(o["rows"][b], w["rows"]) and np.array_equal(o["xyz"][b], w["xyz"])
    for n in (1, 4096):
        v, rn = variant(blocks, num_point=n), R.RefSampler(rooms, n)
        o = run(v, dev, [A] * 6, np.arange(6), 4, 1)
        for b in range(6):
            w = rn.item(A, b, 4, 1)
            assert o["count"][b] == w["count"] and o["info"][b] == w["info"] and np.array_equal(o["rows"][b], w["rows"])
            assert np.array_equal(o["xyz"][b], w["xyz"]) and np.array_equal(o["labels"][b], w["labels"])
    o = run(blocks, dev, [B_], [77], 1, 1)                                   # a batch of 1
    w = ref.item(B_, 77, 1, 1)
    assert o["count"][0] == w["count"] and o["info"][0] == w["info"] and np.array_equal(o["rows"][0], w["rows"])


def test_argument_checks(blocks, dev, rooms):
    import act_amd.kernels as K
    from act_amd.datasets import DeviceS3DISBlocks
    r, it = i32(dev, [0, 1]), i32(dev, [0, 1])
    ix = blocks.index
    with pytest.raises(ValueError):
        K.s3dis_sample(ix, r, it, 0, 0, 0)                                   # num_point <= 0
    with pytest.raises(ValueError):
        K.s3dis_sample(ix, r, it, -5, 0, 0)
    for bad in ([0, 6], [-1, 0]):
        with pytest.raises(ValueError):
            K.s3dis_sample(ix, i32(dev, bad), it, 64, 0, 0)                  # a room id out of range
    with pytest.raises(ValueError):
        K.s3dis_sample(ix, r.long(), it, 64, 0, 0)                           # wrong dtypes
    with pytest.raises(ValueError):
        K.s3dis_sample(ix, r, it.float(), 64, 0, 0)
    with pytest.raises(ValueError):
        K.s3dis_sample(ix, r, it, 64, 0, 0, center_idx=i32(dev, [0, 1]).long())
    with pytest.raises(ValueError):
        K.s3dis_sample(ix, r, i32(dev, [0, 1, 2]), 64, 0, 0)                 # wrong shapes
    with pytest.raises(ValueError):
        K.s3dis_sample(ix, r.view(2, 1), it.view(2, 1), 64, 0, 0)
    with pytest.raises(ValueError):
        K.s3dis_sample(ix, r, it, 64, 0, 0, center_idx=i32(dev, [0]))
    with pytest.raises(ValueError):
        K.s3dis_sample(ix, r, it, 64, 0, 0, center_idx=i32(dev, [0, 13680]))  # a centre that is not a point of its room (B has 13,680)
    with pytest.raises(ValueError):
        K.s3dis_sample(ix, r.cpu(), it.cpu(), 64, 0, 0)
    with pytest.raises(ValueError):
        K.s3dis_sample(ix, r, it, 64, 0, 0, ws=torch.empty(2 * ix.max_window - 1, dtype=torch.int32, device=dev))   # a workspace too small
    with pytest.raises(ValueError):
        K.s3dis_sample(ix, r, it, 64, 0, 0, ws=torch.empty(2 * ix.max_window, dtype=torch.float32, device=dev))
    bad = copy.copy(ix)
    bad.labels = ix.labels.long()
    with pytest.raises(ValueError):
        K.s3dis_sample(bad, r, it, 64, 0, 0)
    out = K.s3dis_sample(ix, r, it, 64, 0, 0, ws=torch.empty(2 * ix.max_window, dtype=torch.int32, device=dev))     # the smallest that will do
    assert int(out[3].min()) > 1024
    p, l = rooms[C]
    q = p.copy()
    q[3, 0] = np.nan
    with pytest.raises(ValueError):
        DeviceS3DISBlocks([q], [l], 64, device=dev)                          # NaN coordinates at construction


def test_epoch_iterator_on_the_device(blocks, dev):
    got = list(blocks.epoch(16, 2, 5))
    n = len(blocks.room_idxs)
    assert len(got) == n // 16 and n // 16 >= 2
    for pts, target in got:
        assert pts.shape == (16, 2048, 3) and pts.dtype == torch.float32 and target.shape == (16, 2048) and target.dtype == torch.int64
        assert pts.device == dev and target.device == dev and bool(torch.isfinite(pts).all()) and int(target.min()) >= 0
    order = np.random.default_rng((5, 2)).permutation(n)
    o = run(blocks, dev, blocks.room_idxs[order][16:32], np.arange(16, 32), 5, 2)
    assert np.array_equal(got[1][0].cpu().numpy(), o["xyz"]) and np.array_equal(got[1][1].cpu().numpy(), o["labels"])
    last = list(blocks.epoch(16, 2, 5, drop_last=False))[-1]
    assert n % 16 == 0 or last[0].shape[0] == n % 16


def test_runner_with_the_device_sampler(tmp_path):
    cmd = [sys.executable, "-m", "act_amd.tools.runner_semseg", "--synthetic", "--device_sampler", "--max_steps", "3", "--eval_batches", "2",
           "--batch_size", "8", "--log_every", "1", "--log_dir", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-4000:]
    losses = [float(x) for x in re.findall(r"step \d+: loss ([0-9.naninf]+)", r.stdout)]
    assert len(losses) == 3 and np.all(np.isfinite(losses))
    assert re.search(r"device sampler: rooms \d+ bytes, index \d+ bytes", r.stdout)
    assert re.search(r"best mIoU ([0-9.]+)", r.stdout)
