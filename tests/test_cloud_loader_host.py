"""CPU: the numpy restatement of the device object-dataset sampler (tests/cloud_sample_ref.py) against the host datasets' own rules, and the
switch of tools/builder.dataset_builder left off."""
import argparse

import numpy as np
import pytest
import torch

from tests import cloud_sample_ref as R

NS = [1, 2, 7, 257, 1024, 1200, 8192]


def cloud(n, offset, seed, c=3):
    """a random cloud; ``offset`` 1000 puts it far from the origin, where the order of the mean's additions shows in the low bits"""
    g = np.random.default_rng(seed)
    pc = (g.standard_normal((n, c)) * [1.0, 0.5, 2.0, 1.0, 1.0, 1.0][:c]).astype(np.float32)
    pc[:, :3] += np.float32(offset)
    return pc


@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("n", NS)
def test_serial_pc_norm_is_numpys_pc_norm(n, offset):
    from act_amd.datasets.SyntheticDataset import pc_norm
    pc = cloud(n, offset, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = pc_norm(pc)
    got = R.pc_norm_serial(pc)
    assert want.dtype == np.float32 and got.dtype == np.float32
    assert np.array_equal(want.view(np.int32), got.view(np.int32))
    six = cloud(n, offset, n + 1, c=6)                                      # ModelNet's in-place rule: the xyz view of an [n,6] array
    with np.errstate(invalid="ignore", divide="ignore"):
        want = pc_norm(six[:, 0:3])
    assert np.array_equal(want.view(np.int32), R.pc_norm_serial(six[:, 0:3]).view(np.int32))
    if n == 1:
        assert np.isnan(got).all()                                          # one point: 0 / 0, as numpy


@pytest.mark.parametrize("N", [1, 2, 3, 5, 64, 100, 8192])
def test_subsets_have_no_repeats(N):
    for n in sorted({1, N, -(-N // 4)}):
        for draw in range(4):
            rows = R.subset_rows(N, n, 3, 1, draw)
            assert rows.shape == (n,) and rows.min() >= 0 and rows.max() < N and np.unique(rows).size == n
    assert np.array_equal(np.sort(R.subset_rows(N, N, 0, 0, 7)), np.arange(N))          # n == N: a permutation
    assert np.array_equal(R.subset_rows(N, N, 0, 0, 7, permute=False), np.arange(N))
    if N >= 64:
        a = R.subset_rows(N, N, 0, 0, 7)
        assert not np.array_equal(a, R.subset_rows(N, N, 0, 0, 8)) and not np.array_equal(a, R.subset_rows(N, N, 0, 1, 7)) \
            and not np.array_equal(a, R.subset_rows(N, N, 1, 0, 7))


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("M", [10, 11, 12, 2])
def test_shards_are_disjoint_up_to_the_padding_and_cover_every_index(M, world):
    from act_amd.datasets.DeviceClouds import epoch_order
    for shuffle in (True, False):
        order = R.epoch_order(M, 5, 2, shuffle, world)
        assert np.array_equal(order, epoch_order(M, 5, 2, shuffle, world))              # the package's order is the restatement's
        pad = -M % world
        assert order.size == M + pad and np.array_equal(np.sort(order[:M]), np.arange(M))
        assert np.array_equal(order[M:], np.resize(order[:M], M + pad)[M:])             # padded by wrapping
        shards = [R.shard(order, r, world) for r in range(world)]
        assert all(s.size == order.size // world for s in shards)
        allv = np.concatenate(shards)
        assert set(allv.tolist()) == set(range(M))
        counts = np.bincount(allv, minlength=M)
        assert counts.sum() == M + pad and (counts >= 1).all() and (counts - 1).sum() == pad        # only the padding repeats
        if not shuffle:
            assert np.array_equal(order[:M], np.arange(M))
    assert not np.array_equal(R.epoch_order(64, 5, 2), R.epoch_order(64, 5, 3))
    assert not np.array_equal(R.epoch_order(64, 5, 2), R.epoch_order(64, 6, 2))


def test_batches_honour_drop_last():
    ids = np.arange(10)
    assert [len(b) for b in R.batches(ids, 4, False)] == [4, 4, 2] and [len(b) for b in R.batches(ids, 4, True)] == [4, 4]


def test_dataset_builder_without_the_key_returns_a_dataloader():
    from act_amd.tools import builder
    from act_amd.utils.config import EasyDict
    sec = EasyDict(_base_=dict(NAME="ModelNet", N_POINTS=64, NUM_CATEGORY=4, USE_NORMALS=False, SYNTHETIC=True, NUM_SAMPLES=12, DATA_PATH="none"),
                   others=dict(subset="train", bs=4))
    args = argparse.Namespace(distributed=False, num_workers=0)
    for others in (dict(subset="train", bs=4), dict(subset="train", bs=4, device_resident=False)):
        sec.others = EasyDict(others)
        sampler, loader = builder.dataset_builder(args, sec)
        assert sampler is None and type(loader) is torch.utils.data.DataLoader and loader.batch_size == 4 and loader.drop_last
        assert len(loader) == 3


def test_selection_frequencies():
    """N = 64, n = 16, draw ids 0 .. 4095, seed 0, epoch 0: a row is chosen with probability 1/4, so its count is binomial with mean 1,024 and
    standard deviation sqrt(4096 * 1/4 * 3/4) = 27.7; every count lies within 6 of them (858 .. 1,190)"""
    counts = np.zeros(64, np.int64)
    for d in range(4096):
        counts += np.bincount(R.subset_rows(64, 16, 0, 0, d), minlength=64)
    print("selection counts: min %d max %d" % (counts.min(), counts.max()))
    assert counts.sum() == 4096 * 16
    assert counts.min() >= 858 and counts.max() <= 1190
