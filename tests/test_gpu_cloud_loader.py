"""GPU: act_amd/datasets/DeviceClouds.py (resident object datasets) against the host datasets and the numpy restatement, the switch of
tools/builder.dataset_builder, and the two runners on the resident recipes."""
import argparse
import copy
import os

import numpy as np
import pytest
import torch

from tests import cloud_sample_ref as R
from tests.golden.fill import TINY_STAGE2, TINY_FINETUNE

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- ShapeNet, file-backed ---------------------------------------------------------------------------------------------------------------------
def _shapenet(root, M=10, N=64, npoints=16):
    from act_amd.datasets.SyntheticDataset import ShapeNet
    from act_amd.utils.config import EasyDict
    pc_path = os.path.join(root, "pc")
    os.makedirs(pc_path, exist_ok=True)
    g = np.random.default_rng(0)
    clouds = (g.standard_normal((M, N, 3)) + g.uniform(-5, 5, (M, 1, 3))).astype(np.float32)
    names = [(f"{2000 + i % 3:08d}", f"model{i:02d}") for i in range(M)]
    for (tax, mid), c in zip(names, clouds):
        np.save(os.path.join(pc_path, f"{tax}-{mid}.npy"), c)
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("".join(f"{tax}-{mid}.npy\n" for tax, mid in names))
    ds = ShapeNet(EasyDict(N_POINTS=N, subset="train", npoints=npoints, DATA_PATH=str(root), PC_PATH=pc_path))
    return ds, clouds, names


def test_shapenet_epoch_equals_the_restatement(tmp_path):
    from act_amd.datasets import DeviceClouds
    ds, clouds, names = _shapenet(str(tmp_path))
    dc = DeviceClouds.from_dataset(ds, device=DEV)
    assert len(dc) == 10 and dc.npoints == 16 and dc.resident_bytes() == 10 * 64 * 3 * 4
    for drop_last, sizes in ((False, [4, 4, 2]), (True, [4, 4])):
        got = list(dc.epoch(4, epoch=3, seed=7, shuffle=True, drop_last=drop_last))
        want = R.batches(R.epoch_order(10, 7, 3), 4, drop_last)
        assert [len(b[0]) for b in got] == sizes == [len(w) for w in want]
        for (tax, mid, data), ids in zip(got, want):
            assert tax == [names[i][0] for i in ids] and mid == [names[i][1] for i in ids]
            assert data.is_cuda and data.dtype == torch.float32 and tuple(data.shape) == (len(ids), 16, 3)
            for b, i in enumerate(ids):
                assert np.array_equal(_bits(data[b].cpu().numpy()), _bits(R.sample(clouds, i, int(i), 16, 7, 3)[0]))
    seen = sorted(m for _, mids, _ in dc.epoch(4, 0, 0, True, False) for m in mids)
    assert seen == sorted(n[1] for n in names)                                   # every item once
    first = [m for _, mids, _ in dc.epoch(10, 0, 0, shuffle=False, drop_last=False) for m in mids]
    assert first == [n[1] for n in names]                                        # without shuffle: the list's order
    # sample(): the same items by hand, with their source rows
    ids = torch.tensor([3, 9], dtype=torch.int32, device=DEV)
    pts, rows = dc.sample(ids, ids, 7, 3, want_rows=True)
    for b, i in enumerate((3, 9)):
        want, wrows = R.sample(clouds, i, i, 16, 7, 3)
        assert np.array_equal(rows[b].cpu().numpy(), wrows) and np.array_equal(_bits(pts[b].cpu().numpy()), _bits(want))


def test_shapenet_cache_round_trips_and_bad_files_are_named(tmp_path):
    from act_amd.datasets import DeviceClouds
    ds, clouds, names = _shapenet(str(tmp_path))
    cache = str(tmp_path / "packed.npy")
    a = DeviceClouds.from_dataset(ds, device=DEV, cache=cache)
    assert os.path.exists(cache) and np.array_equal(np.load(cache), clouds)
    for tax, mid in names:                                                       # the second construction reads the cache alone
        os.remove(os.path.join(ds.pc_path, f"{tax}-{mid}.npy"))
    b = DeviceClouds.from_dataset(ds, device=DEV, cache=cache)
    assert torch.equal(a.clouds, b.clouds) and b.names == a.names
    x, y = next(iter(a.epoch(10, 1, 2)))[2], next(iter(b.epoch(10, 1, 2)))[2]
    assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    np.save(cache, clouds[:9])
    with pytest.raises(ValueError, match="packed.npy"):
        DeviceClouds.from_dataset(ds, device=DEV, cache=cache)
    ds2, _, names2 = _shapenet(str(tmp_path / "second"))
    bad = os.path.join(ds2.pc_path, f"{names2[4][0]}-{names2[4][1]}.npy")
    np.save(bad, np.zeros((63, 3), np.float32))
    with pytest.raises(ValueError, match="model04"):
        DeviceClouds.from_dataset(ds2, device=DEV)
    with pytest.raises(ValueError):
        DeviceClouds(np.full((2, 8, 3), np.inf, np.float32), 4, device=DEV)
    with pytest.raises(ValueError):
        DeviceClouds(np.zeros((2, 8, 3), np.float32), 9, device=DEV)
    with pytest.raises(ValueError):
        DeviceClouds(np.zeros((2, 8, 3), np.float64), 4, device=DEV)


# ---- ModelNet-style data from in-memory arrays -------------------------------------------------------------------------------------------------
def _modelnet(subset, use_normals, M=7, N=40):
    from act_amd.datasets.SyntheticDataset import ModelNet
    g = np.random.default_rng(5)
    ds = ModelNet.__new__(ModelNet)
    ds.npoints, ds.num_category, ds.subset, ds.use_normals, ds.synthetic = N, 4, subset, use_normals, False
    ds.list_of_points = [(g.standard_normal((N, 6)) + [100.0, -50.0, 7.0, 0, 0, 0]).astype(np.float32) for _ in range(M)]
    ds.list_of_labels = [np.array([i % 4]).astype(np.int32) for i in range(M)]
    ds.datapath = [None] * M
    return ds


@pytest.mark.parametrize("use_normals", [False, True])
def test_modelnet_batches_equal_the_host_items(use_normals):
    from act_amd.datasets import DeviceClouds
    C = 6 if use_normals else 3
    test = _modelnet("test", use_normals)
    host = [test[i] for i in range(len(test))]
    dc = DeviceClouds.from_dataset(test, device=DEV)
    assert not dc.permute and not dc.normalize and tuple(dc.clouds.shape) == (7, 40, C)
    got = list(dc.epoch(3, 0, 0, shuffle=False, drop_last=False))
    assert [b[2][0].shape[0] for b in got] == [3, 3, 1]
    i = 0
    for a, b, (pts, lab) in got:
        assert (a, b) == ("ModelNet", "sample") and pts.is_cuda and lab.is_cuda and lab.dtype == torch.int64 and lab.dim() == 1
        for p, l in zip(pts.cpu().numpy(), lab.tolist()):
            assert np.array_equal(_bits(p), _bits(host[i][2][0].numpy())) and l == host[i][2][1]           # pc_norm on the device = on the host
            i += 1
    assert i == 7
    # a shuffled epoch of the test subset: whole items, gathered by the kernel
    ids = R.epoch_order(7, 1, 2)
    (_, _, (pts, lab)), = list(dc.epoch(7, 2, 1, shuffle=True, drop_last=False))
    for b, k in enumerate(ids):
        assert np.array_equal(_bits(pts[b].cpu().numpy()), _bits(host[k][2][0].numpy())) and int(lab[b]) == host[k][2][1]
    # train: every item a permutation of its rows (normals travel with their points), labels follow the items
    train = _modelnet("train", use_normals)
    dt = DeviceClouds.from_dataset(train, device=DEV)
    assert dt.permute and not dt.normalize and torch.equal(dt.clouds, dc.clouds)
    ids = R.epoch_order(7, 3, 4)
    (_, _, (pts, lab)), = list(dt.epoch(7, 4, 3, shuffle=True, drop_last=True))
    assert lab.tolist() == [host[k][2][1] for k in ids]
    for b, k in enumerate(ids):
        rows = R.subset_rows(40, 40, 3, 4, int(k))
        assert not np.array_equal(rows, np.arange(40))
        assert np.array_equal(_bits(pts[b].cpu().numpy()), _bits(host[k][2][0].numpy()[rows]))


def test_scanobjectnn_and_synthetic_twins():
    from act_amd.datasets import DeviceClouds, build_dataset_from_cfg
    from act_amd.datasets.FinetuneDatasets import ScanObjectNN_hardest
    from act_amd.utils.config import EasyDict
    g = np.random.default_rng(2)
    pts, lab = g.standard_normal((5, 128, 3)).astype(np.float32) * 3 + 1, g.integers(0, 15, 5)
    for subset in ("train", "test"):
        ds = ScanObjectNN_hardest(EasyDict(subset=subset, ROOT="none"), reader=lambda path: (pts, lab))
        dc = DeviceClouds.from_dataset(ds, device=DEV)
        (a, b, (p, l)), = list(dc.epoch(5, 0, 0, shuffle=False, drop_last=False))
        assert (a, b) == ("ScanObjectNN", "sample") and l.tolist() == lab.tolist() and dc.permute == (subset == "train")
        for i in range(5):
            rows = R.subset_rows(128, 128, 0, 0, i, permute=subset == "train")
            assert np.array_equal(_bits(p[i].cpu().numpy()), _bits(pts[i][rows]))                              # no normalisation
    syn = build_dataset_from_cfg(EasyDict(NAME="ShapeNet", N_POINTS=8192, SYNTHETIC=True, NUM_SAMPLES=6, DATA_PATH="none", PC_PATH="none"),
                                 EasyDict(subset="train", npoints=32))
    dc = DeviceClouds.from_dataset(syn, device=DEV)
    assert tuple(dc.clouds.shape) == (6, 32, 3) and dc.permute and dc.normalize and dc.names[2] == ("synthetic", "000002")
    assert np.array_equal(_bits(dc.clouds[2].cpu().numpy()), _bits(syn[2][2].numpy()))
    with pytest.raises(ValueError):
        DeviceClouds.from_dataset(object(), device=DEV)


# ---- DDP shards --------------------------------------------------------------------------------------------------------------------------------
def test_two_rank_shards_match_the_restatement(tmp_path):
    from act_amd.datasets import DeviceClouds
    ds, clouds, names = _shapenet(str(tmp_path), M=9)
    dc = DeviceClouds.from_dataset(ds, device=DEV)
    order = R.epoch_order(9, 4, 6, True, 2)
    assert order.size == 10
    by_id = {}
    for rank in (0, 1):
        ids = R.shard(order, rank, 2)
        got = list(dc.epoch(2, 6, 4, shuffle=True, drop_last=True, rank=rank, world_size=2))
        assert len(got) == 2 and [m for _, mids, _ in got for m in mids] == [names[i][1] for i in ids[:4]]
        whole = list(dc.epoch(5, 6, 4, shuffle=True, drop_last=False, rank=rank, world_size=2))[0][2].cpu().numpy()
        for b, i in enumerate(ids):
            assert np.array_equal(_bits(whole[b]), _bits(R.sample(clouds, i, int(i), 16, 4, 6)[0]))
            by_id.setdefault(int(i), []).append(_bits(whole[b]))
    assert sorted(by_id) == list(range(9))
    dup = [v for v in by_id.values() if len(v) == 2]
    assert len(dup) == 1 and np.array_equal(dup[0][0], dup[0][1])                 # the wrapped item: the same bits on both ranks


# ---- the switch and the runners ----------------------------------------------------------------------------------------------------------------
def _args(tmp, **kw):
    a = argparse.Namespace(log_name="test_resident", use_gpu=True, local_rank=0, distributed=False, sync_bn=False, resume=False, start_ckpts=None,
                           ckpts=None, experiment_path=str(tmp), num_workers=0, world_size=1, val_freq=1, vote=False)
    a.__dict__.update(kw)
    return a


def _tiny(cfg, model, bs, **base):
    """the recipe as shipped at a size a test can afford (tests/test_gpu_augment.py's rule): the tiny model, a small synthetic set"""
    from act_amd.utils.config import EasyDict
    cfg.model = EasyDict(copy.deepcopy(model))
    for split in cfg.dataset.values():
        split._base_.update(NUM_SAMPLES=4 * bs, **base)
        split.others.bs = bs
    cfg.total_bs = bs
    return cfg


def test_dataset_builder_switch(tmp_path):
    from act_amd.tools import builder
    from act_amd.datasets import DeviceCloudLoader
    from act_amd.utils.config import EasyDict
    sec = EasyDict(_base_=dict(NAME="ModelNet", N_POINTS=64, NUM_CATEGORY=4, USE_NORMALS=False, SYNTHETIC=True, NUM_SAMPLES=14, DATA_PATH="none"),
                   others=dict(subset="train", bs=4, device_resident=True))
    sampler, loader = builder.dataset_builder(_args(tmp_path, seed=5, num_workers=8), sec)
    assert sampler is loader and type(loader) is DeviceCloudLoader and len(loader) == 3 and loader.seed == 5 and loader.shuffle and loader.drop_last
    first = [b[2][0].clone() for b in loader]                                    # the internal counter: epoch 0, then epoch 1
    second = [b[2][0].clone() for b in loader]
    assert len(first) == 3 and len(second) == 3 and not torch.equal(torch.cat(first), torch.cat(second))
    loader.set_epoch(0)
    again = [b[2][0] for b in loader]
    assert torch.equal(torch.cat(first).view(torch.int32), torch.cat(again).view(torch.int32))
    sec.others.subset = "test"
    _, test = builder.dataset_builder(_args(tmp_path), sec)
    assert len(test) == 4 and test.seed == 0 and not test.shuffle and not test.drop_last
    assert [b[2][0].shape[0] for b in test] == [4, 4, 4, 2]
    # a file-backed ShapeNet section with the cache key
    ds, clouds, names = _shapenet(str(tmp_path))
    cache = str(tmp_path / "cache.npy")
    shp = EasyDict(_base_=dict(NAME="ShapeNet", N_POINTS=64, DATA_PATH=str(tmp_path), PC_PATH=ds.pc_path),
                   others=dict(subset="train", npoints=16, bs=5, device_resident=True, device_cache=cache))
    _, loader = builder.dataset_builder(_args(tmp_path, seed=1), shp)
    assert os.path.exists(cache) and len(loader) == 2
    tax, mid, data = next(iter(loader))
    i = int(R.epoch_order(10, 1, 0)[0])
    assert mid[0] == names[i][1] and np.array_equal(_bits(data[0].cpu().numpy()), _bits(R.sample(clouds, i, i, 16, 1, 0)[0]))


def test_run_net_of_the_resident_pretrain_recipe(tmp_path, monkeypatch):
    from act_amd.tools import runner_pretrain as RP
    from act_amd.datasets import DeviceCloudLoader
    from act_amd.utils.config import cfg_from_yaml_file
    cfg = _tiny(cfg_from_yaml_file("cfgs/synthetic/pretrain_act_distill_resident.yaml"), TINY_STAGE2, 8)
    assert cfg.svm_val and all(s.others.device_resident for s in cfg.dataset.values()) and set(cfg.dataset) == {"train", "val", "extra_train"}
    cfg.dataset.train.others.npoints = 128
    for s in ("val", "extra_train"):
        cfg.dataset[s]._base_.update(N_POINTS=256, NUM_CATEGORY=4)
    seen = []
    real = RP.validate

    def validate(model, extra, test, *a, **k):
        seen.append((type(extra), type(test)))
        return real(model, extra, test, *a, **k)
    monkeypatch.setattr(RP, "validate", validate)
    torch.manual_seed(0)
    log = RP.run_net(_args(tmp_path), cfg, max_steps=3, log_every=1)
    assert len(log) == 3 and np.isfinite(log).all()
    assert seen == [(DeviceCloudLoader, DeviceCloudLoader)]                      # the validation pass went through the resident loaders


def test_run_net_of_the_resident_finetune_recipe(tmp_path):
    from act_amd.tools import runner_finetune as RF
    from act_amd.tools import builder
    from act_amd.datasets import DeviceCloudLoader
    from act_amd.utils.config import cfg_from_yaml_file
    cfg = _tiny(cfg_from_yaml_file("cfgs/synthetic/finetune_modelnet_resident.yaml"), dict(TINY_FINETUNE, cls_dim=4, num_group=32, group_size=16), 8,
                NUM_CATEGORY=4, N_POINTS=2048)
    assert all(s.others.device_resident for s in cfg.dataset.values()) and cfg.npoints == 1024
    torch.manual_seed(0)
    log = RF.run_net(_args(tmp_path), cfg, max_steps=3, log_every=1)
    assert len(log) == 3 and np.isfinite(np.array(log)).all()
    m, _ = RF.test_net(_args(tmp_path, ckpts=os.path.join(tmp_path, "ckpt-last.pth")), cfg, vote_rounds=1)     # validation through the resident test split
    assert 0.0 <= m.acc <= 100.0
    assert type(builder.dataset_builder(_args(tmp_path), cfg.dataset.test)[1]) is DeviceCloudLoader
