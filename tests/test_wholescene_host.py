"""CPU: whole-room testing host side -- the restated ScannetDatasetWholeScene, its block table, the metric lines of main_test.py and the runner's
argument defaults, against tests/golden/g20_wholescene.npz (recorded from the reference; no GPU)."""
import os

import numpy as np
import pytest

from tests.conftest import golden


def _rooms(tmp_path):
    g = golden("g20_wholescene")
    root = tmp_path / "rooms"
    root.mkdir()
    for name in g["file_list"]:
        np.save(root / name, g["room_" + name[len("Area_5_room_"):-4]])
    return g, str(root)


def test_numpy_major_matches_fixture():
    """the block bounds follow NumPy's scalar promotion rules (NumPy 2: float32 scalar op Python float stays float32)"""
    g = golden("g20_wholescene")
    assert str(g["numpy_version"]).split(".")[0] == np.__version__.split(".")[0]


def test_getitem_restates_reference_bit_for_bit(tmp_path):
    from act_amd.datasets.S3DISDataset import S3DISWholeScene, ScannetDatasetWholeScene
    assert ScannetDatasetWholeScene is S3DISWholeScene
    g, root = _rooms(tmp_path)
    ds = S3DISWholeScene(root, block_points=int(g["block_points"]), split="test", test_area=5)
    assert sorted(ds.file_list) == sorted(g["file_list"])
    assert ds.labelweights.dtype == g["labelweights"].dtype
    assert np.array_equal(ds.labelweights, g["labelweights"]) and np.isinf(ds.labelweights).sum() == 1
    rng = np.random.RandomState(int(g["seed"]))                        # np.random.seed(s), then the rooms in the reference's order
    for name in g["file_list"]:
        tag = name[len("Area_5_room_"):-4]
        i = ds.file_list.index(name)
        data_room, label_room, smpw, index_room = ds.__getitem__(i, rng)
        assert index_room.dtype == np.int64
        assert np.array_equal(index_room.astype(np.int32), g["index_room_" + tag]), tag
        xyz = data_room[:, :, :3].astype(np.float32)
        assert np.array_equal(xyz.view(np.int32), g["data_room_" + tag].view(np.int32)), tag
        assert smpw.dtype == g["sample_weight_" + tag].dtype and np.array_equal(smpw, g["sample_weight_" + tag]), tag
        assert np.array_equal(label_room, ds.semantic_labels_list[i].astype(int)[index_room]), tag


def test_block_table_matches_getitem_blocks(tmp_path):
    """the device table's thresholds select exactly the golden's blocks (np.where over the float64-widened table == the reference's)"""
    from act_amd.datasets.S3DISDataset import S3DISWholeScene
    g, root = _rooms(tmp_path)
    ds = S3DISWholeScene(root, block_points=256)
    for name in g["file_list"]:
        i = ds.file_list.index(name)
        tab, gx, gy = ds.block_table(i)
        xyz = ds.scene_points_list[i][:, :3].astype(np.float64)
        blocks = []
        for b in range(gx * gy):
            lo_x, hi_x, lo_y, hi_y = tab[b, :4]
            idx = np.where((xyz[:, 0] >= lo_x) & (xyz[:, 0] <= hi_x) & (xyz[:, 1] >= lo_y) & (xyz[:, 1] <= hi_y))[0]
            if idx.size:
                blocks.append(set(idx.tolist()))
        rows = g["index_room_" + name[len("Area_5_room_"):-4]].reshape(-1)
        got, k = [], 0
        for s in blocks:
            n = -(-len(s) // 256) * 256
            got.append(set(rows[k:k + n].tolist()))
            k += n
        assert k == rows.size and got == blocks, name
        # each axis' intervals are non-decreasing (the device binary search relies on it)
        for c in range(4):
            axis = tab[:gx, c] if c < 2 else tab[::gx, c]
            assert np.all(np.diff(axis) >= 0)


def test_too_narrow_room_raises_value_error(tmp_path):
    from act_amd.datasets.S3DISDataset import S3DISWholeScene
    d = np.zeros((50, 7), np.float32)
    d[:, 0] = np.linspace(0, 0.4, 50)
    d[:, 1] = np.linspace(0, 3, 50)
    np.save(tmp_path / "Area_5_narrow.npy", d)
    ds = S3DISWholeScene(str(tmp_path), block_points=256)
    with pytest.raises(ValueError, match="Area_5_narrow"):
        ds.block_table(0)


def test_metric_lines_reproduce_reference_from_vote_pool():
    from act_amd.tools.runner_semseg_test import metric_lines
    g = golden("g20_wholescene")
    scene_cms = []
    for name in g["file_list"]:
        tag = name[len("Area_5_room_"):-4]
        pool = g["pool_" + tag]
        pred = np.argmax(pool, 1)
        lab = g["room_" + tag][:, 6].astype(int)
        cm = np.zeros((13, 13), np.int64)
        np.add.at(cm, (lab, pred), 1)
        scene_cms.append((name[:-4], cm))
    rooms, table, finals, _ = metric_lines(scene_cms)
    printed = [str(x) for x in g["printed"]]
    assert rooms == [l for l in printed if l.startswith("Mean IoU of")]
    assert table.splitlines()[1:] == [l for l in printed if l.startswith("class ")]
    assert finals == [l for l in printed if l.startswith("eval ")]


def test_runner_defaults_match_reference():
    from act_amd.tools.runner_semseg_test import parse_args, REFERENCE_ARGS
    g = golden("g20_wholescene")
    ref = dict(zip(g["args_names"], g["args_values"]))
    ours = vars(parse_args([]))
    assert set(ref) == set(REFERENCE_ARGS)
    assert {k: repr(ours[k]) for k in REFERENCE_ARGS} == ref
    assert ours["synthetic"] is False and ours["seed"] == 0 and ours["max_rooms"] == 0


def test_synthetic_whole_scene_writes_area_files(tmp_path):
    from act_amd.datasets.S3DISDataset import SyntheticS3DISWholeScene, SyntheticS3DIS
    ds = SyntheticS3DISWholeScene(str(tmp_path), 256, num_rooms=2, points_per_room=4000)
    assert sorted(os.listdir(tmp_path)) == ["Area_5_synthetic_0.npy", "Area_5_synthetic_1.npy"]
    held = SyntheticS3DIS("test", 256, num_rooms=2, points_per_room=4000)      # the same generator as the training runner's test split
    for name, pts, lab in zip(ds.file_list, ds.scene_points_list, ds.semantic_labels_list):
        k = int(name[-5])
        assert np.array_equal(pts, held.room_points[k]) and np.array_equal(lab, held.room_labels[k])
