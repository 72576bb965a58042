"""CPU: S3DIS data pipeline, synthetic rooms, the segmentation model's state_dict layout and the runner's argument defaults (no GPU)."""
import os

import numpy as np

from tests.conftest import golden


def _write_rooms(tmp_path):
    """two tiny rooms of area 1 and one of area 5, xyzrgbl float32"""
    rs = np.random.RandomState(5)
    rooms = {}
    for name, n, lab_hi in (("Area_1_office_1.npy", 3000, 13), ("Area_1_hall_2.npy", 1800, 7), ("Area_5_office_3.npy", 2500, 13)):
        xyz = rs.uniform([0, 0, 0], [1.2, 1.1, 3.0], size=(n, 3))
        rgb = rs.uniform(0, 255, size=(n, 3))
        lab = rs.randint(0, lab_hi, size=n)
        d = np.concatenate([xyz, rgb, lab[:, None]], axis=1).astype(np.float32)
        np.save(os.path.join(tmp_path, name), d)
        rooms[name] = d
    (tmp_path / "readme.txt").write_text("not a room")
    return rooms


def _restated_item(points, labels, num_point, rng):
    """dataset.py:119-147 restated with the same generator calls"""
    n = points.shape[0]
    while True:
        center = points[rng.choice(n)][:3]
        bmin, bmax = center - [0.5, 0.5, 0], center + [0.5, 0.5, 0]
        idx = np.where((points[:, 0] >= bmin[0]) & (points[:, 0] <= bmax[0]) & (points[:, 1] >= bmin[1]) & (points[:, 1] <= bmax[1]))[0]
        if idx.size > 1024:
            break
    sel = rng.choice(idx, num_point, replace=idx.size < num_point)
    sp = points[sel, :].copy()
    sp[:, 0] -= center[0]
    sp[:, 1] -= center[1]
    return sp[:, :3].astype(np.float32), labels[sel], center, idx


def test_s3dis_split_weights_and_blocks(tmp_path):
    from act_amd.datasets.S3DISDataset import S3DISDataset
    rooms = _write_rooms(tmp_path)
    tr = S3DISDataset("train", str(tmp_path), num_point=1024, test_area=5, rng=np.random.default_rng(3))
    te = S3DISDataset("test", str(tmp_path), num_point=1024, test_area=5, rng=np.random.default_rng(3))
    assert tr.rooms == ["Area_1_hall_2.npy", "Area_1_office_1.npy"] and te.rooms == ["Area_5_office_3.npy"]
    # labelweights = (max(p) / p)^(1/3) over the split's histogram
    labs = np.concatenate([rooms[r][:, 6] for r in tr.rooms])
    hist = np.histogram(labs, range(14))[0].astype(np.float32)
    p = hist / hist.sum()
    np.testing.assert_allclose(tr.labelweights, np.power(p.max() / p, 1 / 3.0), rtol=1e-6)
    # rooms in proportion to their point counts
    counts = np.array([1800, 3000])
    num_iter = int(counts.sum() / 1024)
    expect = np.concatenate([[i] * int(round(c / counts.sum() * num_iter)) for i, c in enumerate(counts)])
    np.testing.assert_array_equal(tr.room_idxs, expect)
    # items against the restatement with the same seeded generator
    rng = np.random.default_rng(3)
    for i in range(len(tr)):
        xyz, lab = tr[i]
        r = tr.room_idxs[i]
        d = rooms[tr.rooms[r]]
        exyz, elab, center, idx = _restated_item(d[:, :6], d[:, 6], 1024, rng)
        assert xyz.shape == (1024, 3) and xyz.dtype == np.float32 and lab.shape == (1024,)
        np.testing.assert_array_equal(xyz, exyz)
        np.testing.assert_array_equal(lab, elab)
        assert np.all(np.abs(xyz[:, :2]) <= 0.5 + 1e-6)                  # inside the 1 m x 1 m block around its centre
        np.testing.assert_array_equal(xyz[:, 2], exyz[:, 2])              # z is not centred
    assert len(te) == int(2500 / 1024) and te[0][0].shape == (1024, 3)


def test_s3dis_small_block_draws_with_replacement(tmp_path):
    from act_amd.datasets.S3DISDataset import S3DISDataset
    _write_rooms(tmp_path)
    ds = S3DISDataset("train", str(tmp_path), num_point=4096, test_area=5, rng=np.random.default_rng(0))
    xyz, lab = ds[0]
    assert xyz.shape == (4096, 3) and lab.shape == (4096,)
    assert len(np.unique(xyz, axis=0)) < 4096                             # fewer points in the block than asked: repeats


def test_synthetic_rooms_deterministic_and_complete():
    from act_amd.datasets.S3DISDataset import SyntheticS3DIS
    a = SyntheticS3DIS("train", 2048, num_rooms=3, seed=4)
    b = SyntheticS3DIS("train", 2048, num_rooms=3, seed=4)
    c = SyntheticS3DIS("train", 2048, num_rooms=3, seed=5)
    assert set(np.unique(np.concatenate(a.room_labels)).astype(int)) == set(range(13))
    for ra, rb in zip(a.room_points, b.room_points):
        np.testing.assert_array_equal(ra, rb)
    assert not np.array_equal(a.room_points[0], c.room_points[0])
    for i in (0, 5):
        xa, la = a[i]
        xb, lb = b[i]
        np.testing.assert_array_equal(xa, xb)
        np.testing.assert_array_equal(la, lb)
        assert xa.shape == (2048, 3) and la.dtype == np.int64 and la.min() >= 0 and la.max() < 13
    assert np.all(np.isfinite(a.labelweights)) and a.labelweights.min() == 1.0
    te = SyntheticS3DIS("test", 2048, num_rooms=3, seed=4)
    assert not np.array_equal(te.room_points[0], a.room_points[0])     # held-out rooms


def test_state_dict_matches_reference_layout():
    from act_amd.models.semseg import get_model
    g = golden("g18_semseg")
    sd = get_model(13).state_dict()
    assert list(sd.keys()) == list(g["sd_keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(g["sd_shapes"])


def test_runner_defaults_match_reference():
    from act_amd.tools.runner_semseg import parse_args, REFERENCE_ARGS
    g = golden("g18_semseg")
    ref = dict(zip(g["args_names"], g["args_values"]))
    ours = vars(parse_args([]))
    assert set(ref) == set(REFERENCE_ARGS)
    assert {k: repr(ours[k]) for k in REFERENCE_ARGS} == ref
    assert ours["synthetic"] is False and ours["max_steps"] == 0


def test_seg_metrics_restate_reference():
    """OA / mAcc / mIoU from a confusion matrix == main.py:243-300 restated over the label / prediction arrays"""
    from act_amd.tools.runner_semseg import seg_metrics
    rs = np.random.RandomState(2)
    lab = rs.randint(0, 13, size=5000)
    pred = np.where(rs.rand(5000) < 0.6, lab, rs.randint(0, 13, size=5000))
    pred[pred == 12] = 11                                                 # a class never predicted
    cm = np.zeros((13, 13), np.int64)
    np.add.at(cm, (lab, pred), 1)
    m = seg_metrics(cm)
    seen = [np.sum(lab == l) for l in range(13)]
    corr = [np.sum((pred == l) & (lab == l)) for l in range(13)]
    deno = [np.sum((pred == l) | (lab == l)) for l in range(13)]
    assert m["miou"] == np.mean(np.array(corr) / (np.array(deno, dtype=np.float64) + 1e-6))
    assert m["macc"] == np.mean(np.array(corr) / (np.array(seen, dtype=np.float64) + 1e-6))
    assert m["oa"] == np.sum(pred == lab) / float(lab.size)
