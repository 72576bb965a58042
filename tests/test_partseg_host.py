"""CPU: ShapeNetPart data pipeline, synthetic shapes, the part-segmentation model's state_dict layout, the runner's argument defaults and the
host metric function against a transcription of the reference's evaluation loop (no GPU)."""
import json
import os

import numpy as np

from tests.conftest import golden

SEG_CLASSES = {'Earphone': [16, 17, 18], 'Motorbike': [30, 31, 32, 33, 34, 35], 'Rocket': [41, 42, 43],
               'Car': [8, 9, 10, 11], 'Laptop': [28, 29], 'Cap': [6, 7], 'Skateboard': [44, 45, 46], 'Mug': [36, 37],
               'Guitar': [19, 20, 21], 'Bag': [4, 5], 'Lamp': [24, 25, 26, 27], 'Table': [47, 48, 49],
               'Airplane': [0, 1, 2, 3], 'Pistol': [38, 39, 40], 'Chair': [12, 13, 14, 15], 'Knife': [22, 23]}


def _write_tree(root):
    """three categories in the reference's layout: synsetoffset2category.txt, train_test_split/*.json, <synset>/<token>.txt"""
    rs = np.random.RandomState(7)
    cats = [("Airplane", "02691156", [0, 1, 2, 3]), ("Bag", "02773838", [4, 5]), ("Cap", "02954340", [6, 7])]
    (root / "synsetoffset2category.txt").write_text("".join(f"{c}\t{s}\n" for c, s, _ in cats))
    split = {"train": [], "val": [], "test": []}
    shapes = {}
    for ci, (c, syn, parts) in enumerate(cats):
        os.makedirs(root / syn)
        for j in range(4):
            tok = f"{syn[-3:]}{j:03d}"
            n = 300 + 37 * j
            xyz = rs.uniform(-3, 5, size=(n, 3))
            nrm = rs.standard_normal((n, 3))
            lab = rs.choice(parts, size=n)
            np.savetxt(root / syn / f"{tok}.txt", np.concatenate([xyz, nrm, lab[:, None]], 1), fmt="%.6f")
            shapes[(c, tok)] = np.loadtxt(root / syn / f"{tok}.txt").astype(np.float32)
            split[("train", "train", "val", "test")[j]].append(f"shape_data/{syn}/{tok}")
    os.makedirs(root / "train_test_split")
    for s, lst in split.items():
        (root / "train_test_split" / f"shuffled_{s}_file_list.json").write_text(json.dumps(lst))
    return cats, shapes


def test_part_normal_dataset_layout(tmp_path):
    from act_amd.datasets.ShapeNetPartDataset import PartNormalDataset, pc_normalize
    cats, shapes = _write_tree(tmp_path)
    sizes = {"train": 6, "val": 3, "test": 3, "trainval": 9}
    for split, n in sizes.items():
        ds = PartNormalDataset(str(tmp_path), npoints=512, split=split, rng=np.random.default_rng(0))
        assert len(ds) == n
        assert list(ds.classes) == ["Airplane", "Bag", "Cap"] and ds.classes == {"Airplane": 0, "Bag": 1, "Cap": 2}
    ds = PartNormalDataset(str(tmp_path), npoints=512, split="test", rng=np.random.default_rng(3))
    rng = np.random.default_rng(3)
    for i in range(len(ds)):
        pts, cls, seg = ds[i]
        cat, fn = ds.datapath[i]
        d = shapes[(cat, os.path.basename(fn)[:-4])]
        assert pts.shape == (512, 3) and pts.dtype == np.float32 and cls.dtype == np.int32 and cls.shape == (1,)
        assert seg.shape == (512,) and seg.dtype == np.int32 and cls[0] == [c for c, _, _ in cats].index(cat)
        choice = rng.choice(len(d), 512, replace=True)                    # same generator calls as the dataset
        np.testing.assert_allclose(pts, pc_normalize(d[:, :3])[choice], rtol=1e-6, atol=1e-6)
        np.testing.assert_array_equal(seg, d[choice, -1].astype(np.int32))
        assert np.linalg.norm(pts, axis=1).max() <= 1 + 1e-5
    # a second read normalises a copy: the cache keeps the file's values
    ds[0]
    np.testing.assert_array_equal(ds.cache[0][0], shapes[(ds.datapath[0][0], os.path.basename(ds.datapath[0][1])[:-4])][:, :3])
    dn = PartNormalDataset(str(tmp_path), npoints=64, split="train", normal_channel=True, rng=np.random.default_rng(0))
    p, _, _ = dn[0]
    assert p.shape == (64, 6)
    d = shapes[(dn.datapath[0][0], os.path.basename(dn.datapath[0][1])[:-4])]
    rows = [np.where((d[:, 3:6] == r[3:6]).all(1))[0][0] for r in p]      # the normal columns are the file's, untouched
    np.testing.assert_allclose(p[:, :3], pc_normalize(d[:, :3])[rows], rtol=1e-6, atol=1e-6)


def test_seg_tables_and_category_ranges():
    from act_amd.datasets.ShapeNetPartDataset import seg_classes, seg_label_to_cat, CATEGORIES
    assert seg_classes == SEG_CLASSES
    assert len(seg_label_to_cat) == 50 and seg_label_to_cat[0] == "Airplane" and seg_label_to_cat[49] == "Table"
    first = 0
    for c in CATEGORIES:                                                  # alphabetical order: every category's parts are one range
        assert seg_classes[c] == list(range(first, first + len(seg_classes[c])))
        first += len(seg_classes[c])
    assert first == 50


def test_synthetic_shapes_deterministic_and_in_range():
    from act_amd.datasets.ShapeNetPartDataset import SyntheticShapeNetPart, CATEGORIES, seg_classes
    a = SyntheticShapeNetPart("trainval", 1024, shapes_per_category=2, seed=3)
    b = SyntheticShapeNetPart("trainval", 1024, shapes_per_category=2, seed=3)
    c = SyntheticShapeNetPart("trainval", 1024, shapes_per_category=2, seed=4)
    t = SyntheticShapeNetPart("test", 1024, shapes_per_category=2, seed=3)
    assert len(a) == 32
    assert not np.array_equal(a.points[0], c.points[0]) and not np.array_equal(a.points[0], t.points[0])
    for i in range(len(a)):
        np.testing.assert_array_equal(a.points[i], b.points[i])
        pa, ca, sa = a[i]
        pb, cb, sb = b[i]
        np.testing.assert_array_equal(pa, pb)
        np.testing.assert_array_equal(sa, sb)
        cat = CATEGORIES[ca[0]]
        assert ca[0] == i // 2 and pa.shape == (1024, 3) and pa.dtype == np.float32 and sa.dtype == np.int32
        assert set(np.unique(a.seg[i])) == set(seg_classes[cat])          # every part present, none outside the range
        assert abs(np.linalg.norm(a.points[i], axis=1).max() - 1) < 1e-5 and np.abs(a.points[i].mean(0)).max() < 1e-5


def test_state_dict_matches_reference_layout():
    from act_amd.models.partseg import get_model
    g = golden("g19_partseg")
    sd = get_model(50).state_dict()
    assert list(sd.keys()) == list(g["sd_keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(g["sd_shapes"])


def test_runner_defaults_match_reference():
    from act_amd.tools.runner_partseg import parse_args, REFERENCE_ARGS
    g = golden("g19_partseg")
    ref = dict(zip(g["args_names"], g["args_values"]))
    ours = vars(parse_args([]))
    assert set(ref) == set(REFERENCE_ARGS)
    diff = {k for k in REFERENCE_ARGS if repr(ours[k]) != ref[k]}
    assert diff == {"ckpts"} and ours["ckpts"] is None                    # the reference's default names a file of its authors' machine
    assert ours["synthetic"] is False and ours["max_steps"] == 0 and ours["batch_size"] == 16


def reference_metrics(pred, target):
    """main.py:235-299 transcribed over [S, N] prediction / target arrays (float64 numpy); absent categories / parts left out of the means"""
    seg_label_to_cat = {l: c for c in SEG_CLASSES for l in SEG_CLASSES[c]}
    total_seen_class = np.zeros(50)
    total_correct_class = np.zeros(50)
    shape_ious = {c: [] for c in SEG_CLASSES}
    for l in range(50):
        total_seen_class[l] += np.sum(target == l)
        total_correct_class[l] += np.sum((pred == l) & (target == l))
    for i in range(target.shape[0]):
        segp, segl = pred[i], target[i]
        cat = seg_label_to_cat[segl[0]]
        part_ious = [0.0 for _ in range(len(SEG_CLASSES[cat]))]
        for l in SEG_CLASSES[cat]:
            if np.sum(segl == l) == 0 and np.sum(segp == l) == 0:
                part_ious[l - SEG_CLASSES[cat][0]] = 1.0
            else:
                part_ious[l - SEG_CLASSES[cat][0]] = np.sum((segl == l) & (segp == l)) / float(np.sum((segl == l) | (segp == l)))
        shape_ious[cat].append(np.mean(part_ious))
    all_ious = [v for c in shape_ious for v in shape_ious[c]]
    per_cat = {c: np.mean(v) for c, v in shape_ious.items() if v}
    m = total_seen_class > 0
    return dict(accuracy=np.sum(pred == target) / float(target.size), class_avg_accuracy=np.mean(total_correct_class[m] / total_seen_class[m]),
                class_avg_iou=np.mean(list(per_cat.values())), inctance_avg_iou=np.mean(all_ious), per_category=per_cat)


def counts_from_arrays(pred, target):
    """the records the evaluation kernel writes, built on the host from prediction / target arrays"""
    from act_amd.datasets.ShapeNetPartDataset import CATEGORIES
    seg_label_to_cat = {l: c for c in SEG_CLASSES for l in SEG_CLASSES[c]}
    S = target.shape[0]
    counts = np.zeros((S, 16), np.int32)
    for i in range(S):
        cat = seg_label_to_cat[target[i, 0]]
        parts = SEG_CLASSES[cat]
        for j, l in enumerate(parts):
            counts[i, j] = np.sum((pred[i] == l) & (target[i] == l))
            counts[i, 6 + j] = np.sum((pred[i] == l) | (target[i] == l))
        counts[i, 12], counts[i, 13] = CATEGORIES.index(cat), len(parts)
    seen = np.array([np.sum(target == l) for l in range(50)], np.int64)
    correct = np.array([np.sum((pred == l) & (target == l)) for l in range(50)], np.int64)
    return counts, seen, correct


def test_part_metrics_restate_reference():
    from act_amd.tools.runner_partseg import part_metrics
    rs = np.random.RandomState(11)
    S, N = 40, 300
    cats = sorted(SEG_CLASSES)
    target = np.zeros((S, N), np.int64)
    pred = np.zeros((S, N), np.int64)
    for i in range(S):
        parts = SEG_CLASSES[cats[i % 13]]                                  # 13 of the 16 categories occur
        target[i] = rs.choice(parts, size=N)
        pred[i] = np.where(rs.rand(N) < 0.7, target[i], rs.choice(parts, size=N))
    # a part absent from both target and prediction of a shape (IoU 1.0): Motorbike shape with parts 30, 31 only
    mi = [i for i in range(S) if cats[i % 13] == "Motorbike"][0]
    target[mi] = rs.choice([30, 31], size=N)
    target[mi, 0] = 30
    pred[mi] = np.where(rs.rand(N) < 0.5, target[mi], 31)
    counts, seen, correct = counts_from_arrays(pred, target)
    m = part_metrics(counts, seen, correct)
    r = reference_metrics(pred, target)
    for k in ("accuracy", "class_avg_accuracy", "class_avg_iou", "inctance_avg_iou"):
        assert abs(m[k] - r[k]) <= 1e-12, (k, m[k], r[k])
    assert set(m["per_category"]) == set(r["per_category"]) and len(m["per_category"]) == 13
    for c in r["per_category"]:
        assert abs(m["per_category"][c] - r["per_category"][c]) <= 1e-12
    assert (counts[mi, 6 + 2:6 + 6] == 0).all()                            # parts 32..35 absent on both sides
