"""ShapeNetPart for part segmentation (reference: part_segmentation/dataset.py:64-162, main.py seg_classes) and a synthetic stand-in.

``PartNormalDataset`` reads the reference's layout under ``root``: ``synsetoffset2category.txt`` (category name, synset directory; the line order
is the category id order), ``train_test_split/shuffled_{train,val,test}_file_list.json`` and one ``<synset>/<token>.txt`` of
``x y z nx ny nz label`` rows per shape.  Items are ``(points float32 [npoints, 3 | 6], cls int32 [1], seg int32 [npoints])``: xyz through
``pc_normalize``, then ``npoints`` rows drawn with replacement.  The reference normalises its cached array in place; here a copy is normalised
(the cache keeps the file's values).  The random stream is an injectable ``numpy.random.Generator``.

``SyntheticShapeNetPart`` generates shapes for all 16 categories for machines without the data: every shape is assembled from primitives (boxes,
cylinders, spheres, discs), each primitive carrying one part label of its category's range, so the labels follow from the geometry.
"""
import json
import os

import numpy as np
import torch.utils.data as data

seg_classes = {'Earphone': [16, 17, 18], 'Motorbike': [30, 31, 32, 33, 34, 35], 'Rocket': [41, 42, 43],
               'Car': [8, 9, 10, 11], 'Laptop': [28, 29], 'Cap': [6, 7], 'Skateboard': [44, 45, 46], 'Mug': [36, 37],
               'Guitar': [19, 20, 21], 'Bag': [4, 5], 'Lamp': [24, 25, 26, 27], 'Table': [47, 48, 49],
               'Airplane': [0, 1, 2, 3], 'Pistol': [38, 39, 40], 'Chair': [12, 13, 14, 15], 'Knife': [22, 23]}
seg_label_to_cat = {label: cat for cat in seg_classes for label in seg_classes[cat]}      # {0: 'Airplane', ..., 49: 'Table'}
CATEGORIES = sorted(seg_classes)          # the order of synsetoffset2category.txt: category id = index
NUM_CATEGORIES = len(CATEGORIES)
NUM_PARTS = 50


def pc_normalize(pc):
    """centre on the centroid, scale into the unit sphere (pointnet_util.py pc_normalize); returns a new array"""
    centroid = np.mean(pc, axis=0)
    pc = pc - centroid
    m = np.max(np.sqrt(np.sum(pc ** 2, axis=1)))
    return pc / m


class PartNormalDataset(data.Dataset):
    def __init__(self, root='./data/shapenetcore_partanno_segmentation_benchmark_v0_normal', npoints=2500, split='train', class_choice=None,
                 normal_channel=False, rng=None):
        self.npoints = npoints
        self.root = root
        self.normal_channel = normal_channel
        self.rng = rng if rng is not None else np.random.default_rng()
        self.cat = {}
        with open(os.path.join(self.root, 'synsetoffset2category.txt'), 'r') as f:
            for line in f:
                ls = line.strip().split()
                if ls:
                    self.cat[ls[0]] = ls[1]
        self.classes_original = dict(zip(self.cat, range(len(self.cat))))
        if class_choice is not None:
            self.cat = {k: v for k, v in self.cat.items() if k in class_choice}
        ids = {}
        for s in ('train', 'val', 'test'):
            with open(os.path.join(self.root, 'train_test_split', f'shuffled_{s}_file_list.json'), 'r') as f:
                ids[s] = set(str(d.split('/')[2]) for d in json.load(f))
        if split == 'trainval':
            keep = ids['train'] | ids['val']
        elif split in ids:
            keep = ids[split]
        else:
            raise ValueError(f'Unknown split: {split}')
        self.meta = {}
        for item in self.cat:
            dir_point = os.path.join(self.root, self.cat[item])
            fns = sorted(os.listdir(dir_point))
            self.meta[item] = [os.path.join(dir_point, os.path.splitext(os.path.basename(fn))[0] + '.txt') for fn in fns if fn[0:-4] in keep]
        self.datapath = [(item, fn) for item in self.cat for fn in self.meta[item]]
        self.classes = {i: self.classes_original[i] for i in self.cat}
        self.seg_classes = seg_classes
        self.cache = {}
        self.cache_size = 20000

    def __getitem__(self, index):
        if index in self.cache:
            point_set, cls, seg = self.cache[index]
        else:
            cat, fn = self.datapath[index]
            cls = np.array([self.classes[cat]]).astype(np.int32)
            d = np.loadtxt(fn).astype(np.float32)
            point_set = d[:, 0:6] if self.normal_channel else d[:, 0:3]
            seg = d[:, -1].astype(np.int32)
            if len(self.cache) < self.cache_size:
                self.cache[index] = (point_set, cls, seg)
        point_set = point_set.copy()
        point_set[:, 0:3] = pc_normalize(point_set[:, 0:3])
        choice = self.rng.choice(len(seg), self.npoints, replace=True)
        return point_set[choice, :], cls, seg[choice]

    def __len__(self):
        return len(self.datapath)


# ---- synthetic shapes ---------------------------------------------------------------------------------------------------------
def _box(rng, n, lo, hi):
    """n points on the surface of the axis-aligned box [lo, hi] (faces in proportion to their area)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    e = hi - lo
    areas = np.array([e[1] * e[2], e[1] * e[2], e[0] * e[2], e[0] * e[2], e[0] * e[1], e[0] * e[1]]) + 1e-9
    face = rng.choice(6, size=n, p=areas / areas.sum())
    p = lo + rng.random((n, 3)) * e
    ax = face // 2
    p[np.arange(n), ax] = np.where(face % 2 == 0, lo[ax], hi[ax])
    return p


def _cyl(rng, n, c, r, h, axis=2):
    """n points on the side of a cylinder of radius r, length h along ``axis``, centred at c"""
    t = rng.random(n) * 2 * np.pi
    z = (rng.random(n) - 0.5) * h
    loc = np.stack([r * np.cos(t), r * np.sin(t), z], 1)
    perm = {0: [2, 0, 1], 1: [0, 2, 1], 2: [0, 1, 2]}[axis]
    return loc[:, perm] + np.asarray(c)


def _sphere(rng, n, c, r, flat=(1.0, 1.0, 1.0), upper=False):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if upper:
        v[:, 2] = np.abs(v[:, 2])
    return v * r * np.asarray(flat) + np.asarray(c)


def _disc(rng, n, c, r, axis=2):
    rr = r * np.sqrt(rng.random(n))
    t = rng.random(n) * 2 * np.pi
    loc = np.stack([rr * np.cos(t), rr * np.sin(t), np.zeros(n)], 1)
    perm = {0: [2, 0, 1], 1: [0, 2, 1], 2: [0, 1, 2]}[axis]
    return loc[:, perm] + np.asarray(c)


def synthetic_shape(cat, rng, n=2048):
    """one shape of category ``cat``: (xyz float32 [n, 3] normalised like pc_normalize, part labels int32 [n] within seg_classes[cat])"""
    P = seg_classes[cat]
    u = lambda a, b: rng.uniform(a, b)
    prims = []                                           # (weight, sampler(k) -> [k, 3], label)

    def add(w, fn, lab):
        prims.append((w, fn, lab))
    if cat == 'Airplane':                                # body, wings, tail, engines
        L, wspan = u(1.6, 2.2), u(1.6, 2.4)
        add(3, lambda k: _cyl(rng, k, (0, 0, 0), 0.12, L, axis=0), P[0])
        add(3, lambda k: _box(rng, k, (-0.25, -wspan / 2, -0.02), (0.15, wspan / 2, 0.02)), P[1])
        add(1, lambda k: _box(rng, k, (-L / 2, -0.02, 0), (-L / 2 + 0.2, 0.02, u(0.3, 0.45))), P[2])
        add(1, lambda k: np.concatenate([_cyl(rng, k // 2, (0.0, -wspan / 4, -0.12), 0.06, 0.3, axis=0),
                                         _cyl(rng, k - k // 2, (0.0, wspan / 4, -0.12), 0.06, 0.3, axis=0)]), P[3])
    elif cat == 'Bag':                                   # bag body, handle
        add(4, lambda k: _box(rng, k, (-0.5, -0.2, 0), (0.5, 0.2, u(0.6, 0.9))), P[0])
        add(1, lambda k: _cyl(rng, k, (0, 0, 1.0), 0.3, 0.04, axis=1) * (1, 1, 1), P[1])
    elif cat == 'Cap':                                   # crown, peak
        add(3, lambda k: _sphere(rng, k, (0, 0, 0), 0.5, (1, 1, u(0.6, 0.9)), upper=True), P[0])
        add(1, lambda k: _box(rng, k, (0.3, -0.3, 0), (0.9, 0.3, 0.02)), P[1])
    elif cat == 'Car':                                   # roof, wheels, body, hood
        add(1, lambda k: _box(rng, k, (-0.4, -0.35, 0.45), (0.3, 0.35, 0.65)), P[0])
        add(1, lambda k: np.concatenate([_cyl(rng, k // 4 + (k % 4 if j == 0 else 0), (x, y, 0.12), 0.12, 0.06, axis=1)
                                         for j, (x, y) in enumerate([(-0.55, -0.38), (-0.55, 0.38), (0.55, -0.38), (0.55, 0.38)])]), P[1])
        add(3, lambda k: _box(rng, k, (-0.8, -0.35, 0.12), (0.5, 0.35, 0.45)), P[2])
        add(1, lambda k: _box(rng, k, (0.5, -0.35, 0.12), (0.9, 0.35, 0.35)), P[3])
    elif cat == 'Chair':                                 # back, seat, legs, arms
        h = u(0.4, 0.55)
        add(2, lambda k: _box(rng, k, (-0.3, 0.25, h), (0.3, 0.3, h + u(0.4, 0.6))), P[0])
        add(2, lambda k: _box(rng, k, (-0.3, -0.3, h - 0.05), (0.3, 0.3, h)), P[1])
        add(2, lambda k: np.concatenate([_cyl(rng, k // 4 + (k % 4 if j == 0 else 0), (x, y, (h - 0.05) / 2), 0.03, h - 0.05)
                                         for j, (x, y) in enumerate([(-0.27, -0.27), (-0.27, 0.27), (0.27, -0.27), (0.27, 0.27)])]), P[2])
        add(1, lambda k: np.concatenate([_box(rng, k // 2, (-0.32, -0.3, h + 0.2), (-0.28, 0.25, h + 0.24)),
                                         _box(rng, k - k // 2, (0.28, -0.3, h + 0.2), (0.32, 0.25, h + 0.24))]), P[3])
    elif cat == 'Earphone':                              # earcups, headband, cord
        add(2, lambda k: np.concatenate([_sphere(rng, k // 2, (-0.4, 0, 0), 0.15), _sphere(rng, k - k // 2, (0.4, 0, 0), 0.15)]), P[0])
        add(2, lambda k: (lambda t: np.stack([0.4 * np.cos(t), np.zeros(k), 0.5 * np.sin(t)], 1))(rng.uniform(0, np.pi, k)), P[1])
        add(1, lambda k: _cyl(rng, k, (-0.4, 0, -0.45), 0.015, 0.6), P[2])
    elif cat == 'Guitar':                                # head, neck, body
        add(1, lambda k: _box(rng, k, (-0.08, 1.0, -0.02), (0.08, 1.25, 0.02)), P[0])
        add(2, lambda k: _box(rng, k, (-0.04, 0.3, -0.02), (0.04, 1.0, 0.02)), P[1])
        add(4, lambda k: _sphere(rng, k, (0, 0, 0), 0.35, (1, 1, 0.2)), P[2])
    elif cat == 'Knife':                                 # blade, handle
        add(2, lambda k: _box(rng, k, (0, -0.06, -0.01), (u(0.8, 1.1), 0.06, 0.01)), P[0])
        add(1, lambda k: _cyl(rng, k, (-0.25, 0, 0), 0.05, 0.5, axis=0), P[1])
    elif cat == 'Lamp':                                  # base, pole, shade, bulb-holder
        add(1, lambda k: _disc(rng, k, (0, 0, 0), 0.3), P[0])
        add(1, lambda k: _cyl(rng, k, (0, 0, 0.5), 0.03, 1.0), P[1])
        add(2, lambda k: _cyl(rng, k, (0, 0, 1.1), 0.3, 0.3), P[2])
        add(1, lambda k: _sphere(rng, k, (0, 0, 0.98), 0.07), P[3])
    elif cat == 'Laptop':                                # keyboard, screen
        ang = u(1.2, 1.9)
        add(1, lambda k: _box(rng, k, (-0.5, 0, 0), (0.5, 0.7, 0.03)), P[0])
        add(1, lambda k: (lambda q: np.stack([q[:, 0], -q[:, 1] * np.cos(ang), q[:, 1] * np.sin(ang)], 1))(_box(rng, k, (-0.5, 0, 0), (0.5, 0.7, 0.02))), P[1])
    elif cat == 'Motorbike':                             # gas tank, seat, wheels, handle, light, frame
        add(1, lambda k: _sphere(rng, k, (0.2, 0, 0.55), 0.15, (1.5, 1, 0.8)), P[0])
        add(1, lambda k: _box(rng, k, (-0.4, -0.1, 0.55), (0.0, 0.1, 0.6)), P[1])
        add(3, lambda k: np.concatenate([_cyl(rng, k // 2, (-0.6, 0, 0.25), 0.25, 0.08, axis=1),
                                         _cyl(rng, k - k // 2, (0.6, 0, 0.25), 0.25, 0.08, axis=1)]), P[2])
        add(1, lambda k: _cyl(rng, k, (0.45, 0, 0.85), 0.02, 0.6, axis=1), P[3])
        add(1, lambda k: _sphere(rng, k, (0.65, 0, 0.7), 0.06), P[4])
        add(2, lambda k: _box(rng, k, (-0.6, -0.04, 0.25), (0.6, 0.04, 0.45)), P[5])
    elif cat == 'Mug':                                   # handle, body
        add(1, lambda k: (lambda t: np.stack([0.42 + 0.15 * np.cos(t), np.zeros(k), 0.45 + 0.2 * np.sin(t)], 1))(rng.uniform(-np.pi / 2, np.pi / 2, k)), P[0])
        add(4, lambda k: _cyl(rng, k, (0, 0, 0.45), 0.35, 0.9), P[1])
    elif cat == 'Pistol':                                # barrel, handle, trigger
        add(2, lambda k: _box(rng, k, (-0.1, -0.05, 0.3), (0.7, 0.05, 0.45)), P[0])
        add(2, lambda k: _box(rng, k, (-0.1, -0.05, -0.2), (0.1, 0.05, 0.3)), P[1])
        add(1, lambda k: _box(rng, k, (0.15, -0.02, 0.15), (0.25, 0.02, 0.3)), P[2])
    elif cat == 'Rocket':                                # body, fins, nose
        add(3, lambda k: _cyl(rng, k, (0, 0, 0.6), 0.15, 1.2), P[0])
        add(1, lambda k: np.concatenate([_box(rng, k // 2, (-0.4, -0.01, 0), (0.4, 0.01, 0.3)),
                                         _box(rng, k - k // 2, (-0.01, -0.4, 0), (0.01, 0.4, 0.3))]), P[1])
        add(1, lambda k: _sphere(rng, k, (0, 0, 1.2), 0.15, (1, 1, 2.5), upper=True), P[2])
    elif cat == 'Skateboard':                            # wheels, deck, trucks
        add(1, lambda k: np.concatenate([_cyl(rng, k // 4 + (k % 4 if j == 0 else 0), (x, y, 0.04), 0.04, 0.04, axis=1)
                                         for j, (x, y) in enumerate([(-0.35, -0.1), (-0.35, 0.1), (0.35, -0.1), (0.35, 0.1)])]), P[0])
        add(3, lambda k: _box(rng, k, (-0.5, -0.13, 0.12), (0.5, 0.13, 0.14)), P[1])
        add(1, lambda k: np.concatenate([_box(rng, k // 2, (-0.38, -0.1, 0.08), (-0.32, 0.1, 0.12)),
                                         _box(rng, k - k // 2, (0.32, -0.1, 0.08), (0.38, 0.1, 0.12))]), P[2])
    elif cat == 'Table':                                 # top, legs, support
        h = u(0.6, 0.8)
        add(3, lambda k: _box(rng, k, (-0.6, -0.4, h), (0.6, 0.4, h + 0.04)), P[0])
        add(2, lambda k: np.concatenate([_cyl(rng, k // 4 + (k % 4 if j == 0 else 0), (x, y, h / 2), 0.03, h)
                                         for j, (x, y) in enumerate([(-0.55, -0.35), (-0.55, 0.35), (0.55, -0.35), (0.55, 0.35)])]), P[1])
        add(1, lambda k: _box(rng, k, (-0.55, -0.02, 0.15), (0.55, 0.02, 0.2)), P[2])
    else:
        raise KeyError(cat)
    w = np.array([p[0] for p in prims], np.float64)
    counts = np.maximum(1, np.floor(w / w.sum() * n).astype(int))
    counts[np.argmax(counts)] += n - counts.sum()
    xyz = np.concatenate([fn(k) for (_, fn, _), k in zip(prims, counts)])
    lab = np.concatenate([np.full(k, l, np.int32) for (_, _, l), k in zip(prims, counts)])
    xyz = xyz * rng.uniform(0.85, 1.15, size=3) + rng.normal(0, 0.005, size=xyz.shape)
    perm = rng.permutation(n)
    return pc_normalize(xyz[perm]).astype(np.float32), lab[perm]


class SyntheticShapeNetPart(data.Dataset):
    """``shapes_per_category`` generated shapes of each of the 16 categories from ``seed`` (the test split from another stream), sampled like
    PartNormalDataset: items ``(points float32 [npoints, 3], cls int32 [1], seg int32 [npoints])``"""

    def __init__(self, split='trainval', npoints=2048, shapes_per_category=8, seed=0, points_per_shape=2048, rng=None):
        super().__init__()
        self.npoints = npoints
        gen = np.random.default_rng(seed + (0 if split in ('train', 'trainval') else 1000))
        self.points, self.cls, self.seg = [], [], []
        for ci, cat in enumerate(CATEGORIES):
            for _ in range(shapes_per_category):
                xyz, lab = synthetic_shape(cat, gen, points_per_shape)
                self.points.append(xyz)
                self.cls.append(np.array([ci], np.int32))
                self.seg.append(lab)
        self.seg_classes = seg_classes
        self.rng = rng if rng is not None else np.random.default_rng(seed + (17 if split in ('train', 'trainval') else 1017))

    def __getitem__(self, index):
        choice = self.rng.choice(len(self.seg[index]), self.npoints, replace=True)
        return self.points[index][choice], self.cls[index], self.seg[index][choice]

    def __len__(self):
        return len(self.points)
