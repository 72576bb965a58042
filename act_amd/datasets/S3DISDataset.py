"""S3DIS blocks for semantic segmentation (reference: semantic_segmentation/dataset.py:72-147) and a synthetic stand-in.

``S3DISDataset`` reads the reference's layout: ``Area_*`` room files (``.npy``, xyzrgbl, N x 7) under ``data_root``, split by ``test_area``,
labelweights (max(p) / p)^(1/3) over the split's label histogram, rooms drawn in proportion to their point count, a random 1 m x 1 m column
with more than 1024 points, ``num_point`` points drawn from it (with replacement when it has fewer), x / y centred on the block centre.
Items are ``(xyz [num_point, 3], labels [num_point])``.  The random stream is an injectable ``numpy.random.Generator``.

``SyntheticS3DIS`` generates rooms on the fly for machines without the data: labels are a deterministic function of local geometry
(floor, ceiling, walls, columns, a beam, windows and doors in the walls, and box-shaped furniture classes), all 13 ids.
"""
import os

import numpy as np
import torch.utils.data as data

CLASSES = ['ceiling', 'floor', 'wall', 'beam', 'column', 'window', 'door', 'table', 'chair', 'sofa', 'bookcase', 'board', 'clutter']
NUM_CLASSES = len(CLASSES)


def label_weights(labels_all):
    """(max(p) / p)^(1/3) of the label histogram over range(14) (dataset.py:96-110)"""
    hist = np.zeros(NUM_CLASSES)
    for lab in labels_all:
        tmp, _ = np.histogram(lab, range(NUM_CLASSES + 1))
        hist += tmp
    p = hist.astype(np.float32)
    p = p / np.sum(p)
    return np.power(np.amax(p) / p, 1 / 3.0)


def room_index(num_point_all, num_point, sample_rate=1.0):
    """room of every item: rooms in proportion to their point counts (dataset.py:111-117)"""
    num_point_all = np.asarray(num_point_all)
    sample_prob = num_point_all / np.sum(num_point_all)
    num_iter = int(np.sum(num_point_all) * sample_rate / num_point)
    idxs = []
    for index in range(len(num_point_all)):
        idxs.extend([index] * int(round(sample_prob[index] * num_iter)))
    return np.array(idxs)


def sample_block(points, labels, num_point, block_size, rng):
    """random block column with more than 1024 points, num_point points from it, x / y centred on the block centre (dataset.py:119-147)"""
    n = points.shape[0]
    while True:
        center = points[rng.choice(n)][:3]
        bmin = center - [block_size / 2.0, block_size / 2.0, 0]
        bmax = center + [block_size / 2.0, block_size / 2.0, 0]
        idx = np.where((points[:, 0] >= bmin[0]) & (points[:, 0] <= bmax[0]) & (points[:, 1] >= bmin[1]) & (points[:, 1] <= bmax[1]))[0]
        if idx.size > 1024:
            break
    sel = rng.choice(idx, num_point, replace=idx.size < num_point)
    xyz = points[sel, :3].copy()                                         # centred in the room file's dtype, as the reference does
    xyz[:, 0] -= center[0]
    xyz[:, 1] -= center[1]
    return xyz.astype(np.float32), labels[sel].astype(np.int64)


class S3DISDataset(data.Dataset):
    def __init__(self, split='train', data_root='trainval_fullarea', num_point=4096, test_area=5, block_size=1.0, sample_rate=1.0,
                 transform=None, rng=None):
        super().__init__()
        self.num_point, self.block_size, self.transform = num_point, block_size, transform
        self.rng = rng if rng is not None else np.random.default_rng()
        rooms = sorted(r for r in os.listdir(data_root) if 'Area_' in r)
        tag = 'Area_{}'.format(test_area)
        rooms = [r for r in rooms if (tag not in r) == (split == 'train')]
        self.rooms = rooms
        self.room_points, self.room_labels = [], []
        for name in rooms:
            d = np.load(os.path.join(data_root, name))                   # xyzrgbl, N x 7
            self.room_points.append(d[:, 0:6])
            self.room_labels.append(d[:, 6])
        self.labelweights = label_weights(self.room_labels)
        self.room_idxs = room_index([lab.size for lab in self.room_labels], num_point, sample_rate)

    def __getitem__(self, idx):
        r = self.room_idxs[idx]
        xyz, lab = sample_block(self.room_points[r], self.room_labels[r], self.num_point, self.block_size, self.rng)
        if self.transform is not None:
            xyz, lab = self.transform(xyz, lab)
        return xyz, lab

    def __len__(self):
        return len(self.room_idxs)


def synthetic_room(rng, n=60000):
    """one box-shaped room (xyzrgbl, n x 7): points on floor / ceiling / four walls plus a column, a beam and furniture boxes; each label
    follows from where the point lies (which surface, which box)"""
    W, D, H = rng.uniform(4.0, 7.0), rng.uniform(4.0, 7.0), rng.uniform(2.6, 3.2)
    parts = []

    def plane(axis, value, lo, hi, count, lab):
        p = rng.uniform(lo, hi, size=(count, 3))
        p[:, axis] = value + rng.normal(0, 0.005, count)
        parts.append((p, np.full(count, lab)))

    def box(lo, hi, count, lab):
        p = rng.uniform(lo, hi, size=(count, 3))
        face = rng.integers(0, 5, count)                                 # four sides + top
        for k in range(count):
            f = face[k]
            if f == 4:
                p[k, 2] = hi[2]
            else:
                ax = f // 2
                p[k, ax] = lo[ax] if f % 2 == 0 else hi[ax]
        parts.append((p, np.full(count, lab)))

    k = n // 20
    plane(2, 0.0, [0, 0, 0], [W, D, 0], 3 * k, 1)                        # floor
    plane(2, H, [0, 0, H], [W, D, H], 3 * k, 0)                          # ceiling
    for ax, v, span in ((0, 0.0, D), (0, W, D), (1, 0.0, W), (1, D, W)):
        p = rng.uniform([0, 0, 0], [W, D, H], size=(2 * k, 3))
        p[:, ax] = v + rng.normal(0, 0.005, 2 * k)
        t = p[:, 1 - ax]                                                 # position along the wall
        lab = np.full(2 * k, 2)
        lab[(t > 0.3 * span) & (t < 0.5 * span) & (p[:, 2] > 1.0) & (p[:, 2] < 2.0)] = 5      # window
        lab[(t > 0.7 * span) & (t < 0.85 * span) & (p[:, 2] < 2.1)] = 6                       # door
        lab[(t > 0.05 * span) & (t < 0.2 * span) & (p[:, 2] > 1.0) & (p[:, 2] < 1.8) & (lab == 2)] = 11   # board
        parts.append((p, lab))
    box([0.2, 0.2, 0], [0.5, 0.5, H], k, 4)                              # column
    box([0, D / 2 - 0.15, H - 0.4], [W, D / 2 + 0.15, H], k, 3)          # beam
    cx, cy = rng.uniform(1.5, W - 1.5), rng.uniform(1.5, D - 1.5)
    box([cx - 0.6, cy - 0.4, 0], [cx + 0.6, cy + 0.4, 0.75], k, 7)       # table
    box([cx + 0.8, cy - 0.25, 0], [cx + 1.3, cy + 0.25, 0.45], k, 8)     # chair
    box([0.8, D - 1.2, 0], [2.6, D - 0.3, 0.8], k, 9)                    # sofa
    box([W - 0.5, 1.0, 0], [W - 0.1, 2.5, 2.0], k, 10)                   # bookcase
    box([W - 1.6, D - 1.0, 0], [W - 1.0, D - 0.4, 0.3], k, 12)           # clutter
    xyz = np.concatenate([p for p, _ in parts]).astype(np.float32)
    lab = np.concatenate([l for _, l in parts]).astype(np.float32)
    rgb = np.zeros((xyz.shape[0], 3), np.float32)
    return np.concatenate([xyz, rgb, lab[:, None]], axis=1)


class SyntheticS3DIS(data.Dataset):
    """``num_rooms`` synthetic rooms from ``seed``, sampled into blocks exactly as S3DISDataset does (same labelweights / room index rules)"""

    def __init__(self, split='train', num_point=2048, num_rooms=8, seed=0, block_size=1.0, sample_rate=1.0, points_per_room=60000, rng=None):
        super().__init__()
        self.num_point, self.block_size = num_point, block_size
        gen = np.random.default_rng(seed + (0 if split == 'train' else 1000))
        rooms = [synthetic_room(gen, points_per_room) for _ in range(num_rooms)]
        self.room_points = [r[:, 0:6] for r in rooms]
        self.room_labels = [r[:, 6] for r in rooms]
        self.labelweights = label_weights(self.room_labels)
        self.room_idxs = room_index([lab.size for lab in self.room_labels], num_point, sample_rate)
        self.rng = rng if rng is not None else np.random.default_rng(seed + (17 if split == 'train' else 1017))

    def __getitem__(self, idx):
        r = self.room_idxs[idx]
        return sample_block(self.room_points[r], self.room_labels[r], self.num_point, self.block_size, self.rng)

    def __len__(self):
        return len(self.room_idxs)
