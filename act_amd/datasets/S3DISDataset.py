"""S3DIS blocks for semantic segmentation (reference: semantic_segmentation/dataset.py:72-147) and a synthetic stand-in.

``S3DISDataset`` reads the reference's layout: ``Area_*`` room files (``.npy``, xyzrgbl, N x 7) under ``data_root``, split by ``test_area``,
labelweights (max(p) / p)^(1/3) over the split's label histogram, rooms drawn in proportion to their point count, a random 1 m x 1 m column
with more than 1024 points, ``num_point`` points drawn from it (with replacement when it has fewer), x / y centred on the block centre.
Items are ``(xyz [num_point, 3], labels [num_point])``.  The random stream is an injectable ``numpy.random.Generator``.

``SyntheticS3DIS`` generates rooms on the fly for machines without the data: labels are a deterministic function of local geometry
(floor, ceiling, walls, columns, a beam, windows and doors in the walls, and box-shaped furniture classes), all 13 ids.

``S3DISWholeScene`` (alias ``ScannetDatasetWholeScene``, reference: dataset.py:150-235) tiles whole rooms with overlapping blocks for
main_test.py: the per-block thresholds / centres for the device path (``block_table``) and the reference's host ``__getitem__`` restated with an
injectable ``numpy.random.RandomState``.  ``SyntheticS3DISWholeScene`` writes synthetic rooms as ``Area_5_*.npy`` files and loads them.
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


class S3DISWholeScene:
    """whole rooms of ``test_area`` (split 'test') or of the other areas (split 'train'), as dataset.py ScannetDatasetWholeScene loads them:
    ``file_list`` in ``os.listdir`` order, ``scene_points_list`` (xyzrgb, the file's dtype), ``semantic_labels_list``, and ``labelweights``
    over the split ((max(p) / p)^(1/3), float32; a class absent from the split gets an infinite weight, whose rows never vote)."""

    def __init__(self, root, block_points=4096, split='test', test_area=5, stride=0.5, block_size=1.0, padding=0.001):
        self.block_points, self.block_size, self.padding, self.root, self.split, self.stride = block_points, block_size, padding, root, split, stride
        assert split in ['train', 'test']
        tag = 'Area_%d' % test_area
        self.file_list = [d for d in os.listdir(root) if (d.find(tag) == -1) == (split == 'train')]
        self.scene_points_list, self.semantic_labels_list, self.scene_points_num = [], [], []
        for file in self.file_list:
            data = np.load(os.path.join(root, file))
            self.scene_points_list.append(data[:, :6])
            self.semantic_labels_list.append(data[:, 6])
            self.scene_points_num.append(data.shape[0])
        with np.errstate(divide='ignore'):
            self.labelweights = label_weights(self.semantic_labels_list)

    def __len__(self):
        return len(self.scene_points_list)

    def scene_name(self, index):
        return self.file_list[index][:-4]

    def _grid(self, index):
        points = self.scene_points_list[index]
        coord_min, coord_max = np.amin(points, axis=0)[:3], np.amax(points, axis=0)[:3]
        grid_x = int(np.ceil(float(coord_max[0] - coord_min[0] - self.block_size) / self.stride) + 1)
        grid_y = int(np.ceil(float(coord_max[1] - coord_min[1] - self.block_size) / self.stride) + 1)
        if grid_x <= 0 or grid_y <= 0:
            raise ValueError(f"room {self.file_list[index]} is too narrow for a {self.block_size} m block at stride {self.stride} "
                             f"(extent {float(coord_max[0] - coord_min[0]):.3f} x {float(coord_max[1] - coord_min[1]):.3f}): no block to test")
        return coord_min, coord_max, grid_x, grid_y

    def _bounds(self, coord_min, coord_max, index_x, index_y):
        """the reference's block expressions, in the room file's dtype (NumPy 2 scalar promotion: float32 stays float32)"""
        s_x = coord_min[0] + index_x * self.stride
        e_x = min(s_x + self.block_size, coord_max[0])
        s_x = e_x - self.block_size
        s_y = coord_min[1] + index_y * self.stride
        e_y = min(s_y + self.block_size, coord_max[1])
        s_y = e_y - self.block_size
        return (s_x - self.padding, e_x + self.padding, s_y - self.padding, e_y + self.padding,
                s_x + self.block_size / 2.0, s_y + self.block_size / 2.0)

    def block_table(self, index):
        """-> (table float64 [grid_y * grid_x, 6] = lo_x, hi_x, lo_y, hi_y, cx, cy of block index_y * grid_x + index_x, grid_x, grid_y).
        Every entry is formed in the file's dtype and widened exactly, so float64 comparisons on the device equal the reference's."""
        coord_min, coord_max, grid_x, grid_y = self._grid(index)
        table = np.array([[float(v) for v in self._bounds(coord_min, coord_max, ix, iy)] for iy in range(grid_y) for ix in range(grid_x)],
                         dtype=np.float64)
        return table, grid_x, grid_y

    def __getitem__(self, index, rng=None):
        """dataset.py:186-235 with np.random replaced by ``rng`` (a numpy.random.RandomState: ``RandomState(s)`` draws what ``np.random.seed(s)``
        does) -> (data_room [blocks, block_points, 9], label_room, sample_weight, index_room [blocks, block_points])"""
        rng = np.random if rng is None else rng
        points = self.scene_points_list[index]
        labels = self.semantic_labels_list[index]
        coord_min, coord_max, grid_x, grid_y = self._grid(index)
        data_room, label_room, sample_weight, index_room = [], [], [], []
        for index_y in range(0, grid_y):
            for index_x in range(0, grid_x):
                lo_x, hi_x, lo_y, hi_y, cx, cy = self._bounds(coord_min, coord_max, index_x, index_y)
                point_idxs = np.where((points[:, 0] >= lo_x) & (points[:, 0] <= hi_x) & (points[:, 1] >= lo_y) & (points[:, 1] <= hi_y))[0]
                if point_idxs.size == 0:
                    continue
                num_batch = int(np.ceil(point_idxs.size / self.block_points))
                point_size = int(num_batch * self.block_points)
                replace = False if (point_size - point_idxs.size <= point_idxs.size) else True
                point_idxs_repeat = rng.choice(point_idxs, point_size - point_idxs.size, replace=replace)
                point_idxs = np.concatenate((point_idxs, point_idxs_repeat))
                rng.shuffle(point_idxs)
                data_batch = points[point_idxs, :]
                normlized_xyz = np.zeros((point_size, 3))
                normlized_xyz[:, 0] = data_batch[:, 0] / coord_max[0]
                normlized_xyz[:, 1] = data_batch[:, 1] / coord_max[1]
                normlized_xyz[:, 2] = data_batch[:, 2] / coord_max[2]
                data_batch[:, 0] = data_batch[:, 0] - cx
                data_batch[:, 1] = data_batch[:, 1] - cy
                data_batch[:, 3:6] /= 255.0
                data_room.append(np.concatenate((data_batch, normlized_xyz), axis=1))
                label_batch = labels[point_idxs].astype(int)
                label_room.append(label_batch)
                sample_weight.append(self.labelweights[label_batch].astype(np.float64))   # the reference hstacks onto a float64 []
                index_room.append(point_idxs)
        data_room = np.concatenate(data_room)
        return (data_room.reshape((-1, self.block_points, data_room.shape[1])), np.concatenate(label_room).reshape((-1, self.block_points)),
                np.concatenate(sample_weight).reshape((-1, self.block_points)), np.concatenate(index_room).reshape((-1, self.block_points)))


ScannetDatasetWholeScene = S3DISWholeScene


def write_synthetic_rooms(root, num_rooms=8, seed=0, points_per_room=60000, test_area=5):
    """``num_rooms`` synthetic rooms of SyntheticS3DIS's test split (the same generator, held out from its training rooms) written as
    ``Area_<test_area>_synthetic_<i>.npy`` (xyzrgbl float32) under ``root``; -> the file names"""
    os.makedirs(root, exist_ok=True)
    gen = np.random.default_rng(seed + 1000)
    names = []
    for i in range(num_rooms):
        name = 'Area_%d_synthetic_%d.npy' % (test_area, i)
        np.save(os.path.join(root, name), synthetic_room(gen, points_per_room))
        names.append(name)
    return names


class SyntheticS3DISWholeScene(S3DISWholeScene):
    """write_synthetic_rooms into ``root``, then load them as S3DISWholeScene does"""

    def __init__(self, root, block_points=4096, num_rooms=8, seed=0, points_per_room=60000, test_area=5, **kw):
        write_synthetic_rooms(root, num_rooms, seed, points_per_room, test_area)
        super().__init__(root, block_points, 'test', test_area, **kw)
