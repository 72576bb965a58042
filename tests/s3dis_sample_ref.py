"""numpy restatement of the device S3DIS block sampler (csrc/s3dis_sample.hip, act_amd/datasets/S3DISDevice.py) and the rooms its tests use:
the cell function, the member order, the 64-bit centre draw, the attempts, the accept / fallback rule and both selections."""
import numpy as np

M32 = 0xFFFFFFFF


# ---- the keyed draws (csrc/ws_hash.h), as tests/test_gpu_wholescene.py restates them ------------------------------------------------------------
def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def feistel(x, n, key):
    x = np.asarray(x, dtype=np.uint64).copy()
    if n <= 1:
        return np.zeros_like(x)
    bits = max(2, int(n - 1).bit_length())
    bits += bits & 1
    h = bits // 2
    mask = np.uint64((1 << h) - 1)
    todo = np.ones(x.shape, bool)
    while todo.any():
        L, R = x[todo] >> np.uint64(h), x[todo] & mask
        for i in range(4):
            F = mix32(R ^ mix32((int(key) + i * 0x9e3779b9) & M32)) & mask
            L, R = R, L ^ F
        x[todo] = (L << np.uint64(h)) | R
        todo = x >= n
    return x


def item_key(seed, epoch, item):
    k = int(mix32((seed & M32) ^ 0x13198a2e))
    k = int(mix32(k ^ (epoch & M32)))
    return int(mix32(k ^ (item & M32)))


def center_draw(k0, t, P):
    """attempt t's centre: a 64-bit hash h, point hi64(h * P)"""
    ka = int(mix32(k0 ^ int(mix32(t ^ 0x85a308d3))))
    h = (int(mix32(ka ^ 1)) << 32) | int(mix32(ka ^ 2))
    return (h * P) >> 64


# ---- rooms ------------------------------------------------------------------------------------------------------------------------------------------
def _lattice(ox, oy, nx, ny, nz, step, seed):
    x, y, z = np.meshgrid(ox + np.arange(nx) * step, oy + np.arange(ny) * step, np.arange(nz) * 0.25, indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float64)
    return p[np.random.default_rng(seed).permutation(p.shape[0])]            # point order is not grid order


def _labels(n):
    return ((np.arange(n) * 7 + 3) % 13).astype(np.int32)


def room_a():
    """12,936 points: x in {0, 1/16, ..., 3}, y in {0, ..., 2}, 8 levels; column counts 648 .. 2,312"""
    p = _lattice(0.0, 0.0, 49, 33, 8, 1 / 16, 1)
    return p, _labels(p.shape[0])


def room_b():
    """13,680 points: origin (-3.25, 10.5), 40 x 57 columns at 1/16, 6 levels; column counts 486 .. 1,734"""
    p = _lattice(-3.25, 10.5, 40, 57, 6, 1 / 16, 2)
    return p, _labels(p.shape[0])


def room_c():
    """600 points, 25 x 6 columns at 1/8, 4 levels: every column holds at most 216"""
    p = _lattice(0.0, 0.0, 25, 6, 4, 1 / 8, 3)
    return p, _labels(p.shape[0])


def room_d():
    """1,500 points inside 0.1 m, every coordinate twice: one cell, count = P"""
    q = np.random.default_rng(4).uniform(0.0, 0.1, size=(750, 3)) + [5.0, -2.0, 0.0]
    p = np.concatenate([q, q])[np.random.default_rng(5).permutation(1500)]
    return p, _labels(1500)


def room_e():
    """50,000 uniform random float64 points of a 6 x 5 x 3 m box"""
    p = np.random.default_rng(6).uniform([-1.0, 2.0, 0.0], [5.0, 7.0, 3.0], size=(50000, 3))
    return p, _labels(50000)


# ---- the sampler --------------------------------------------------------------------------------------------------------------------------------
def cell_of(v, origin, cell, g):
    return np.clip(np.floor((np.asarray(v, np.float64) - origin) / cell), 0, g - 1).astype(np.int64)


class RefSampler:
    """rooms: list of (points [P, 3], labels [P]); float32 rooms are promoted to float64 (exact)"""

    def __init__(self, rooms, num_point, block_size=1.0, min_points=1024, max_tries=64):
        self.pts = [np.asarray(p)[:, :3].astype(np.float64) for p, _ in rooms]
        self.lab = [np.asarray(l).astype(np.int64) for _, l in rooms]
        self.num_point, self.half, self.cell, self.min_points, self.max_tries = num_point, block_size / 2.0, block_size / 4.0, min_points, max_tries
        self.origin = [p[:, :2].min(axis=0) for p in self.pts]
        self.dims = [(np.floor((p[:, :2].max(axis=0) - o) / self.cell).astype(np.int64) + 1) for p, o in zip(self.pts, self.origin)]

    def cells(self, room):
        """cell iy * gx + ix of every point of the room"""
        p, o, (gx, gy) = self.pts[room], self.origin[room], self.dims[room]
        return cell_of(p[:, 1], o[1], self.cell, gy) * gx + cell_of(p[:, 0], o[0], self.cell, gx)

    def window(self, room, ci):
        """the overlapped cell range of the column of centre point ci: (ix0, ix1, iy0, iy1)"""
        p, o, (gx, gy) = self.pts[room], self.origin[room], self.dims[room]
        cx, cy = p[ci, 0], p[ci, 1]
        return (int(cell_of(cx - self.half, o[0], self.cell, gx)), int(cell_of(cx + self.half, o[0], self.cell, gx)),
                int(cell_of(cy - self.half, o[1], self.cell, gy)), int(cell_of(cy + self.half, o[1], self.cell, gy)))

    def members(self, room, ci):
        """np.where of the column, listed cell by cell (row-major), ascending point index inside a cell"""
        p = self.pts[room]
        cx, cy = p[ci, 0], p[ci, 1]
        idx = np.where((p[:, 0] >= cx - self.half) & (p[:, 0] <= cx + self.half) & (p[:, 1] >= cy - self.half) & (p[:, 1] <= cy + self.half))[0]
        return idx[np.argsort(self.cells(room)[idx], kind="stable")]

    def select(self, k0, count):
        """positions of the member list taken by outputs 0 .. num_point - 1"""
        j = np.arange(self.num_point)
        if count >= self.num_point:
            return feistel(j, count, int(mix32(k0 ^ 0x03707344))).astype(np.int64)
        h = mix32(mix32(j) ^ mix32(k0 ^ 0xa4093822))
        return ((h * np.uint64(count)) >> np.uint64(32)).astype(np.int64)

    def item(self, room, item, seed, epoch, center_idx=None):
        """-> dict(center_idx, info, count, rows, xyz, labels, members, counts (of every attempt made))"""
        P, k0 = self.pts[room].shape[0], item_key(seed, epoch, item)
        counts = []
        if center_idx is not None:
            ci, info = int(center_idx), 1
            mem = self.members(room, ci)
        else:
            for t in range(self.max_tries):
                ci = center_draw(k0, t, P)
                mem = self.members(room, ci)
                counts.append(mem.size)
                if mem.size > self.min_points:
                    info = t + 1
                    break
            else:
                t = int(np.argmax(counts))                                   # the largest count, the earliest on ties
                ci, info = center_draw(k0, t, P), -self.max_tries
                mem = self.members(room, ci)
        rows = mem[self.select(k0, mem.size)]
        p = self.pts[room]
        xyz = np.stack([(p[rows, 0] - p[ci, 0]).astype(np.float32), (p[rows, 1] - p[ci, 1]).astype(np.float32), p[rows, 2].astype(np.float32)], axis=1)
        return dict(center_idx=ci, info=info, count=mem.size, rows=rows, xyz=xyz, labels=self.lab[room][rows], members=mem, counts=counts)
