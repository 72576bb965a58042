"""S3DIS training blocks sampled on the device from resident rooms (csrc/s3dis_sample.hip): the device twin of ``S3DISDataset.sample_block``.

All rooms of a split live on the device as one float64 ``[P_total, 3]`` tensor (float32 rooms are promoted, which is exact) with int32 labels.
Every room is indexed once by a uniform 2-D grid of square cells of side ``block_size / 4`` (``build_index``), stored as a CSR, and a whole batch of
blocks comes out of one launch that reads only the cells a column overlaps.  Membership, the ``> min_points`` rule and the two selection rules
are ``sample_block``'s; the draws are keyed hashes of ``(seed, epoch, item id, attempt)``, not ``np.random``'s, and there are at most
``max_tries`` attempts (then the fullest column seen is taken and ``info`` says so).
"""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from .S3DISDataset import room_index

CELLS_PER_BLOCK = 4
MAX_ROOM_CELLS = 1 << 24
# cell(hi) - cell(lo) of a window [c - bs/2, c + bs/2]: (hi - o) / cell - (lo - o) / cell is CELLS_PER_BLOCK up to rounding, far below one cell, so
# the two floors differ by at most CELLS_PER_BLOCK + 1 and a window overlaps at most CELLS_PER_BLOCK + 2 cells per axis (clamping only narrows it)
WINDOW_CELLS = CELLS_PER_BLOCK + 2

S3DISSample = namedtuple("S3DISSample", "xyz labels rows count center_idx info")


def cell_of(v, origin, cell, g):
    """clamp(floor((v - origin) / cell), 0, g - 1) in float64 (a float64 tensor -> int64): monotone non-decreasing in v"""
    return torch.floor((v - origin) / cell).clamp_(0, g - 1).to(torch.int64)


def build_index(xyz, room_off, block_size=1.0):
    """grid index of rooms stored back to back.  xyz float64 [P_total, 3] (CPU or device tensor), room_off: R + 1 increasing ints.
    -> namespace(xyz, room_off int64 [R+1], grid_origin float64 [R,2] (min x, min y of the room), grid_dims int64 [R,3] (gx, gy, the room's first
    cell in cell_off), cell_off int64 [cells+1], cell_pts int32 [P_total] (point index within the room: cell iy*gx + ix of a room owns
    cell_pts[cell_off[k]:cell_off[k+1]], ascending), cell, block_size, max_window (the most points any WINDOW_CELLS x WINDOW_CELLS window of
    cells of one room holds: an upper bound of every column's candidates))"""
    if xyz.dtype != torch.float64 or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("build_index: xyz must be float64 [P, 3]")
    room_off = [int(v) for v in room_off]
    if len(room_off) < 2 or room_off[0] != 0 or room_off[-1] != xyz.shape[0] or any(b <= a for a, b in zip(room_off, room_off[1:])):
        raise ValueError("build_index: room_off must run from 0 to P in increasing steps (no empty room)")
    if any(b - a > (1 << 31) - 1 for a, b in zip(room_off, room_off[1:])):
        raise ValueError("build_index: a room has more than 2^31 - 1 points")
    if not block_size > 0:
        raise ValueError("build_index: block_size must be positive")
    cell = float(block_size) / CELLS_PER_BLOCK
    dev = xyz.device
    origins, dims, offs, pts, wmax, base = [], [], [], [], [], 0
    for a, b in zip(room_off, room_off[1:]):
        xy = xyz[a:b, :2]
        lo, hi = xy.min(dim=0).values, xy.max(dim=0).values
        if not bool(torch.isfinite(lo).all() and torch.isfinite(hi).all()):
            raise ValueError("build_index: non-finite coordinates")
        g = torch.floor((hi - lo) / cell).to(torch.int64) + 1
        gx, gy = int(g[0]), int(g[1])
        if gx * gy > MAX_ROOM_CELLS:
            raise ValueError(f"build_index: a room of {gx} x {gy} cells of {cell} m (outlier points?)")
        key = cell_of(xy[:, 1], lo[1], cell, gy) * gx + cell_of(xy[:, 0], lo[0], cell, gx)
        order = torch.sort(key, stable=True).indices                          # stable: ascending point index inside a cell
        counts = torch.bincount(key, minlength=gx * gy)
        grid = torch.nn.functional.pad(counts.view(gy, gx), (1, WINDOW_CELLS - 1, 1, WINDOW_CELLS - 1)).cumsum(0).cumsum(1)
        W = WINDOW_CELLS
        wmax.append((grid[W:, W:] - grid[:-W, W:] - grid[W:, :-W] + grid[:-W, :-W]).max())
        origins.append(lo)
        dims.append((gx, gy, base))
        offs.append(counts.cumsum(0) - counts + a)                            # exclusive offsets, shifted to the room's place in cell_pts
        pts.append(order.to(torch.int32))
        base += gx * gy
    cell_off = torch.cat(offs + [torch.full((1,), room_off[-1], dtype=torch.int64, device=dev)])
    return SimpleNamespace(xyz=xyz, room_off=torch.tensor(room_off, dtype=torch.int64, device=dev), grid_origin=torch.stack(origins),
                           grid_dims=torch.tensor(dims, dtype=torch.int64, device=dev), cell_off=cell_off, cell_pts=torch.cat(pts), cell=cell,
                           block_size=float(block_size), max_window=int(torch.stack(wmax).max()))


class DeviceS3DISBlocks:
    """resident rooms + grid index + the sampler.  ``room_points``: one array [P_r, >= 3] per room (xyz first; float32 or float64),
    ``room_labels``: one array [P_r] per room."""

    def __init__(self, room_points, room_labels, num_point, block_size=1.0, min_points=1024, max_tries=64, device="cuda", labelweights=None,
                 room_idxs=None):
        if len(room_points) == 0 or len(room_points) != len(room_labels):
            raise ValueError("DeviceS3DISBlocks: one label array per room, at least one room")
        if int(num_point) <= 0 or int(max_tries) <= 0 or int(min_points) < 0:
            raise ValueError("DeviceS3DISBlocks: num_point and max_tries must be positive, min_points >= 0")
        xyz = []
        for p, l in zip(room_points, room_labels):
            p = np.asarray(p)
            if p.ndim != 2 or p.shape[1] < 3 or p.shape[0] == 0 or np.asarray(l).shape != (p.shape[0],):
                raise ValueError("DeviceS3DISBlocks: a room is [P, >= 3] points with [P] labels, P > 0")
            p = p[:, :3].astype(np.float64)
            if not np.isfinite(p).all():
                raise ValueError("DeviceS3DISBlocks: non-finite coordinates in a room")
            xyz.append(p)
        self.num_point, self.block_size, self.min_points, self.max_tries = int(num_point), float(block_size), int(min_points), int(max_tries)
        self.device = torch.device(device)
        sizes = [p.shape[0] for p in xyz]
        room_off = np.concatenate([[0], np.cumsum(sizes)])
        self.index = build_index(torch.from_numpy(np.concatenate(xyz)).to(self.device), room_off, block_size)
        self.index.labels = torch.from_numpy(np.concatenate([np.asarray(l).astype(np.int32) for l in room_labels])).to(self.device)
        self.index.min_points, self.index.max_tries = self.min_points, self.max_tries
        self.labelweights = labelweights
        self.room_idxs = np.asarray(room_idxs if room_idxs is not None else room_index(sizes, num_point), dtype=np.int64)
        if self.room_idxs.size and (self.room_idxs.min() < 0 or self.room_idxs.max() >= len(sizes)):
            raise ValueError("DeviceS3DISBlocks: room_idxs names a room that is not there")
        self._ws = None

    @classmethod
    def from_dataset(cls, ds, device="cuda", min_points=1024, max_tries=64):
        """the rooms, label weights and room proportions of an S3DISDataset / SyntheticS3DIS"""
        return cls(ds.room_points, ds.room_labels, ds.num_point, ds.block_size, min_points, max_tries, device, labelweights=ds.labelweights,
                   room_idxs=ds.room_idxs)

    def __len__(self):
        return len(self.room_idxs)

    def resident_bytes(self):
        """-> (bytes of the rooms: xyz + labels, bytes of the grid index)"""
        ix = self.index
        nbytes = lambda *ts: sum(t.numel() * t.element_size() for t in ts)
        return nbytes(ix.xyz, ix.labels), nbytes(ix.room_off, ix.grid_origin, ix.grid_dims, ix.cell_off, ix.cell_pts)

    def sample(self, room_ids, item_ids, seed, epoch, center_idx=None, validate=True):
        """one launch -> S3DISSample(xyz float32 [B,num_point,3], labels int64 [B,num_point], rows int32 [B,num_point] (point index within the
        room), count, center_idx, info int32 [B]); room_ids / item_ids (/ center_idx) int32 [B] on the device"""
        from .. import kernels as K
        B = room_ids.numel() if torch.is_tensor(room_ids) else 0
        if B > 0 and (self._ws is None or self._ws.numel() < B * self.index.max_window):
            self._ws = K.s3dis_sample_workspace(self.index, B)
        return S3DISSample(*K.s3dis_sample(self.index, room_ids, item_ids, self.num_point, seed, epoch, center_idx, self._ws, validate))

    def epoch(self, batch_size, epoch, seed, shuffle=True, drop_last=True):
        """iterator of (pts float32 [B, num_point, 3], target int64 [B, num_point]) on the device.  The order is a permutation of room_idxs drawn
        on the host from default_rng((seed, epoch)) and uploaded once; item ids are the positions in it; batches slice it on the device."""
        n = len(self.room_idxs)
        order = np.random.default_rng((int(seed), int(epoch))).permutation(n) if shuffle else np.arange(n)
        rooms = torch.from_numpy(self.room_idxs[order].astype(np.int32)).to(self.device)
        items = torch.arange(n, dtype=torch.int32, device=self.device)
        for s in range(0, n, batch_size):
            e = min(s + batch_size, n)
            if e - s < batch_size and drop_last:
                break
            out = self.sample(rooms[s:e], items[s:e], seed, epoch, validate=False)      # (room_idxs was checked at construction)
            yield out.xyz, out.labels
