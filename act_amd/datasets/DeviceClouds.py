"""Object datasets resident on the device (csrc/cloud_sample.hip): the device twin of the ``__getitem__`` + DataLoader path of ShapeNet, ModelNet,
ModelNetFewShot and ScanObjectNN*.

A split stays on the device as one float32 [M,N,C] tensor (ShapeNet-55 ``whole``: 5.16 GB, ModelNet40 train: 0.97 GB).  A batch is one launch,
one workgroup per item: a keyed subset of ``npoints`` of the N rows without replacement in random order (the contract of the reference's
``permutation[:npoints]``) and numpy's ``pc_norm``, bit for bit.  Every draw is a function of (seed, epoch, dataset index), so a result does not
depend on the batch or the rank it is made in.  The draws are keyed hashes, not numpy's generator: a run is reproducible, but it is not
sample-for-sample the host loader's run.

``DeviceClouds.from_dataset`` reproduces each dataset's item rule and batch tuple; ``DeviceCloudLoader`` is the small iterable that
``tools/builder.dataset_builder`` returns in place of (sampler, DataLoader) for a dataset section with ``others.device_resident: True``."""
import os

import numpy as np
import torch

from .SyntheticDataset import read_points


def epoch_order(M, seed, epoch, shuffle=True, world_size=1):
    """the order of an epoch, the same on every rank: drawn on the host from default_rng((seed, epoch)) (the identity without ``shuffle``) and
    padded by wrapping to a multiple of ``world_size``, as DistributedSampler pads"""
    order = np.random.default_rng((int(seed), int(epoch))).permutation(M) if shuffle else np.arange(M)
    return np.resize(order, M + (-M % world_size)).astype(np.int64)


class DeviceClouds:
    """``clouds`` float32 [M,N,3|6] (xyz first), kept on ``device``.  A batch holds ``npoints`` rows per item: a keyed subset in random order
    with ``permute`` (else the first ``npoints`` rows), pc_norm'd with ``normalize``.  Without ``labels`` an epoch yields ShapeNet's
    ``(taxonomy ids, model ids, points)`` and ``names`` lists one (taxonomy id, model id) per item; with ``labels`` (one integer per item) it
    yields ``(names[0], names[1], (points, int64 labels on the device))`` and ``names`` is that pair (default ('ModelNet', 'sample'))."""

    def __init__(self, clouds, npoints, labels=None, names=None, permute=True, normalize=True, device="cuda"):
        from .. import kernels as K
        c = clouds if torch.is_tensor(clouds) else torch.from_numpy(np.ascontiguousarray(clouds))
        if c.dtype != torch.float32 or c.dim() != 3 or c.shape[2] not in (3, 6) or c.shape[0] < 1 or c.shape[1] < 1:
            raise ValueError(f"DeviceClouds: clouds must be float32 [M,N,3] or [M,N,6] with M, N > 0, got {c.dtype} {tuple(c.shape)}")
        self.npoints = int(npoints)
        if not 1 <= self.npoints <= min(c.shape[1], K.lib.act_cloud_sample_max_points()):
            raise ValueError(f"DeviceClouds: npoints must be in [1, min(N, {K.lib.act_cloud_sample_max_points()})], got {npoints} with N = {c.shape[1]}")
        self.device = torch.device(device)
        self.clouds = c.to(self.device).contiguous()
        if not bool(torch.isfinite(self.clouds).all()):
            raise ValueError("DeviceClouds: non-finite values in the clouds")
        M = self.clouds.shape[0]
        self.permute, self.normalize = bool(permute), bool(normalize)
        self.labels = None
        if labels is not None:
            lab = np.asarray(labels).reshape(-1)
            if lab.size != M:
                raise ValueError(f"DeviceClouds: {M} clouds but {lab.size} labels")
            self.labels = torch.from_numpy(lab.astype(np.int64)).to(self.device)
            self.names = tuple(names) if names is not None else ("ModelNet", "sample")
            if len(self.names) != 2:
                raise ValueError("DeviceClouds: with labels, names is the pair of strings that heads every batch tuple")
        else:
            self.names = [tuple(p) for p in names] if names is not None else [("", f"{i:06d}") for i in range(M)]
            if len(self.names) != M or any(len(p) != 2 for p in self.names):
                raise ValueError(f"DeviceClouds: names must list one (taxonomy id, model id) per cloud ({M})")

    def __len__(self):
        return self.clouds.shape[0]

    def resident_bytes(self):
        """bytes of the resident clouds and labels"""
        return sum(t.numel() * t.element_size() for t in (self.clouds, self.labels) if t is not None)

    def sample(self, item_ids, draw_ids, seed, epoch, want_rows=False, validate=True):
        """one launch -> points float32 [B,npoints,C] (and src_rows int32 [B,npoints] with ``want_rows``); item_ids / draw_ids int32 [B] on the device"""
        from .. import kernels as K
        with torch.cuda.device(self.clouds.device):                          # (a launch goes to the current device's current stream)
            return K.cloud_sample(self.clouds, item_ids, draw_ids, self.npoints, seed, epoch, self.permute, self.normalize, want_rows, validate)

    def epoch(self, batch_size, epoch, seed, shuffle=True, drop_last=True, rank=0, world_size=1):
        """iterator of the dataset's batch tuples, the points (and labels) on the device.  Rank ``rank`` takes order[rank::world_size] of
        epoch_order; the draw id of an item is its dataset index.  A subset that neither permutes, normalises nor drops rows is served as
        slices of the resident array when its indices are consecutive."""
        if int(batch_size) < 1 or not 0 <= int(rank) < int(world_size):
            raise ValueError("DeviceClouds.epoch: batch_size must be positive and 0 <= rank < world_size")
        ids = epoch_order(len(self), seed, epoch, shuffle, world_size)[rank::world_size]
        dev_ids = torch.from_numpy(ids.astype(np.int32)).to(self.device)
        plain = not self.permute and not self.normalize and self.npoints == self.clouds.shape[1]
        for s in range(0, len(ids), batch_size):
            e = min(s + batch_size, len(ids))
            if e - s < batch_size and drop_last:
                break
            if plain and np.all(np.diff(ids[s:e]) == 1):
                data = self.clouds[int(ids[s]):int(ids[s]) + e - s]           # (a view: evaluation reads it, nothing writes to it)
            else:
                data = self.sample(dev_ids[s:e], dev_ids[s:e], seed, epoch, validate=False)     # (the ids come from range(M))
            if self.labels is None:
                yield [self.names[i][0] for i in ids[s:e]], [self.names[i][1] for i in ids[s:e]], data
            else:
                yield self.names[0], self.names[1], (data, self.labels[dev_ids[s:e].long()])

    # ---- the datasets -----------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_dataset(cls, ds, device="cuda", cache=None):
        """the resident twin of a ShapeNet, ModelNet, ModelNetFewShot or ScanObjectNN* dataset.  ``cache`` (file-backed ShapeNet only): a .npy
        file that stores the packed [M,N,3] array, so a later run starts with one read."""
        kind = type(ds).__name__
        if kind == "ShapeNet":
            return cls._from_shapenet(ds, device, cache)
        if kind in ("ModelNet", "ModelNetFewShot"):
            return cls._from_modelnet(ds, device)
        if kind.startswith("ScanObjectNN"):
            train = ds.subset == "train"
            return cls(np.asarray(ds.points, dtype=np.float32), ds.points.shape[1], labels=ds.labels, names=("ScanObjectNN", "sample"),
                       permute=train, normalize=False, device=device)
        raise ValueError(f"DeviceClouds.from_dataset: no device twin for {kind}")

    @classmethod
    def _from_shapenet(cls, ds, device, cache):
        if ds.synthetic:                                                     # the generated items: already pc_norm'd, npoints rows each
            items = [ds[i] for i in range(len(ds))]
            clouds = np.stack([it[2].numpy() for it in items])
            return cls(clouds, ds.sample_points_num, names=[(it[0], it[1]) for it in items], device=device)
        names = [(f["taxonomy_id"], f["model_id"]) for f in ds.file_list]
        want = (len(ds.file_list), ds.npoints, 3)
        if cache is not None and os.path.exists(cache):
            clouds = np.load(cache)
            if clouds.shape != want or clouds.dtype != np.float32:
                raise ValueError(f"DeviceClouds: {cache} holds {clouds.dtype} {clouds.shape}, the file list needs float32 {want}")
        else:
            clouds = np.empty(want, np.float32)
            for i, f in enumerate(ds.file_list):
                path = os.path.join(ds.pc_path, f["file_path"])
                pc = read_points(path)
                if pc.shape != want[1:]:
                    raise ValueError(f"DeviceClouds: {path} holds a cloud of shape {pc.shape}, expected {want[1:]}")
                clouds[i] = pc
            if cache is not None:
                tmp = cache + ".tmp.npy"
                np.save(tmp, clouds)
                os.replace(tmp, cache)
        return cls(clouds, ds.sample_points_num, names=names, device=device)

    @classmethod
    def _from_modelnet(cls, ds, device):
        from .. import kernels as K
        train = ds.subset == "train"
        if getattr(ds, "synthetic", False):                                  # the generated items: already pc_norm'd
            items = [ds[i][2] for i in range(len(ds))]
            return cls(np.stack([p.numpy() for p, _ in items]), ds.npoints, labels=[l for _, l in items], permute=train, normalize=False,
                       device=device)
        if hasattr(ds, "list_of_points"):
            pts, labels = ds.list_of_points, [int(l[0]) for l in ds.list_of_labels]
        else:                                                                # ModelNetFewShot: (points, label, _) per item
            pts, labels = [p for p, _, _ in ds.dataset], [int(l) for _, l, _ in ds.dataset]
        shapes = {np.shape(p) for p in pts}
        if len(shapes) != 1:
            raise ValueError(f"DeviceClouds: the clouds of a resident split must have one shape, got {sorted(shapes)}")
        clouds = np.stack([np.asarray(p, dtype=np.float32) for p in pts])
        if not ds.use_normals:
            clouds = clouds[:, :, 0:3]
        dc = cls(clouds, clouds.shape[1], labels=labels, permute=train, normalize=False, device=device)
        # pc_norm once, before any shuffle (the reference's order), by the sampling kernel without a permutation
        ids = torch.arange(len(dc), dtype=torch.int32, device=dc.device)
        with torch.cuda.device(dc.device):
            for s in range(0, len(dc), 1024):
                dc.clouds[s:s + 1024] = K.cloud_sample(dc.clouds, ids[s:s + 1024], ids[s:s + 1024], dc.npoints, 0, 0, permute=False,
                                                       normalize=True, validate=False)
        return dc


class DeviceCloudLoader:
    """what the runners iterate in place of a DataLoader, and call ``set_epoch`` on in place of a DistributedSampler.  Without ``set_epoch``
    an internal counter gives every ``__iter__`` the next epoch."""

    def __init__(self, clouds, batch_size, shuffle, drop_last, seed=0, rank=0, world_size=1):
        self.dataset, self.batch_size, self.shuffle, self.drop_last = clouds, int(batch_size), bool(shuffle), bool(drop_last)
        self.seed, self.rank, self.world_size = int(seed), int(rank), int(world_size)
        self._epoch, self._count = None, 0

    def set_epoch(self, epoch):
        self._epoch = int(epoch)

    def __len__(self):
        n = -(-len(self.dataset) // self.world_size)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        epoch = self._epoch if self._epoch is not None else self._count
        self._count += 1
        return self.dataset.epoch(self.batch_size, epoch, self.seed, self.shuffle, self.drop_last, self.rank, self.world_size)
