"""numpy restatement of the device object-dataset sampler (csrc/cloud_sample.hip, act_amd/datasets/DeviceClouds.py): the key of a draw, the
keyed subset, pc_norm in the kernel's (numpy's) order of operations, the epoch order and its shards."""
import numpy as np

from tests.s3dis_sample_ref import M32, mix32, feistel          # csrc/ws_hash.h, restated once

SALT = 0x299f31d0
PERMUTE, NORMALIZE = 1, 2
MAX_POINTS = 8192


def draw_key(seed, epoch, draw_id):
    k = int(mix32((seed & M32) ^ SALT))
    k = int(mix32(k ^ (epoch & M32)))
    return int(mix32(k ^ (draw_id & M32)))


def subset_rows(N, n, seed, epoch, draw_id, permute=True):
    """source rows of positions 0 .. n-1: n distinct rows of [0, N) in keyed random order, or 0 .. n-1"""
    j = np.arange(n)
    return feistel(j, N, draw_key(seed, epoch, draw_id)).astype(np.int64) if permute else j.astype(np.int64)


def pc_norm_serial(pc):
    """pc float32 [n,3] -> pc_norm(pc), every operation spelled out in fp32: column sums one row at a time in ascending order, / float32(n),
    subtract, the largest sqrt((x*x + y*y) + z*z), divide (0 / 0 -> NaN)"""
    pc = np.ascontiguousarray(pc, dtype=np.float32)
    s = np.zeros(3, np.float32)
    for row in pc:
        s = s + row
    c = pc - s / np.float32(pc.shape[0])
    d = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        return c / d.max()


def sample(clouds, item, draw_id, n, seed, epoch, flags=PERMUTE | NORMALIZE):
    """-> (out float32 [n,C], src_rows int64 [n]) of one item of clouds float32 [M,N,C]"""
    cloud = np.asarray(clouds[item], dtype=np.float32)
    rows = subset_rows(cloud.shape[0], n, seed, epoch, draw_id, bool(flags & PERMUTE))
    out = cloud[rows].copy()
    if flags & NORMALIZE:
        out[:, 0:3] = pc_norm_serial(out[:, 0:3])
    return out, rows


def epoch_order(M, seed, epoch, shuffle=True, world_size=1):
    """the order of an epoch, the same on every rank: a permutation from default_rng((seed, epoch)) (the identity without shuffle), padded by
    wrapping to a multiple of world_size"""
    order = np.random.default_rng((int(seed), int(epoch))).permutation(M) if shuffle else np.arange(M)
    return np.resize(order, M + (-M % world_size)).astype(np.int64)          # (np.resize repeats the array from its start)


def shard(order, rank, world_size):
    return order[rank::world_size]


def batches(ids, batch_size, drop_last):
    out = [ids[s:s + batch_size] for s in range(0, len(ids), batch_size)]
    return [b for b in out if len(b) == batch_size or not drop_last]
