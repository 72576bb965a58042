"""GPU: whole-room sliding-window testing (csrc/wholescene.hip, act_amd/tools/runner_semseg_test.py) against np.where, a numpy restatement of
the keyed draws, the reference's recorded blocks (tests/golden/g20_wholescene.npz) and main_test.py's add_vote / argmax / metrics."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import golden, ROOT
from tests.golden.fill import fill_module

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- numpy restatement of the keyed draws (csrc/wholescene.hip) -----------------------------------------------------------------------------
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


def rows_ref(members, moff, bid, roff, seed, room, vote):
    out = np.empty(int(roff[-1]), np.int64)
    for s, b in enumerate(bid):
        cnt, ps = int(moff[b + 1] - moff[b]), int(roff[s + 1] - roff[s])
        pad = ps - cnt
        k = mix32(seed ^ 0x243f6a88)
        k = mix32(k ^ np.uint64(room))
        k = mix32(k ^ np.uint64(vote))
        k = mix32(k ^ np.uint64(b))
        i = feistel(np.arange(ps), ps, int(mix32(k ^ np.uint64(1))))
        m = i.copy()
        f = i >= cnt
        if pad <= cnt:
            m[f] = feistel(i[f] - cnt, cnt, int(mix32(k ^ np.uint64(2))))
        else:
            h = mix32(mix32(i[f] - cnt) ^ mix32(k ^ np.uint64(3)))
            m[f] = (h * np.uint64(cnt)) >> np.uint64(32)
        out[roff[s]:roff[s + 1]] = members[moff[b] + m.astype(np.int64)]
    return out


def add_vote(pool, point_idx, pred_label, weight):
    """main_test.py add_vote, as written"""
    B, N = pred_label.shape
    for b in range(B):
        for n in range(N):
            if weight[b, n] != 0 and not np.isinf(weight[b, n]):
                pool[int(point_idx[b, n]), int(pred_label[b, n])] += 1
    return pool


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------------
def _golden_ds(tmp_path):
    from act_amd.datasets.S3DISDataset import S3DISWholeScene
    g = golden("g20_wholescene")
    root = tmp_path / "rooms"
    root.mkdir(exist_ok=True)
    for name in g["file_list"]:
        np.save(root / name, g["room_" + name[len("Area_5_room_"):-4]])
    return g, S3DISWholeScene(str(root), block_points=int(g["block_points"]))


def _members_host(xyz, tab, gx, gy):
    out = []
    for b in range(gx * gy):
        lo_x, hi_x, lo_y, hi_y = tab[b, :4]
        out.append(np.where((xyz[:, 0] >= lo_x) & (xyz[:, 0] <= hi_x) & (xyz[:, 1] >= lo_y) & (xyz[:, 1] <= hi_y))[0])
    return out


def _check_members(dev, xyz, tab, gx, gy):
    from act_amd import kernels as K
    x = torch.from_numpy(np.ascontiguousarray(xyz[:, :3], dtype=np.float64)).to(dev)
    t = torch.from_numpy(tab).to(dev)
    counts, off, mem = K.scene_members(x, t, gx, gy)
    counts2, off2, mem2 = K.scene_members(x, t, gx, gy)
    off, mem = off.cpu().numpy(), mem.cpu().numpy()
    assert np.array_equal(counts, counts2) and np.array_equal(off, off2.cpu().numpy()) and np.array_equal(mem, mem2.cpu().numpy())
    ref = _members_host(xyz[:, :3].astype(np.float64), tab, gx, gy)
    assert np.array_equal(counts, [r.size for r in ref])
    assert off[0] == 0 and np.array_equal(np.diff(off), counts)
    for b, r in enumerate(ref):
        assert np.array_equal(mem[off[b]:off[b + 1]], r), b
    return counts, off, mem


# ---- 1. membership -----------------------------------------------------------------------------------------------------------------------------
def test_membership_equals_np_where(dev, tmp_path):
    g, ds = _golden_ds(tmp_path)
    for i in range(len(ds)):
        tab, gx, gy = ds.block_table(i)
        _check_members(dev, ds.scene_points_list[i], tab, gx, gy)
    # a random 200k-point room, float32 file, 6.3 m x 4.1 m, with a coherent run and a shuffled tail
    from act_amd.datasets.S3DISDataset import S3DISWholeScene
    rs = np.random.RandomState(5)
    pts = np.zeros((200000, 7), np.float32)
    pts[:, :3] = rs.uniform([0.3, -2.0, 0], [6.6, 2.1, 3], size=(200000, 3))
    pts[:100000] = pts[:100000][np.argsort(pts[:100000, 0], kind="stable")]
    np.save(tmp_path / "Area_5_big.npy", pts)
    big = S3DISWholeScene(str(tmp_path), block_points=2048)
    i = big.file_list.index("Area_5_big.npy")
    tab, gx, gy = big.block_table(i)
    _check_members(dev, big.scene_points_list[i], tab, gx, gy)


# ---- 2. keyed index build -----------------------------------------------------------------------------------------------------------------------
def _layout(counts, bp):
    bid = np.nonzero(counts)[0]
    roff = np.concatenate([[0], np.cumsum((counts[bid] + bp - 1) // bp * bp)])
    return bid, roff


def test_keyed_rows_equal_numpy_restatement(dev):
    from act_amd import kernels as K
    rs = np.random.RandomState(7)
    counts = np.array([0, 1, 5, 31, 32, 33, 63, 64, 65, 100, 128, 200, 0, 7, 1000], np.int64)
    moff = np.concatenate([[0], np.cumsum(counts)])
    members = np.concatenate([np.sort(rs.choice(50000, c, replace=False)) for c in counts]).astype(np.int32)
    d = lambda a: torch.from_numpy(np.asarray(a, np.int32)).to(dev)
    for bp in (64, 65):                                                      # cnt 32: pad == cnt at 64, pad == cnt + 1 at 65
        bid, roff = _layout(counts, bp)
        for seed, room, vote in ((0, 0, 0), (3, 1, 2), (0xFFFFFFFF, 7, 1)):
            rows = K.scene_rows(d(members), d(moff), d(bid), d(roff), int(roff[-1]), bp, seed, room, vote).cpu().numpy()
            assert np.array_equal(rows, rows_ref(members, moff, bid, roff, seed, room, vote)), (bp, seed, room, vote)
            for s, b in enumerate(bid):
                blk = rows[roff[s]:roff[s + 1]]
                mem = members[moff[b]:moff[b + 1]]
                cnt, pad = mem.size, blk.size - mem.size
                u, c = np.unique(blk, return_counts=True)
                assert c.sum() == cnt + pad and np.all(np.isin(mem, u)) and np.all(np.isin(u, mem))   # every member, nothing else
                if pad <= cnt:
                    assert c.max() <= 2 and (c == 2).sum() == pad           # without replacement: pad distinct members twice
    bid, roff = _layout(counts, 64)
    r2 = K.scene_rows(d(members), d(moff), d(bid), d(roff), int(roff[-1]), 64, 1, 0, 0).cpu().numpy()
    r3 = K.scene_rows(d(members), d(moff), d(bid), d(roff), int(roff[-1]), 64, 1, 0, 1).cpu().numpy()
    assert not np.array_equal(r2, r3)                                        # another vote, other draws


def test_shuffle_is_a_permutation_for_every_size(dev):
    """block_points 1: point_size == cnt, no fill, so each block's rows are a keyed permutation of its members, sizes 1 .. 5000"""
    from act_amd import kernels as K
    n = np.arange(1, 5001, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(n)])
    d = lambda a: torch.from_numpy(np.asarray(a, np.int32)).to(dev)
    members = d(np.arange(off[-1]))
    rows = K.scene_rows(members, d(off), d(np.arange(n.size)), d(off), int(off[-1]), 1, 11, 0, 0).cpu().numpy().astype(np.int64)
    seg = np.repeat(np.arange(n.size), n)
    assert np.all(rows >= off[seg]) and np.all(rows < off[seg + 1])
    assert np.array_equal(np.sort(rows), np.arange(off[-1]))
    assert (rows != np.arange(off[-1])).mean() > 0.9


# ---- 3. gather with the reference's injected rows --------------------------------------------------------------------------------------------------
def test_gather_with_injected_rows_equals_reference_bit_for_bit(dev, tmp_path):
    from act_amd.tools.runner_semseg_test import Room
    from act_amd import kernels as K
    g, ds = _golden_ds(tmp_path)
    for name in g["file_list"]:
        tag = name[len("Area_5_room_"):-4]
        room = Room(ds, ds.file_list.index(name), dev)
        rows = torch.from_numpy(g["index_room_" + tag].reshape(-1)).to(dev)
        assert rows.numel() == room.R
        out = K.scene_gather(room.xyz, room.table, rows, room.block_ids, room.row_off).cpu().numpy()
        assert np.array_equal(out.view(np.int32), g["data_room_" + tag].reshape(-1, 3).view(np.int32)), tag


# ---- 4. vote ------------------------------------------------------------------------------------------------------------------------------------
def test_vote_equals_add_vote(dev):
    from act_amd import kernels as K
    rs = np.random.RandomState(9)
    P, C, bp = 300, 13, 32
    label = rs.randint(0, C, size=P)
    lw = (1 + rs.rand(C)).astype(np.float32)
    lw[3], lw[7] = 0.0, np.inf                                               # zero and infinite weight classes never vote
    votes = torch.zeros(P, C, dtype=torch.int32, device=dev)
    pool = np.zeros((P, C))
    lab_d = torch.from_numpy(label.astype(np.int32)).to(dev)
    lw_d = torch.from_numpy(lw).to(dev)
    for nb in (4, 4, 3):                                                     # the last batch is partial
        idx = rs.randint(0, P, size=(nb, bp))
        idx[0, :8] = idx[0, 8]                                               # duplicated rows vote once per occurrence
        logp = rs.standard_normal((nb, bp, C)).astype(np.float32)
        logp[0, :5, :] = logp[0, :5, 2:3]                                    # all tied: class 0
        logp[1, :5, 4] = logp[1, :5, 9] = 10.0                               # tied maxima: the lower class
        K.scene_vote(torch.from_numpy(logp).to(dev), torch.from_numpy(idx.astype(np.int32)).to(dev), lab_d, lw_d, votes)
        pred = torch.from_numpy(logp).max(2)[1].numpy()                     # CPU torch, as main_test.py takes it
        pool = add_vote(pool, idx, pred, lw[label[idx]])
    assert np.array_equal(votes.cpu().numpy(), pool.astype(np.int32))


# ---- 5. finish ----------------------------------------------------------------------------------------------------------------------------------
def test_finish_equals_numpy(dev):
    from act_amd import kernels as K
    rs = np.random.RandomState(10)
    P, C = 70001, 13
    votes = rs.randint(0, 3, size=(P, C)).astype(np.int32)
    votes[:100] = 0                                                          # no votes: class 0
    votes[100:200] = 2                                                       # all tied: class 0
    label = rs.randint(-1, C, size=P).astype(np.int32)                       # -1: not counted
    pred, cm = K.scene_finish(torch.from_numpy(votes).to(dev), torch.from_numpy(label).to(dev))
    ref = np.argmax(votes, 1)
    assert np.array_equal(pred.cpu().numpy(), ref)
    cm_ref = np.zeros((C, C), np.int64)
    ok = label >= 0
    np.add.at(cm_ref, (label[ok], ref[ok]), 1)
    assert np.array_equal(cm.cpu().numpy(), cm_ref)


# ---- 6. end to end on the golden rooms --------------------------------------------------------------------------------------------------------------
def _model(dev):
    from act_amd.models.semseg import get_model
    return fill_module(get_model(13), "g20.").to(dev).eval()


def test_end_to_end_with_injected_rows_equals_host_restatement(dev, tmp_path):
    from act_amd.tools.runner_semseg_test import evaluate_room, metric_lines, room_miou
    g, ds = _golden_ds(tmp_path)
    model = _model(dev)
    lw = torch.from_numpy(ds.labelweights.astype(np.float32)).to(dev)
    B, bp = 4, int(g["block_points"])
    scene_cms = []
    for name in g["file_list"]:
        tag = name[len("Area_5_room_"):-4]
        i = ds.file_list.index(name)
        rows = g["index_room_" + tag]
        pred, cm = evaluate_room(model, ds, i, 1, B, lw, dev, rows=[torch.from_numpy(rows.reshape(-1)).to(dev)])
        # host restatement: the golden's float32 blocks through the same model in the same batches, add_vote, np.argmax
        data = g["data_room_" + tag]
        pool = np.zeros((ds.scene_points_num[i], 13))
        with torch.no_grad():
            for s in range(0, data.shape[0], B):
                x = torch.from_numpy(data[s:s + B]).to(dev)
                lab = model(x.transpose(2, 1)).cpu().max(2)[1].numpy()
                pool = add_vote(pool, rows[s:s + B], lab, g["sample_weight_" + tag][s:s + B])
        ref = np.argmax(pool, 1)
        assert np.array_equal(pred, ref), tag
        label = ds.semantic_labels_list[i].astype(int)
        cm_ref = np.zeros((13, 13), np.int64)
        np.add.at(cm_ref, (label, ref), 1)
        assert np.array_equal(cm, cm_ref)
        iou_map = np.array([np.sum((ref == l) & (label == l)) / (np.sum((ref == l) | (label == l)) + 1e-6) for l in range(13)])
        seen = np.array([np.sum(label == l) for l in range(13)])
        assert room_miou(cm) == np.mean(iou_map[seen != 0])
        scene_cms.append((name[:-4], cm))
    lines, _, finals, m = metric_lines(scene_cms)
    assert len(lines) == 2 and 0 <= m["miou"] <= 1


# ---- 7. runner --------------------------------------------------------------------------------------------------------------------------------------
def _run(args, cwd, timeout=900):
    r = subprocess.run([sys.executable, "-m", "act_amd.tools.runner_semseg_test"] + args, cwd=cwd, capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stdout


def test_runner_synthetic_writes_reference_outputs_deterministically(tmp_path):
    outs = []
    for k in range(2):
        cwd = tmp_path / ("run%d" % k)
        cwd.mkdir()
        _run(["--synthetic", "--max_rooms", "1", "--num_votes", "2", "--visual", "--log_dir", "t", "--seed", "3"], str(cwd))
        vis = cwd / "log" / "semantic_seg" / "t" / "visual"
        assert (cwd / "log" / "semantic_seg" / "t" / "eval.txt").exists()
        files = sorted(os.listdir(vis))
        assert files == ["Area_5_synthetic_0.txt", "Area_5_synthetic_0_gt.obj", "Area_5_synthetic_0_pred.obj"], files
        pts = np.load(cwd / "log" / "semantic_seg" / "t" / "synthetic_rooms" / "Area_5_synthetic_0.npy")
        txt = (vis / "Area_5_synthetic_0.txt").read_text()
        assert len(txt.splitlines()) == pts.shape[0]
        gt = (vis / "Area_5_synthetic_0_gt.obj").read_text().splitlines()
        assert len(gt) == pts.shape[0] and gt[0].startswith("v ")
        outs.append([(vis / f).read_bytes() for f in files])
    assert outs[0] == outs[1]


# ---- 8. no host synchronisation inside a vote ---------------------------------------------------------------------------------------------------------
def test_no_host_sync_inside_a_vote(dev, tmp_path):
    from act_amd.tools.runner_semseg_test import Room, run_vote
    g, ds = _golden_ds(tmp_path)
    model = _model(dev)
    lw = torch.from_numpy(ds.labelweights.astype(np.float32)).to(dev)
    room = Room(ds, 0, dev)
    votes = torch.zeros(room.P, 13, dtype=torch.int32, device=dev)
    with torch.no_grad():
        run_vote(model, room, room.rows(0, 0, 0), votes, lw, 4)            # warm-up (allocations, GEMM first use)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            run_vote(model, room, room.rows(0, 0, 1), votes, lw, 4)
        finally:
            torch.cuda.set_sync_debug_mode("default")


# ---- 9. eval forward without the adjacency ---------------------------------------------------------------------------------------------------------
def test_eval_forward_without_adjacency_is_bit_identical(dev):
    from tests.golden.fill import clouds
    model = _model(dev)
    x = torch.from_numpy(clouds(20, 4, 2048)).to(dev).transpose(1, 2)
    with torch.no_grad():
        a = model(x)
    with torch.enable_grad():
        b = model(x)
    assert b.requires_grad and torch.equal(a, b.detach())


# ---- 10. checkpoint quality ------------------------------------------------------------------------------------------------------------------------
def test_trained_checkpoint_whole_room_miou(tmp_path):
    from act_amd.datasets.S3DISDataset import SyntheticS3DIS
    train = [sys.executable, "-m", "act_amd.tools.runner_semseg", "--synthetic", "--max_steps", "150", "--batch_size", "8", "--warmup_epoch", "0",
             "--learning_rate", "0.0005", "--log_every", "50", "--eval_batches", "2", "--num_workers", "2", "--log_dir", str(tmp_path / "train")]
    r = subprocess.run(train, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    ck = str(tmp_path / "train" / "checkpoints" / "best_model.pth")
    out = _run(["--synthetic", "--max_rooms", "2", "--num_votes", "1", "--ckpts", ck, "--log_dir", "q"], str(tmp_path))
    miou = float(re.search(r"eval point avg class IoU: ([0-9.]+)", out).group(1))
    held = SyntheticS3DIS("test", 2048, num_rooms=2)                          # the same held-out rooms
    lab = np.concatenate(held.room_labels).astype(np.int64)
    const = (np.bincount(lab, minlength=13) / lab.size).max() / 13            # best constant predictor's whole-room mIoU
    print(f"whole-room mIoU {miou:.4f}, best constant {const:.4f}")
    assert miou >= 3 * const, (miou, const)
