"""S3DIS whole-room sliding-window testing with voting (reference: semantic_segmentation/main_test.py), single GPU.

    python -m act_amd.tools.runner_semseg_test --root data/stanford_indoor3d/ --ckpts log/semantic_seg/exp/checkpoints/best_model.pth
    python -m act_amd.tools.runner_semseg_test --synthetic --ckpts best_model.pth --max_rooms 2

Same arguments and defaults as the reference, plus ``--synthetic`` (synthetic rooms written as Area_<test_area>_*.npy under the log directory,
act_amd.datasets.S3DISDataset.SyntheticS3DISWholeScene), ``--seed`` (key of the device draws) and ``--max_rooms``.  Every room of the test area is
tiled with overlapping 1 m blocks at a 0.5 m stride (dataset.py ScannetDatasetWholeScene); each of ``--num_votes`` passes fills and shuffles every
block to a multiple of ``--num_point`` rows, classifies all blocks in batches of ``--batch_size`` and adds one vote per row; each point takes the
class with the most votes.  Everything but the model runs in csrc/wholescene.hip: membership once per room, then per vote the keyed row build,
gather + centre and voting, with no host synchronisation; a room pays two host reads (its block counts and its predictions).  Outputs as the
reference writes them: ``log/semantic_seg/<log_dir>/eval.txt``, ``visual/<scene>.txt`` (one predicted label per point) and, with ``--visual``,
``<scene>_pred.obj`` / ``<scene>_gt.obj``.  Metrics are formed on the host in float64 from the per-room confusion matrices, with main_test.py's
formulas.  Draws differ from np.random (counter-based, keyed by seed, room, vote, block); ``evaluate_room(..., rows=...)`` injects row lists
instead (the reference's index_room).
"""
import argparse
import logging
import os
from pathlib import Path

import numpy as np
import torch

from .. import kernels as K
from ..datasets.S3DISDataset import S3DISWholeScene, SyntheticS3DISWholeScene, CLASSES, NUM_CLASSES
from ..models.semseg import get_model

# data_utils/indoor3d_util.py g_label2color (class index -> RGB)
G_LABEL2COLOR = np.array([[0, 255, 0], [0, 0, 255], [0, 255, 255], [255, 255, 0], [255, 0, 255], [100, 100, 255], [200, 200, 100],
                          [170, 120, 200], [255, 0, 0], [200, 100, 100], [10, 200, 100], [200, 200, 200], [50, 50, 50]])


def parse_args(argv=None):
    p = argparse.ArgumentParser('Model')
    p.add_argument('--model', type=str, default='pt', help='model name')
    p.add_argument('--optimizer_part', type=str, default='all', help='training all parameters or optimizing the new layers only')
    p.add_argument('--batch_size', type=int, default=32, help='batch Size during training')
    p.add_argument('--epoch', default=60, type=int, help='epoch to run')
    p.add_argument('--warmup_epoch', default=10, type=int, help='warmup epoch')
    p.add_argument('--learning_rate', default=0.0002, type=float, help='initial learning rate')
    p.add_argument('--gpu', type=str, default='0', help='specify GPU devices')
    p.add_argument('--log_dir', type=str, default='./exp', help='log path')
    p.add_argument('--normal', action='store_true', default=False, help='use normals')
    p.add_argument('--ckpts', type=str, default=None, help='ckpts')
    p.add_argument('--root', type=str, default='../data/stanford_indoor3d/', help='data root')
    p.add_argument('--num_point', type=int, default=2048, help='point number [default: 4096]')
    p.add_argument('--test_area', type=int, default=5, help='area for testing, option: 1-6 [default: 5]')
    p.add_argument('--num_votes', type=int, default=3, help='aggregate segmentation scores with voting [default: 5]')
    p.add_argument('--visual', action='store_true', default=False, help='visualize result [default: False]')
    # not in the reference
    p.add_argument('--synthetic', action='store_true', default=False, help='synthetic rooms instead of the S3DIS files')
    p.add_argument('--seed', type=int, default=0, help='key of the block fill / shuffle draws')
    p.add_argument('--max_rooms', type=int, default=0, help='test at most this many rooms (0: all)')
    return p.parse_args(argv)


REFERENCE_ARGS = ('model', 'optimizer_part', 'batch_size', 'epoch', 'warmup_epoch', 'learning_rate', 'gpu', 'log_dir', 'normal', 'ckpts', 'root',
                  'num_point', 'test_area', 'num_votes', 'visual')


# ---- metrics (main_test.py, float64 on the host from int64 confusion matrices: rows = label, columns = prediction) --------------------------
def _class_counts(cm):
    cm = np.asarray(cm, dtype=np.int64)
    correct = np.diag(cm)
    seen = cm.sum(axis=1)
    deno = seen + cm.sum(axis=0) - correct
    return correct, seen, deno


def room_miou(cm):
    """'Mean IoU of <scene>': mean of correct / (deno + 1e-6) over the classes present in the room"""
    correct, seen, deno = _class_counts(cm)
    iou_map = correct / (np.array(deno, dtype=np.float64) + 1e-6)
    return float(np.mean(iou_map[seen != 0]))


def total_metrics(cm):
    """summed confusion matrix -> dict(iou per class correct / deno, miou (with +1e-6), macc, oa) as main_test.py forms them"""
    correct, seen, deno = _class_counts(cm)
    IoU = correct / (np.array(deno, dtype=np.float64) + 1e-6)
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = correct / deno.astype(np.float64)
    return dict(iou=iou, miou=float(np.mean(IoU)), macc=float(np.mean(correct / (np.array(seen, dtype=np.float64) + 1e-6))),
                oa=float(np.sum(correct) / float(np.sum(seen) + 1e-6)))


def metric_lines(scene_cms):
    """[(scene, cm)] -> the reference's printed lines: one 'Mean IoU of' per room, the per-class IoU table, the three final figures"""
    lines = ['Mean IoU of %s: %.4f' % (name, room_miou(cm)) for name, cm in scene_cms]
    m = total_metrics(sum(np.asarray(cm, dtype=np.int64) for _, cm in scene_cms))
    table = '------- IoU --------\n'
    for l in range(NUM_CLASSES):
        table += 'class %s, IoU: %.3f \n' % (CLASSES[l] + ' ' * (14 - len(CLASSES[l])), m['iou'][l])
    return lines, table, ['eval point avg class IoU: %f' % m['miou'], 'eval whole scene point avg class acc: %f' % m['macc'],
                          'eval whole scene point accuracy: %f' % m['oa']], m


# ---- one room on the device ----------------------------------------------------------------------------------------------------------------
class Room:
    """device state of one room: xyz float64, labels int32, block table, members (one host read: the block counts), and the row layout of
    the non-empty blocks (block_ids, row_off: ceil(count / block_points) * block_points rows each, in the reference's block order)"""

    def __init__(self, ds, index, device):
        pts = ds.scene_points_list[index]
        self.name = ds.scene_name(index)
        self.P = pts.shape[0]
        self.block_points = ds.block_points
        table, self.gx, self.gy = ds.block_table(index)
        self.xyz = torch.from_numpy(np.ascontiguousarray(pts[:, :3], dtype=np.float64)).to(device)
        self.table = torch.from_numpy(table).to(device)
        self.label = torch.from_numpy(ds.semantic_labels_list[index].astype(int).astype(np.int32)).to(device)
        counts, self.offsets, self.members = K.scene_members(self.xyz, self.table, self.gx, self.gy)
        bid = np.nonzero(counts)[0]
        if bid.size == 0:
            raise ValueError(f"room {ds.file_list[index]}: no block holds a point")
        size = (counts[bid] + self.block_points - 1) // self.block_points * self.block_points
        roff = np.concatenate([[0], np.cumsum(size)])
        self.counts, self.R, self.num_blocks = counts, int(roff[-1]), int(roff[-1]) // self.block_points
        self.block_ids = torch.from_numpy(bid.astype(np.int32)).to(device)
        self.row_off = torch.from_numpy(roff.astype(np.int32)).to(device)

    def rows(self, seed, room, vote):
        return K.scene_rows(self.members, self.offsets, self.block_ids, self.row_off, self.R, self.block_points, seed, room, vote)


def run_vote(model, room, rows, votes, labelweights, batch_size):
    """one vote of one room, no host synchronisation: gather + centre every row, classify the blocks in batches (the last one at its real
    size), add the votes"""
    bp = room.block_points
    data = K.scene_gather(room.xyz, room.table, rows, room.block_ids, room.row_off).view(room.num_blocks, bp, 3)
    for s in range(0, room.num_blocks, batch_size):
        e = min(s + batch_size, room.num_blocks)
        logp = model(data[s:e].transpose(2, 1))
        K.scene_vote(logp, rows[s * bp:e * bp], room.label, labelweights, votes)


@torch.no_grad()
def evaluate_room(model, ds, index, num_votes, batch_size, labelweights, device, seed=0, rows=None, room=None):
    """-> (pred numpy int32 [P], cm numpy int64 [13, 13]); ``rows``: optional list of injected row lists (one int32 [R] per vote)"""
    room = room if room is not None else Room(ds, index, device)
    votes = torch.zeros(room.P, NUM_CLASSES, dtype=torch.int32, device=device)
    for v in range(num_votes):
        r = rows[v] if rows is not None else room.rows(seed, index, v)
        run_vote(model, room, r, votes, labelweights, batch_size)
    pred, cm = K.scene_finish(votes, room.label)
    return pred.cpu().numpy(), cm.cpu().numpy()


def _write_obj(path, xyz, colors):
    np.savetxt(path, np.concatenate([xyz.astype(np.float64), colors.astype(np.float64)], axis=1), fmt='v %f %f %f %d %d %d')


def main(argv=None):
    args = parse_args(argv)
    if 'CUDA_VISIBLE_DEVICES' not in os.environ:
        os.environ['CUDA_VISIBLE_DEVICES'] = args.gpu
    experiment_dir = 'log/semantic_seg/' + args.log_dir
    visual_dir = Path(experiment_dir + '/visual/')
    visual_dir.mkdir(parents=True, exist_ok=True)
    logger = logging.getLogger("Model")
    logger.setLevel(logging.INFO)
    handler = logging.FileHandler('%s/eval.txt' % experiment_dir)
    handler.setLevel(logging.INFO)
    handler.setFormatter(logging.Formatter('%(asctime)s - %(name)s - %(levelname)s - %(message)s'))
    logger.addHandler(handler)

    def log_string(s):
        logger.info(s)
        print(s, flush=True)

    log_string('PARAMETER ...')
    log_string(args)
    if args.synthetic:
        ds = SyntheticS3DISWholeScene(os.path.join(experiment_dir, 'synthetic_rooms'), args.num_point, num_rooms=args.max_rooms or 8,
                                      seed=args.seed, test_area=args.test_area)
    else:
        ds = S3DISWholeScene(args.root, split='test', test_area=args.test_area, block_points=args.num_point)
    log_string("The number of test data is: %d" % len(ds))
    device = torch.device('cuda', torch.cuda.current_device())
    torch.manual_seed(args.seed)                                          # the initial weights of entries a checkpoint does not hold
    model = get_model(NUM_CLASSES).to(device)
    print('# generator parameters:', sum(p.numel() for p in model.parameters()))
    model.load_model_from_ckpt_withrename(args.ckpts)
    model = model.eval()
    labelweights = torch.from_numpy(np.asarray(ds.labelweights, dtype=np.float32)).to(device)

    n = len(ds) if not args.max_rooms else min(args.max_rooms, len(ds))
    log_string('---- EVALUATION WHOLE SCENE----')
    scene_cms = []
    for i in range(n):
        name = ds.scene_name(i)
        print("Inference [%d/%d] %s ..." % (i + 1, n, name), flush=True)
        pred, cm = evaluate_room(model, ds, i, args.num_votes, args.batch_size, labelweights, device, seed=args.seed)
        scene_cms.append((name, cm))
        correct, _, deno = _class_counts(cm)
        print(correct / (np.array(deno, dtype=np.float64) + 1e-6))
        log_string('Mean IoU of %s: %.4f' % (name, room_miou(cm)))
        print('----------------------------')
        np.savetxt(os.path.join(visual_dir, name + '.txt'), pred, fmt='%d')
        if args.visual:
            pts = ds.scene_points_list[i]
            gt = ds.semantic_labels_list[i].astype(int)
            _write_obj(os.path.join(visual_dir, name + '_pred.obj'), pts[:, :3], G_LABEL2COLOR[pred])
            _write_obj(os.path.join(visual_dir, name + '_gt.obj'), pts[:, :3], G_LABEL2COLOR[gt])
    _, table, finals, m = metric_lines(scene_cms)
    log_string(table)
    for line in finals:
        log_string(line)
    print("Done!")
    logger.removeHandler(handler)
    handler.close()
    return m


if __name__ == '__main__':
    main()
