"""S3DIS semantic segmentation: training + block evaluation (reference: semantic_segmentation/main.py), single GPU.

    python -m act_amd.tools.runner_semseg --root data/stanford_indoor3d --ckpts act_pretrain.pth
    python -m act_amd.tools.runner_semseg --synthetic --max_steps 150
    python -m act_amd.tools.runner_semseg --synthetic --model pointnet2_sem_seg            # the PointNet++ SSG baseline
    python -m act_amd.tools.runner_semseg --synthetic --model dgcnn_semseg                 # the DGCNN baseline; any other --model: the Transformer

Same arguments and defaults as the reference, plus ``--synthetic`` (generated rooms, act_amd.datasets.S3DISDataset.SyntheticS3DIS), ``--max_steps``
(stop training after that many steps, then evaluate once), ``--log_every``, ``--seed``, ``--eval_batches`` and ``--device_sampler`` (blocks sampled
on the device from resident rooms, act_amd.datasets.S3DISDevice, in place of the two DataLoaders; its draws are keyed hashes, not
np.random's).  Per step, like the reference:
isotropic scale U[0.8, 1.25] and shift U[-0.1, 0.1]^3 per cloud (here one launch on the device), the weighted NLL with the train split's
labelweights, ``optimizer.step()``, gradient clipping at 10, a second ``optimizer.step()``, ``zero_grad`` (main.py:209-223).  No host
synchronisation per step: loss and correct counts accumulate on the device and are read once per ``--log_every`` steps.  Evaluation accumulates
an int64 confusion matrix on the device and reads it once; OA, mAcc, mIoU and per-class IoU follow main.py:243-300.  Checkpoints
``{epoch, class_avg_iou, model_state_dict, optimizer_state_dict}`` as the reference writes them.
"""
import argparse
import os
import time

import numpy as np
import torch

from . import builder
from .. import kernels as K
from ..datasets.S3DISDataset import S3DISDataset, SyntheticS3DIS, CLASSES, NUM_CLASSES
from ..datasets.data_transforms import PointcloudScaleAndTranslate
from ..models.semseg import get_model, get_loss


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
    p.add_argument('--npoint', type=int, default=2048, help='point Number')
    p.add_argument('--test_area', type=int, default=5, help='test_area')
    p.add_argument('--normal', action='store_true', default=False, help='use normals')
    p.add_argument('--ckpts', type=str, default=None, help='ckpts')
    p.add_argument('--root', type=str, default='../data/stanford_indoor3d/', help='data root')
    # not in the reference
    p.add_argument('--synthetic', action='store_true', default=False, help='generated rooms instead of the S3DIS files')
    p.add_argument('--max_steps', type=int, default=0, help='stop training after this many steps (0: run every epoch)')
    p.add_argument('--log_every', type=int, default=20, help='steps between two reads of the accumulated loss / accuracy')
    p.add_argument('--eval_batches', type=int, default=0, help='evaluate on at most this many test batches (0: all)')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--num_workers', type=int, default=4)
    p.add_argument('--device_sampler', action='store_true', default=False, help='sample the blocks on the device from resident rooms')
    return p.parse_args(argv)


REFERENCE_ARGS = ('model', 'optimizer_part', 'batch_size', 'epoch', 'warmup_epoch', 'learning_rate', 'gpu', 'log_dir', 'npoint', 'test_area',
                  'normal', 'ckpts', 'root')


def add_weight_decay(model, weight_decay=1e-5, skip_list=(), optimizer_part='all'):
    """main.py add_weight_decay: 'only_new' trains the parameters whose name contains 'cls' (the segmentation head) only"""
    decay, no_decay = [], []
    for name, param in model.named_parameters():
        if not param.requires_grad:
            continue
        if optimizer_part == 'only_new' and 'cls' not in name:
            continue
        if len(param.shape) == 1 or name.endswith(".bias") or 'token' in name or name in skip_list:
            no_decay.append(param)
        else:
            decay.append(param)
    return [{'params': no_decay, 'weight_decay': 0.}, {'params': decay, 'weight_decay': weight_decay}]


def seg_metrics(cm):
    """confusion matrix [C, C] (rows: target, columns: prediction) -> OA, mAcc, mIoU, per-class IoU (main.py:243-300)"""
    cm = np.asarray(cm, dtype=np.int64)
    correct_class = np.diag(cm).astype(np.float64)
    seen_class = cm.sum(axis=1).astype(np.float64)
    deno_class = (cm.sum(axis=1) + cm.sum(axis=0) - np.diag(cm)).astype(np.float64)
    total = cm.sum()
    oa = correct_class.sum() / float(total) if total else 0.0
    miou = np.mean(correct_class / (deno_class + 1e-6))
    macc = np.mean(correct_class / (seen_class + 1e-6))
    iou = correct_class / np.maximum(deno_class, 1.0)
    return dict(oa=float(oa), macc=float(macc), miou=float(miou), iou=iou)


def _seed_worker(worker_id):
    """every loader worker draws blocks from its own stream (derived from the loader's seed)"""
    info = torch.utils.data.get_worker_info()
    info.dataset.rng = np.random.default_rng(info.seed % (1 << 32))


def datasets(args):
    if args.synthetic:
        return (SyntheticS3DIS('train', args.npoint, seed=args.seed), SyntheticS3DIS('test', args.npoint, seed=args.seed))
    rng = np.random.default_rng(args.seed)
    return (S3DISDataset('train', args.root, args.npoint, args.test_area, rng=rng),
            S3DISDataset('test', args.root, args.npoint, args.test_area, rng=np.random.default_rng(args.seed + 1)))


class _EpochLoader:
    """one epoch of a DeviceS3DISBlocks as an iterable of (pts, target) on the device: what ``evaluate`` takes in place of a DataLoader"""

    def __init__(self, blocks, batch_size, seed, shuffle, drop_last, epoch=0):
        self.blocks, self.batch_size, self.seed, self.shuffle, self.drop_last, self.epoch = blocks, batch_size, seed, shuffle, drop_last, epoch

    def __iter__(self):
        return self.blocks.epoch(self.batch_size, self.epoch, self.seed, self.shuffle, self.drop_last)


@torch.no_grad()
def evaluate(model, loader, weights, device, max_batches=0):
    """-> (metrics dict, mean loss); one host read of the confusion matrix and the loss sum"""
    model.eval()
    crit = get_loss()
    cm = torch.zeros(NUM_CLASSES, NUM_CLASSES, dtype=torch.int64, device=device)
    loss_sum = torch.zeros((), dtype=torch.float32, device=device)
    n = 0
    for i, (pts, target) in enumerate(loader):
        if max_batches and i >= max_batches:
            break
        if pts.device != device:
            pts = pts.to(device, torch.float32, non_blocking=True)
            target = target.to(device, torch.int64, non_blocking=True)
        target = target.reshape(-1)
        logp = model(pts.transpose(2, 1))
        loss_sum += crit(logp, target, weights)
        K.confusion(logp.reshape(-1, NUM_CLASSES), target, NUM_CLASSES, out=cm)
        n += 1
    m = seg_metrics(cm.cpu().numpy())
    return m, float(loss_sum.item()) / max(n, 1)


def build_model(args):
    """``--model pointnet2_sem_seg``: the PointNet++ SSG baseline (models/pointnet2_nets.py) on the xyz channels the blocks carry; ``--model
    dgcnn_semseg``: the DGCNN baseline (models/dgcnn_nets.py) on the same channels; every other value: the Transformer"""
    if args.model == 'pointnet2_sem_seg':
        from ..models.pointnet2_nets import pointnet2_sem_seg
        return pointnet2_sem_seg(NUM_CLASSES, in_channel=3)
    if args.model == 'dgcnn_semseg':
        from ..models.dgcnn_nets import dgcnn_semseg
        return dgcnn_semseg(NUM_CLASSES, in_channel=3)
    return get_model(NUM_CLASSES)


def main(argv=None):
    args = parse_args(argv)
    torch.manual_seed(args.seed)
    device = torch.device('cuda', torch.cuda.current_device())
    train_set, test_set = datasets(args)
    if args.device_sampler:
        from ..datasets.S3DISDevice import DeviceS3DISBlocks
        train_blocks, test_blocks = DeviceS3DISBlocks.from_dataset(train_set, device), DeviceS3DISBlocks.from_dataset(test_set, device)
        room_bytes, index_bytes = (sum(v) for v in zip(train_blocks.resident_bytes(), test_blocks.resident_bytes()))
        print(f"device sampler: rooms {room_bytes} bytes, index {index_bytes} bytes", flush=True)
        train_loader = None
        test_loader = _EpochLoader(test_blocks, args.batch_size, args.seed + 1, shuffle=False, drop_last=False)
    else:
        g = torch.Generator().manual_seed(args.seed)
        train_loader = torch.utils.data.DataLoader(train_set, batch_size=args.batch_size, shuffle=True, num_workers=args.num_workers, drop_last=True,
                                                   generator=g, pin_memory=True, persistent_workers=args.num_workers > 0,
                                                   worker_init_fn=_seed_worker)
        test_loader = torch.utils.data.DataLoader(test_set, batch_size=args.batch_size, shuffle=False, num_workers=args.num_workers,
                                                  generator=torch.Generator().manual_seed(args.seed + 1), worker_init_fn=_seed_worker)
    weights = torch.tensor(np.asarray(train_set.labelweights, dtype=np.float32), device=device)
    print(f"train samples {len(train_set)}, test samples {len(test_set)}, labelweights {np.round(train_set.labelweights, 3).tolist()}", flush=True)

    model = build_model(args).to(device)
    crit = get_loss()
    if args.ckpts is not None:
        model.load_model_from_ckpt(args.ckpts)
    print('# generator parameters:', sum(p.numel() for p in model.parameters()), flush=True)
    groups = add_weight_decay(model, weight_decay=0.05, optimizer_part=args.optimizer_part)
    optimizer = builder.FusedAdamW(groups, lr=args.learning_rate, weight_decay=0.05, fused=True)
    scheduler = builder.CosineLRScheduler(optimizer, t_initial=args.epoch, lr_min=1e-6, warmup_lr_init=1e-6, warmup_t=args.warmup_epoch,
                                          cycle_limit=1, t_in_epochs=True)
    augment = PointcloudScaleAndTranslate(scale_low=0.8, scale_high=1.25, translate_range=0.1)
    ckpt_dir = os.path.join(args.log_dir, 'checkpoints')
    os.makedirs(ckpt_dir, exist_ok=True)
    best_iou, step, done = -1.0, 0, False
    loss_acc = torch.zeros((), dtype=torch.float32, device=device)
    correct_acc = torch.zeros((), dtype=torch.int64, device=device)
    seen, t0 = 0, time.time()
    model.zero_grad(set_to_none=True)
    for epoch in range(args.epoch):
        model.train()
        for pts, target in (train_blocks.epoch(args.batch_size, epoch, args.seed) if args.device_sampler else train_loader):
            if not args.device_sampler:
                pts = pts.to(device, torch.float32, non_blocking=True).contiguous()
                target = target.to(device, torch.int64, non_blocking=True)
            target = target.reshape(-1)
            B = pts.shape[0]
            scale = torch.empty(B, 1, device=device).uniform_(0.8, 1.25).expand(B, 3)       # isotropic (provider.random_scale_point_cloud)
            augment(pts, scale=scale)
            logp = model(pts.transpose(2, 1))
            loss, correct = crit.with_correct(logp, target, weights)
            loss.backward()
            optimizer.step()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 10, norm_type=2)
            optimizer.step()
            model.zero_grad(set_to_none=True)
            loss_acc += loss.detach()
            correct_acc += correct
            seen += B * args.npoint
            step += 1
            if step % args.log_every == 0:
                l, c = loss_acc.item() / args.log_every, correct_acc.item() / seen
                print(f"epoch {epoch} step {step}: loss {l:.4f} acc {100 * c:.2f}% lr {optimizer.param_groups[0]['lr']:.2e} "
                      f"({(time.time() - t0) / args.log_every * 1e3:.1f} ms/step)", flush=True)
                loss_acc.zero_(); correct_acc.zero_(); seen, t0 = 0, time.time()
            if args.max_steps and step >= args.max_steps:
                done = True
                break
        scheduler.step(epoch)                                             # main.py: after the epoch, with its index
        if args.device_sampler:
            test_loader.epoch = epoch
        m, eval_loss = evaluate(model, test_loader, weights, device, args.eval_batches)
        print(f"eval epoch {epoch}: loss {eval_loss:.4f} OA {100 * m['oa']:.2f} mAcc {100 * m['macc']:.2f} mIoU {100 * m['miou']:.2f}", flush=True)
        print("IoU " + " ".join(f"{c}:{100 * v:.1f}" for c, v in zip(CLASSES, m['iou'])), flush=True)
        if m['miou'] >= best_iou:
            best_iou = m['miou']
            torch.save({'epoch': epoch, 'class_avg_iou': m['miou'], 'model_state_dict': model.state_dict(),
                        'optimizer_state_dict': optimizer.state_dict()}, os.path.join(ckpt_dir, 'best_model.pth'))
        if done:
            break
    print(f"best mIoU {100 * best_iou:.2f}", flush=True)
    return best_iou


if __name__ == '__main__':
    main()
