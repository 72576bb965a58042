"""Stage-II pretraining loop (reference: tools/runner_pretrain.py:53-226), same ``run_net`` signature.

Differences forced by the hardware-first design, none of them visible in the config surface:
  * augmentation, masking, token compaction and the loss run on the device without host synchronisation;
  * DDP is created with broadcast_buffers=False (BatchNorm statistics stay per rank, exactly as the
    reference's non-SyncBN default) and without find_unused_parameters: the never-used heads
    (lm_head / cls_head) are kept in the state_dict but frozen, so gradients are a single bucketed RCCL
    all-reduce overlapped with backward;
  * the logged loss is all-reduced every step but read back only every ``log_every`` steps;
  * the linear-SVM validation (reference :47-51, :228-287, which its run_net never calls) is solved on the device (utils/svm.py) and is
    opt-in: ``svm_val: True`` in the config, a ``dataset.extra_train`` section and a positive ``--val_freq``;
  * a weighted k-NN probe of the same features (utils/knn_probe.py; no solver, nothing to tune) runs next to the SVM or instead of it:
    ``knn_val: {k: [10, 20], T: 0.07}`` under the same two other conditions.
"""
import time
import os
import weakref

import torch
import torch.nn as nn

from . import builder
from ..datasets.data_transforms import PointcloudScaleAndTranslate, build_transforms
from ..utils import dist_utils, misc
from ..utils.AverageMeter import AverageMeter
from ..utils.logger import get_logger, print_log

train_transforms = PointcloudScaleAndTranslate()


class Acc_Metric:
    def __init__(self, acc=0.):
        self.acc = acc.acc if hasattr(acc, "acc") else (acc['acc'] if isinstance(acc, dict) else acc)

    def better_than(self, other):
        return self.acc > other.acc

    def state_dict(self):
        return {'acc': self.acc}


def evaluate_svm(train_features, train_labels, test_features, test_labels):
    """accuracy (percent) on the test features of a LinearSVC fitted to the train features (reference :47-51), on device tensors: the solve
    and the prediction stay on the device, the accuracy is the one value read back"""
    from ..utils.svm import LinearSVC
    clf = LinearSVC().fit(train_features, train_labels)
    pred = clf.predict(test_features)
    return float((pred == test_labels.to(pred.dtype)).sum() * 100. / pred.shape[0])


def evaluate_knn(train_features, train_labels, test_features, test_labels, ks=(10, 20), T=0.07):
    """{"knn@k": top-1 accuracy (percent), "knn@k/top5": ...} on the test features of the weighted k-NN vote over the train features (cosine
    similarity, weights exp(sim / T)): search, vote and the hit counts stay on the device, the counts are the one thing read back"""
    from ..utils.knn_probe import KNNClassifier
    ks = [int(ks)] if isinstance(ks, int) else [int(k) for k in ks]
    return KNNClassifier(k=ks, T=float(T)).fit(train_features, train_labels).score(test_features, test_labels)


def extract_features(base_model, dataloader, npoints):
    """(features [n, C], labels [n]) of a ModelNet-style loader, concatenated on the device: misc.fps to ``npoints``, ``forward(noaug=True)``"""
    feats, labels = [], []
    for _, _, data in dataloader:
        points = misc.fps(data[0].cuda(non_blocking=True), npoints)
        assert points.size(1) == npoints
        feats.append(base_model(points, noaug=True).detach())
        labels.append(data[1].cuda(non_blocking=True).view(-1))
    return torch.cat(feats, dim=0), torch.cat(labels, dim=0)


def validate(base_model, extra_train_dataloader, test_dataloader, epoch, val_writer, args, config, logger=None):
    """Point-BERT's linear-SVM protocol (reference :228-287): features of the extra_train and val splits, a linear SVM on the first, accuracy
    on the second.  Under ``args.distributed`` the features are all-gathered and every rank solves the same problem.
    ``knn_val`` in the config adds the weighted k-NN probe on the same (gathered) features; it alone makes its first k's top-1 the metric, next
    to ``svm_val`` the SVM accuracy stays the metric and the k-NN accuracies are logged."""
    svm_val, knn_val = bool(config.get('svm_val', False)), config.get('knn_val', None)
    if not knn_val:
        svm_val = True                                  # (called directly without either key: the SVM protocol, as before)
    print_log(f"[VALIDATION] Start validating epoch {epoch}", logger=logger)
    base_model.eval()
    npoints = config.dataset.train.others.npoints
    with torch.no_grad():
        train_features, train_label = extract_features(base_model, extra_train_dataloader, npoints)
        test_features, test_label = extract_features(base_model, test_dataloader, npoints)
        if args.distributed:
            train_features, train_label, test_features, test_label = (dist_utils.gather_tensor(t, args) for t in
                                                                      (train_features, train_label, test_features, test_label))
        train_features, test_features = train_features.float(), test_features.float()
        if svm_val:
            svm_acc = evaluate_svm(train_features, train_label, test_features, test_label)
            print_log('[Validation] EPOCH: %d  acc = %.4f' % (epoch, svm_acc), logger=logger)
        if knn_val:
            ks = knn_val.get('k', [10, 20])
            ks = [int(ks)] if isinstance(ks, int) else [int(k) for k in ks]
            knn_acc = evaluate_knn(train_features, train_label, test_features, test_label, ks, float(knn_val.get('T', 0.07)))
            for k in ks:
                print_log('[Validation] EPOCH: %d  knn@%d = %.4f' % (epoch, k, knn_acc['knn@%d' % k]), logger=logger)
    if val_writer is not None:
        if svm_val:
            val_writer.add_scalar('Metric/ACC', svm_acc, epoch)
        if knn_val:
            for k in ks:
                val_writer.add_scalar('Metric/KNN@%d' % k, knn_acc['knn@%d' % k], epoch)
    return Acc_Metric(svm_acc if svm_val else knn_acc['knn@%d' % ks[0]])


def freeze_unused_heads(model):
    """lm_head / cls_head never receive gradients in ACT_PointDistillation.forward (models/act.py:190-196 vs
    :269-309); freezing them removes the need for DDP(find_unused_parameters=True)."""
    enc = getattr(model, "ACT_encoder", None)
    if enc is not None:
        for m in (enc.lm_head, enc.cls_head):
            for p in m.parameters():
                p.requires_grad = False


def set_stack_chunk(model, chunk):
    """blocks per composite host call for every TransformerEncoder / TransformerDecoder of ``model`` (None: process default, 0: whole stack)"""
    from act_amd.models.act import TransformerEncoder, TransformerDecoder
    for m in model.modules():
        if isinstance(m, (TransformerEncoder, TransformerDecoder)):
            m.stack_chunk = chunk


def wrap_ddp(base_model, args):
    device_ids = [args.local_rank % torch.cuda.device_count()] if torch.cuda.is_available() and args.use_gpu else None
    if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1 and "ACT_BLOCK_STACK_CHUNK" not in os.environ:
        # a block stack hands its parameter gradients to DDP when its backward call returns: in chunks of 4 blocks the bucket all-reduces of the
        # deeper blocks start while the shallower ones are still being differentiated.  Set on THIS model's encoder / decoder modules (no process-wide
        # state); bit-identical to any other chunking, the folded gradient of the shared pos included (tests/test_gpu_composite.py)
        set_stack_chunk(base_model, 4)
    return nn.parallel.DistributedDataParallel(base_model, device_ids=device_ids, broadcast_buffers=False,
                                               gradient_as_bucket_view=True, bucket_cap_mb=25)


class _Single(nn.Module):
    """exposes ``.module`` like DataParallel/DDP so builder.build_opti_sche sees the same object shape."""

    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, *a, **k):
        return self.module(*a, **k)


class _Announced:
    """the batch that the previous train_step on THIS model already augmented (in place) and announced to the teacher prefetch: a weak
    reference plus the tensor version right after the augmentation, kept per model in a module-level WeakKeyDictionary (two models trained in one
    process do not see each other's batches; nothing is stored ON the module, so ``torch.save(model)`` / ``mp.spawn(args=(model,))`` still pickle
    it), so the same tensor handed back as ``points`` is not augmented twice"""
    _by_model = weakref.WeakKeyDictionary()

    @staticmethod
    def mark(model, t):
        _Announced._by_model[model] = (weakref.ref(t), t._version)

    @staticmethod
    def is_marked(model, t):
        ref, version = _Announced._by_model.get(model, (None, -1))
        return ref is not None and ref() is t and version == t._version


def transforms_from_config(config):
    """None without the optional top-level key ``train_transforms`` (the module-level object is then used, exactly as before); with it, a
    Compose of the listed {NAME: <class>, <keyword arguments>}: the whole chain is one launch per batch"""
    spec = config.get('train_transforms')
    return build_transforms(spec) if spec is not None else None


def train_step(base_model, optimizer, points, config, num_iter=1, augment=True, draws=None, next_points=None, next_draws=None,
               transforms=None, aug_draws=None, next_aug_draws=None):
    """one optimisation step on a device batch [B,N,3]; returns the detached loss tensor (no host sync).

    ``next_points`` (optional): the NEXT batch.  It is augmented here and announced to the model, which starts its grouping and
    frozen-teacher forward on the auxiliary stream while this batch's backward runs; pass that same tensor as ``points`` of the
    next call (it is not augmented twice).  ``draws`` / ``next_draws`` (parity tests): injected random draws of this step / of the next step's teacher.
    ``transforms``: the Compose of the config's ``train_transforms`` key (None: the module-level ``train_transforms``); ``aug_draws`` /
    ``next_aug_draws``: its injected draws for this batch / the next one."""
    inner = base_model.module if hasattr(base_model, "module") else base_model
    if augment and not _Announced.is_marked(inner, points):
        points = train_transforms(points) if transforms is None else transforms(points, draws=aug_draws)
    loss = base_model(points, draws=draws) if draws is not None else base_model(points)
    if isinstance(loss, tuple):                      # ACT_PointBERT returns (moco, dvae, cutmix): summed (tools/runner_pretrain.py:140-142)
        loss = loss[0] + loss[1] + loss[2]
    if next_points is not None:
        if augment:
            next_points = train_transforms(next_points) if transforms is None else transforms(next_points, draws=next_aug_draws)
            _Announced.mark(inner, next_points)
        if hasattr(inner, "prefetch_teacher"):
            inner.prefetch_teacher(next_points, next_draws) if next_draws is not None else inner.prefetch_teacher(next_points)
    loss.backward()
    if num_iter == config.step_per_update:
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
    return loss.detach()


def run_net(args, config, train_writer=None, val_writer=None, max_steps=None, log_every=100):
    logger = get_logger(args.log_name)
    (train_sampler, train_dataloader), (_, test_dataloader) = builder.dataset_builder(args, config.dataset.train), \
        builder.dataset_builder(args, config.dataset.val)
    # validation is opt-in: without all three of these the loop, its random draws and its checkpoints are what they are without it
    # (svm_val: the linear SVM; knn_val: the weighted k-NN probe; either switches the validation on)
    svm_val = bool(config.dataset.get('extra_train')) and getattr(args, 'val_freq', 0) > 0 and \
        (bool(config.get('svm_val', False)) or bool(config.get('knn_val', None)))
    extra_train_dataloader = builder.dataset_builder(args, config.dataset.extra_train)[1] if svm_val else None
    base_model = builder.model_builder(config.model)
    freeze_unused_heads(base_model)
    transforms = transforms_from_config(config)
    device = torch.device("cuda", args.local_rank % max(1, torch.cuda.device_count()))
    if args.use_gpu:
        torch.cuda.set_device(device)          # every launch goes to the current device's current stream
        base_model.to(device)
    if args.distributed:                       # one enqueue loop per rank on one host: own cores, on the GPU's NUMA node where sysfs tells (ACT_PIN_CORES=0 disables)
        from act_amd.utils.dist_utils import pin_rank
        pin = pin_rank(args.local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", getattr(args, "world_size", 1))), device.index if args.use_gpu else None)
        print_log(f'[rank {args.local_rank}] host affinity: {pin}', logger=logger)
    start_epoch, best_metrics, metrics = 0, Acc_Metric(0.), Acc_Metric(0.)
    if args.resume:
        start_epoch, best_metric = builder.resume_model(base_model, args, logger=logger)
        best_metrics = Acc_Metric(best_metric)
    elif args.start_ckpts is not None:
        builder.load_model(base_model, args.start_ckpts, logger=logger)
    if args.distributed:
        if args.sync_bn:
            base_model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(base_model)
            print_log('Using Synchronized BatchNorm ...', logger=logger)
        base_model = wrap_ddp(base_model, args)
        print_log('Using Distributed Data parallel ...', logger=logger)
    else:
        base_model = _Single(base_model)
    optimizer, scheduler = builder.build_opti_sche(base_model, config)
    if args.resume:
        builder.resume_optimizer(optimizer, args, logger=logger)

    base_model.zero_grad()
    steps = 0
    losses_log = []
    for epoch in range(start_epoch, config.max_epoch + 1):
        if args.distributed:
            train_sampler.set_epoch(epoch)
        base_model.train()
        epoch_start_time = batch_start_time = time.time()
        batch_time, data_time, losses = AverageMeter(), AverageMeter(), AverageMeter(['Loss'])
        num_iter = 0
        n_batches = len(train_dataloader)
        pending = []
        npoints = config.dataset.train.others.npoints
        dataset_name = config.dataset.train._base_.NAME

        def to_points(data):
            if dataset_name == 'ShapeNet':
                pts = data.to(device, non_blocking=True)
            elif dataset_name == 'ModelNet':
                pts = misc.fps(data[0].to(device, non_blocking=True), npoints)
            else:
                raise NotImplementedError(f'Train phase do not support {dataset_name}')
            assert pts.size(1) == npoints
            return pts

        loader = iter(train_dataloader)
        nxt = next(loader, None)
        points = to_points(nxt[2]) if nxt is not None else None
        for idx in range(n_batches):
            if points is None:
                break
            num_iter += 1
            n_itr = epoch * n_batches + idx
            data_time.update(time.time() - batch_start_time)
            nxt = next(loader, None)                         # one batch of look-ahead: its teacher forward overlaps this backward
            next_points = to_points(nxt[2]) if nxt is not None else None
            loss = train_step(base_model, optimizer, points, config, num_iter, next_points=next_points, transforms=transforms)
            points = next_points
            if num_iter == config.step_per_update:
                num_iter = 0
            if args.distributed:
                loss = dist_utils.reduce_tensor(loss, args)
            pending.append(loss)
            steps += 1
            if idx % log_every == 0 or (max_steps is not None and steps >= max_steps):
                vals = torch.stack(pending).tolist()           # the only host sync, once per log interval
                pending = []
                for v in vals:
                    losses.update([v])
                    losses_log.append(v)
                if train_writer is not None:
                    train_writer.add_scalar('Loss/Batch/Loss', vals[-1], n_itr)
                    train_writer.add_scalar('Loss/Batch/LR', optimizer.param_groups[0]['lr'], n_itr)
                batch_time.update(time.time() - batch_start_time)
                print_log('[Epoch %d/%d][Batch %d/%d] BatchTime = %.3f (s) DataTime = %.3f (s) [Losses] = %s lr = %.6f' %
                          (epoch, config.max_epoch, idx + 1, n_batches, batch_time.val(), data_time.val(),
                           ['%.4f' % l for l in losses.val()], optimizer.param_groups[0]['lr']), logger=logger)
            batch_start_time = time.time()
            if max_steps is not None and steps >= max_steps:
                break
        if pending:
            for v in torch.stack(pending).tolist():
                losses.update([v]); losses_log.append(v)
        if scheduler is not None:
            scheduler.step(epoch)
        if train_writer is not None:
            train_writer.add_scalar('Loss/Epoch/Loss_1', losses.avg(0), epoch)
        print_log('[Training] EPOCH: %d EpochTime = %.3f (s) Losses = %s lr = %.6f' %
                  (epoch, time.time() - epoch_start_time, ['%.4f' % l for l in losses.avg()], optimizer.param_groups[0]['lr']),
                  logger=logger)
        if svm_val and epoch % args.val_freq == 0:
            metrics = validate(base_model, extra_train_dataloader, test_dataloader, epoch, val_writer, args, config, logger=logger)
            if metrics.better_than(best_metrics):
                best_metrics = metrics
                builder.save_checkpoint(base_model, optimizer, epoch, metrics, best_metrics, 'ckpt-best', args, logger=logger)
        builder.save_checkpoint(base_model, optimizer, epoch, metrics, best_metrics, 'ckpt-last', args, logger=logger)
        if epoch % 25 == 0 and epoch >= 250:
            builder.save_checkpoint(base_model, optimizer, epoch, metrics, best_metrics, f'ckpt-epoch-{epoch:03d}', args, logger=logger)
        if (config.max_epoch - epoch) < 3:
            builder.save_checkpoint(base_model, optimizer, epoch, metrics, best_metrics, f'ckpt-epoch-{epoch:03d}', args, logger=logger)
        if max_steps is not None and steps >= max_steps:
            break
    if train_writer is not None:
        train_writer.close()
    if val_writer is not None:
        val_writer.close()
    return losses_log
