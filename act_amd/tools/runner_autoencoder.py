"""Stage-I autoencoder training loop (reference: tools/runner_autoencoder.py:18-217), same ``run_net`` signature.

temperature: cosine 1 -> 0.0625 over ``temp.ntime`` iterations (:42-53); KL weight: 0 for the first 10k iterations, then
cosine ``kldweight.start`` -> ``kldweight.target`` (:18-40); loss = recon (CD-L1 coarse + fine) + kld_weight * KL.
``validate`` (the periodic validation of ``run_net``) reports whole-batch Chamfer L1/L2 x1000.

Evaluation of a trained tokenizer (reference :219-420, ``main_autoencoder.py --val / --test``): ``evaluate`` / ``validate_net`` / ``test_net``
below give the reference's full report -- the four per-sample losses, F-Score@0.01 / CDL1 / CDL2 per taxonomy and their macro average --
from one ``kernels.recon_eval`` launch per batch and a single device->host read, without open3d."""
import json
import math
import os
import time

import numpy as np
import torch

from . import builder
from .runner_pretrain import wrap_ddp, _Single
from ..extensions.chamfer_dist import ChamferDistanceL1, ChamferDistanceL2
from ..utils import dist_utils
from ..utils.AverageMeter import AverageMeter
from ..utils.logger import get_logger, print_log


class Metrics:
    """minimal stand-in for utils/metrics.py Metrics: lower CDL1 is better."""

    def __init__(self, name="CDL1", values=None):
        self.name = name
        # a checkpoint written before the first validation stores an empty dict: that means "no best yet"
        self._values = dict(values) if isinstance(values, dict) and name in values else {"CDL1": float("inf"), "CDL2": float("inf")}

    def better_than(self, other):
        return other is None or self._values[self.name] < other._values[other.name]

    def state_dict(self):
        return dict(self._values)


def kld_weight(config, niter):
    start, target, ntime = config.kldweight.start, config.kldweight.target, config.kldweight.ntime
    _niter = niter - 10000
    if _niter > ntime:
        return target
    if _niter < 0:
        return 0.
    return target + (start - target) * (1. + math.cos(math.pi * float(_niter) / ntime)) / 2.


def compute_loss(loss_1, loss_2, config, niter, train_writer):
    w = kld_weight(config, niter)
    if train_writer is not None:
        train_writer.add_scalar('Loss/Batch/KLD_Weight', w, niter)
    return loss_1 + w * loss_2


def get_temp(config, niter):
    if config.get('temp') is None:
        return 0
    start, target, ntime = config.temp.start, config.temp.target, config.temp.ntime
    if niter > ntime:
        return target
    return target + (start - target) * (1. + math.cos(math.pi * float(niter) / ntime)) / 2.


def train_step(base_model, optimizer, points, config, n_itr, num_iter=1, train_writer=None, draws=None):
    temp = get_temp(config, n_itr)
    module = base_model.module
    ret = base_model(points, temperature=temp, hard=False, draws=draws)
    loss_1, loss_2 = module.get_loss(ret, points)
    loss = compute_loss(loss_1, loss_2, config, n_itr, train_writer)
    loss.backward()
    if num_iter == config.step_per_update:
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
    return loss_1.detach(), loss_2.detach(), temp


@torch.no_grad()
def validate(base_model, test_dataloader, epoch, cdl1, cdl2, args, config, device, logger=None, max_batches=None):
    base_model.eval()
    tot1 = tot2 = 0.0
    n = 0
    for idx, (_, _, data) in enumerate(test_dataloader):
        points = data.to(device)
        ret = base_model(points, temperature=1., hard=True)
        dense = ret[1]
        tot1 += cdl1(dense, points).item() * 1000 * points.shape[0]
        tot2 += cdl2(dense, points).item() * 1000 * points.shape[0]
        n += points.shape[0]
        if max_batches is not None and idx + 1 >= max_batches:
            break
    m = Metrics(config.consider_metric, {"CDL1": tot1 / max(n, 1), "CDL2": tot2 / max(n, 1)})
    print_log('[Validation] EPOCH: %d  Metrics = %s' % (epoch, m.state_dict()), logger=logger)
    return m


def run_net(args, config, train_writer=None, val_writer=None, max_steps=None, log_every=100):
    logger = get_logger(args.log_name)
    (train_sampler, train_dataloader), (_, test_dataloader) = builder.dataset_builder(args, config.dataset.train), \
        builder.dataset_builder(args, config.dataset.val)
    base_model = builder.model_builder(config.model)
    device = torch.device("cuda", args.local_rank % max(1, torch.cuda.device_count()))
    if args.use_gpu:
        torch.cuda.set_device(device)          # every launch goes to the current device's current stream
        base_model.to(device)
    start_epoch, best_metrics, metrics = 0, None, None
    if args.resume:
        start_epoch, best = builder.resume_model(base_model, args, logger=logger)
        best_metrics = Metrics(config.consider_metric, best if isinstance(best, dict) else None)
    elif args.start_ckpts is not None:
        builder.load_model(base_model, args.start_ckpts, logger=logger)
    base_model = wrap_ddp(base_model, args) if args.distributed else _Single(base_model)
    optimizer, scheduler = builder.build_opti_sche(base_model, config)
    cdl1, cdl2 = ChamferDistanceL1(), ChamferDistanceL2()
    if args.resume:
        builder.resume_optimizer(optimizer, args, logger=logger)

    base_model.zero_grad()
    steps, log = 0, []
    for epoch in range(start_epoch, config.max_epoch + 1):
        if args.distributed:
            train_sampler.set_epoch(epoch)
        base_model.train()
        epoch_start = batch_start = time.time()
        batch_time, data_time, losses = AverageMeter(), AverageMeter(), AverageMeter(['Loss1', 'Loss2'])
        num_iter, n_batches, pending = 0, len(train_dataloader), []
        for idx, (taxonomy_ids, model_ids, data) in enumerate(train_dataloader):
            num_iter += 1
            n_itr = epoch * n_batches + idx
            data_time.update(time.time() - batch_start)
            if config.dataset.train._base_.NAME != 'ShapeNet':
                raise NotImplementedError(f'Train phase do not support {config.dataset.train._base_.NAME}')
            points = data.to(device, non_blocking=True)
            l1, l2, temp = train_step(base_model, optimizer, points, config, n_itr, num_iter, train_writer)
            if num_iter == config.step_per_update:
                num_iter = 0
            if args.distributed:
                l1, l2 = dist_utils.reduce_tensor(l1, args), dist_utils.reduce_tensor(l2, args)
            pending.append(torch.stack((l1, l2)))
            steps += 1
            if idx % log_every == 0 or (max_steps is not None and steps >= max_steps):
                for v1, v2 in (torch.stack(pending) * 1000).tolist():          # one host sync per log interval
                    losses.update([v1, v2]); log.append((v1, v2))
                pending = []
                if train_writer is not None:
                    train_writer.add_scalar('Loss/Batch/Loss_1', losses.val(0), n_itr)
                    train_writer.add_scalar('Loss/Batch/Loss_2', losses.val(1), n_itr)
                    train_writer.add_scalar('Loss/Batch/Temperature', temp, n_itr)
                    train_writer.add_scalar('Loss/Batch/LR', optimizer.param_groups[0]['lr'], n_itr)
                batch_time.update(time.time() - batch_start)
                print_log('[Epoch %d/%d][Batch %d/%d] BatchTime = %.3f (s) DataTime = %.3f (s) Losses = %s lr = %.6f' %
                          (epoch, config.max_epoch, idx + 1, n_batches, batch_time.val(), data_time.val(),
                           ['%.4f' % l for l in losses.val()], optimizer.param_groups[0]['lr']), logger=logger)
            batch_start = time.time()
            if max_steps is not None and steps >= max_steps:
                break
        for v1, v2 in ((torch.stack(pending) * 1000).tolist() if pending else []):
            losses.update([v1, v2]); log.append((v1, v2))
        if config.scheduler.type != 'function' and scheduler is not None:
            scheduler.step(epoch)
        print_log('[Training] EPOCH: %d EpochTime = %.3f (s) Losses = %s lr = %.6f' %
                  (epoch, time.time() - epoch_start, ['%.4f' % l for l in losses.avg()], optimizer.param_groups[0]['lr']), logger=logger)
        if getattr(base_model.module, 'emd_loss', None):              # model key ``emd_loss``: the epoch's one read of the capped-solve counter
            capped = int(base_model.module.emd_capped.item())
            if capped > 0:
                print_log('[Training] EPOCH: %d WARNING: emd_loss: the bid cap (max_bids = %d) ended the matching of %d group pairs; their '
                          'term is an upper bound without the N * eps guarantee' % (epoch, base_model.module.emd_loss['max_bids'], capped),
                          logger=logger)
            base_model.module.emd_capped.zero_()
        if epoch % args.val_freq == 0 and epoch != 0:
            metrics = validate(base_model, test_dataloader, epoch, cdl1, cdl2, args, config, device, logger=logger)
            if metrics.better_than(best_metrics):
                best_metrics = metrics
                builder.save_checkpoint(base_model, optimizer, epoch, metrics, best_metrics, 'ckpt-best', args, logger=logger)
        builder.save_checkpoint(base_model, optimizer, epoch, metrics, best_metrics, 'ckpt-last', args, logger=logger)
        if max_steps is not None and steps >= max_steps:
            break
    return log


# ---- evaluation of a trained tokenizer (reference :219-420) ------------------------------------------------------------------------------
LOSS_NAMES = ['SparseLossL1', 'SparseLossL2', 'DenseLossL1', 'DenseLossL2']
SYNSET_DICT = './data/shapenet_synset_dict.json'
USEFUL_CATE = ["02691156", "02818832", "04379243", "04099429", "03948459", "03790512", "03642806", "03467517", "03261776", "03001627",
               "02958343", "03759954"]


def _tax(t):
    return t if isinstance(t, str) else (t.item() if hasattr(t, "item") else t)


def aggregate_rows(rows, taxonomy_ids):
    """host part of the evaluation, float64: ``rows`` [n, RECON_FIELDS] as ``kernels.recon_eval`` wrote them, one taxonomy id per row ->
    dict(losses = mean over samples of the four losses x1000, per_taxonomy = {id: (count, [F-Score, CDL1, CDL2])} in order of first
    appearance, overall = mean over taxonomies of the per-taxonomy means (:282-283))"""
    from .. import kernels as K
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, K.RECON_FIELDS)
    if len(taxonomy_ids) != rows.shape[0]:
        raise ValueError(f"{rows.shape[0]} rows for {len(taxonomy_ids)} taxonomy ids")
    losses = [float(v) for v in rows[:, [K.RECON_SPARSE_L1, K.RECON_SPARSE_L2, K.RECON_DENSE_L1, K.RECON_DENSE_L2]].mean(axis=0) * 1000] \
        if rows.shape[0] else [0.0] * 4
    met = rows[:, [K.RECON_FSCORE, K.RECON_CDL1, K.RECON_CDL2]] * np.array([1.0, 1000.0, 1000.0])
    members = {}
    for i, t in enumerate(taxonomy_ids):
        members.setdefault(t, []).append(i)
    per = {t: (len(ix), [float(v) for v in met[ix].mean(axis=0)]) for t, ix in members.items()}
    overall = [float(v) for v in np.mean([v for _, v in per.values()], axis=0)] if per else [0.0] * 3
    return dict(losses=losses, per_taxonomy=per, overall=overall)


def aggregate_emd(emd_rows, taxonomy_ids):
    """the EMD column of ``evaluate`` (config key ``emd_val``): ``emd_rows`` float64 [n, 2] = (value, info) per cloud as
    ``utils.metrics.emd_distance`` returned them -> dict(values, info, per_taxonomy = {id: mean}, overall = mean over taxonomies of the
    per-taxonomy means like the other columns, capped = clouds whose matching the round cap ended)"""
    emd_rows = np.asarray(emd_rows, dtype=np.float64).reshape(-1, 2)
    members = {}
    for i, t in enumerate(taxonomy_ids):
        members.setdefault(t, []).append(i)
    per = {t: float(emd_rows[ix, 0].mean()) for t, ix in members.items()}
    return dict(values=emd_rows[:, 0].copy(), info=emd_rows[:, 1].astype(np.int64), per_taxonomy=per,
                overall=float(np.mean(list(per.values()))) if per else 0.0, capped=int((emd_rows[:, 1] < 0).sum()))


def results_table(per_taxonomy, overall, names=None, synset=None):
    """the reference's TEST RESULTS table (:292-314) as plain text: Taxonomy | #Sample | metrics | Category, a footing row 'Overall'"""
    from ..utils.metrics import Metrics as FullMetrics
    synset = synset or {}
    table = [['Taxonomy', '#Sample'] + list(names or FullMetrics.names()) + ['Category']]
    for t, (count, vals) in per_taxonomy.items():
        table.append([str(t), str(count)] + ['%.3f' % v for v in vals] + [str(synset.get(t, t))])
    table.append(['Overall', '--'] + ['%.3f' % v for v in overall] + ['--'])
    width = [max(len(r[c]) for r in table) for c in range(len(table[0]))]
    rule = '+' + '+'.join('-' * (w + 2) for w in width) + '+'
    line = lambda r: '| ' + ' | '.join(v.ljust(w) for v, w in zip(r, width)) + ' |'
    out = [rule, line(table[0]), rule] + [line(r) for r in table[1:-1]] + [rule, line(table[-1]), rule]
    return '\n'.join(out)


def _synset_names():
    if os.path.exists(SYNSET_DICT):
        with open(SYNSET_DICT) as f:
            return json.load(f)
    return {}


def gumbel_noise(module, sample_ids, seed, device):
    """[B, num_group, num_tokens] gumbel noise, sample i from its own generator state (seed, i): the draw of a cloud does not depend on the
    batch it is evaluated in, and two passes agree bit for bit"""
    gen = torch.Generator(device=device)
    u = torch.empty(len(sample_ids), module.num_group, module.num_tokens, dtype=torch.float32, device=device)
    for r, i in enumerate(sample_ids):
        gen.manual_seed(((int(seed) & 0x7FFFFFFF) << 32) | (int(i) & 0xFFFFFFFF))          # distinct for every (seed, i) below 2^31 / 2^32
        u[r].exponential_(generator=gen)
    return -u.log()


@torch.no_grad()
def eval_batch(module, points, out, row0, seed=0, th=0.01):
    """the per-batch part of ``evaluate`` (no host synchronisation): eval-mode forward with ``hard=True`` on device-resident ``points``
    [B,N,3], rows [row0, row0 + B) of ``out`` from one ``kernels.recon_eval`` launch.  Returns the model's output tuple."""
    from .. import kernels as K
    from ..utils.draws import Draws
    B = points.shape[0]
    noise = gumbel_noise(module, range(row0, row0 + B), seed, points.device)
    ret = module(points, temperature=1., hard=True, draws=Draws({"gumbel": noise}))
    K.recon_eval(ret[0], ret[1], points, out, row0, th)
    return ret


@torch.no_grad()
def evaluate(base_model, test_dataloader, epoch, args, config, logger=None, val_writer=None, batch_size=None, seed=0, max_batches=None):
    """the reference's ``validate`` (:219-323) with batched forwards: the model runs in eval mode with ``hard=True`` (every layer is per-sample
    there), the gumbel noise of sample i is a function of (seed, i), each batch is one ``kernels.recon_eval`` launch into a
    [len(dataset), RECON_FIELDS] device buffer, and that buffer is read ONCE after the last batch; the averages are taken in float64 on the
    host.  ``batch_size``: None keeps the loader's, else the loader's dataset is walked in that batch size.

    Returns ``utils.metrics.Metrics(config.consider_metric, overall)``, overall = mean over taxonomies of the per-taxonomy means.  The details
    ride on the returned object as attributes: ``per_taxonomy`` {id: (count, [F-Score, CDL1, CDL2])}, ``losses`` (the four mean losses x1000),
    ``rows`` (float64 ndarray [samples, RECON_FIELDS]) and ``taxonomy_ids`` / ``model_ids`` (one per row).

    Config key ``emd_val: True`` (or ``emd_val: {eps: ...}``) adds the Earth Mover's Distance of (dense, gt) per cloud
    (``utils.metrics.emd_distance``: the dense output is first reduced to the ground truth's count by farthest-point sampling): a column
    ``EMD`` in the table and its footing row, writer key ``Metric/EMD``, and ``emd`` on the returned object (``aggregate_emd``).  The values
    stay on the device and come to the host in the same single read; the returned ``Metrics`` values are the three they always were."""
    from .. import kernels as K
    from ..utils.metrics import Metrics as FullMetrics
    print_log(f"[VALIDATION] Start validating epoch {epoch}", logger=logger)
    base_model.eval()
    module = builder._unwrap(base_model)
    device = next(module.parameters()).device
    if batch_size is not None and batch_size != test_dataloader.batch_size:
        test_dataloader = torch.utils.data.DataLoader(test_dataloader.dataset, batch_size=int(batch_size), shuffle=False, drop_last=False,
                                                      num_workers=int(getattr(args, "num_workers", 0)), pin_memory=True)
    section = config.dataset.get('test', None) or config.dataset.val
    if section._base_.NAME != 'ShapeNet':
        raise NotImplementedError(f'Train phase do not support {section._base_.NAME}')
    n_samples = len(test_dataloader.dataset)
    out = torch.zeros(n_samples, K.RECON_FIELDS, dtype=torch.float64, device=device)
    emd_val = config.get('emd_val', None)                             # opt-in: True or {eps: ...}; absent or false: nothing below runs
    if emd_val:
        from ..utils.metrics import emd_distance
        emd_eps = emd_val.get('eps', None) if isinstance(emd_val, dict) else None
        emd_out = torch.zeros(n_samples, 2, dtype=torch.float64, device=device)          # per cloud: value, info
    taxonomy_ids, model_ids, row0 = [], [], 0
    for idx, (tax, mids, data) in enumerate(test_dataloader):
        points = data.to(device, non_blocking=True)
        ret = eval_batch(module, points, out, row0, seed)
        if emd_val:
            v, info = emd_distance(ret[1], points, emd_eps)
            emd_out[row0:row0 + points.shape[0], 0] = v
            emd_out[row0:row0 + points.shape[0], 1] = info
        taxonomy_ids += [_tax(t) for t in tax]
        model_ids += [_tax(m) for m in mids]
        row0 += points.shape[0]
        if max_batches is not None and idx + 1 >= max_batches:
            break
    if emd_val:
        rows = torch.cat([out[:row0], emd_out[:row0]], dim=1).cpu().numpy()          # still the one device -> host read
        rows, emd_rows = np.ascontiguousarray(rows[:, :K.RECON_FIELDS]), rows[:, K.RECON_FIELDS:]
    else:
        rows = out[:row0].cpu().numpy()                               # the one device -> host read
    agg = aggregate_rows(rows, taxonomy_ids)
    names, per_taxonomy, overall = FullMetrics.names(), agg["per_taxonomy"], agg["overall"]
    if emd_val:
        emd = aggregate_emd(emd_rows, taxonomy_ids)
        names = names + ['EMD']
        per_taxonomy = {t: (c, v + [emd["per_taxonomy"][t]]) for t, (c, v) in per_taxonomy.items()}
        overall = overall + [emd["overall"]]
        if emd["capped"]:
            print_log('[Validation] EMD: the round cap ended the matching of %d of %d clouds; their values are upper bounds without the '
                      'N * eps guarantee' % (emd["capped"], row0), logger=logger)
    for i in range(1999, row0, 2000):
        r = rows[i]
        print_log('Test[%d/%d] Taxonomy = %s Sample = %s Losses = %s Metrics = %s' %
                  (i + 1, n_samples, taxonomy_ids[i], model_ids[i], ['%.4f' % (l * 1000) for l in r[:4]],
                   ['%.4f' % m for m in (r[K.RECON_FSCORE], r[K.RECON_CDL1] * 1000, r[K.RECON_CDL2] * 1000)]), logger=logger)
    print_log('[Validation] EPOCH: %d  Metrics = %s' % (epoch, ['%.4f' % m for m in agg["overall"]]), logger=logger)
    print_log('============================ TEST RESULTS ============================', logger=logger)
    print_log('\n' + results_table(per_taxonomy, overall, names, _synset_names()), logger=logger)
    if val_writer is not None:
        val_writer.add_scalar('Loss/Epoch/Sparse', agg["losses"][0], epoch)
        val_writer.add_scalar('Loss/Epoch/Dense', agg["losses"][2], epoch)
        for name, v in zip(names, overall):
            val_writer.add_scalar('Metric/%s' % name, v, epoch)
    m = FullMetrics(config.consider_metric, list(agg["overall"]))
    m.per_taxonomy, m.losses, m.rows, m.taxonomy_ids, m.model_ids = agg["per_taxonomy"], agg["losses"], rows, taxonomy_ids, model_ids
    if emd_val:
        m.emd = emd                                                   # not a Metrics item: better_than / state_dict do not see it
    return m


def _load_for_test(args, config, logger):
    print_log('Tester start ... ', logger=logger)
    if args.distributed:
        raise NotImplementedError()
    _, test_dataloader = builder.dataset_builder(args, config.dataset.test)
    base_model = builder.model_builder(config.model)
    builder.load_model(base_model, args.ckpts, logger=logger)
    if args.use_gpu:
        device = torch.device("cuda", args.local_rank % max(1, torch.cuda.device_count()))
        torch.cuda.set_device(device)
        base_model.to(device)
    return base_model, test_dataloader


def validate_net(args, config):
    """evaluate the checkpoint ``args.ckpts`` on ``config.dataset.test`` (reference :325-344); returns what ``evaluate`` returns"""
    logger = get_logger(args.log_name)
    base_model, test_dataloader = _load_for_test(args, config, logger)
    return evaluate(base_model, test_dataloader, 0, args, config, logger=logger)


def _plot(path, gt, dense):
    """gt | reconstruction scatter plot; returns False when matplotlib is not installed"""
    try:
        from matplotlib.figure import Figure
        from matplotlib.backends.backend_agg import FigureCanvasAgg
    except ImportError:
        return False
    fig = Figure(figsize=(8, 4))
    FigureCanvasAgg(fig)
    for k, (pts, title) in enumerate(((gt, 'gt'), (dense, 'dense'))):
        ax = fig.add_subplot(1, 2, k + 1, projection='3d')
        ax.scatter(pts[:, 0], pts[:, 2], pts[:, 1], s=1, c=pts[:, 0], cmap='jet')
        ax.set_axis_off()
        ax.set_title(title)
    fig.savefig(path)
    return True


@torch.no_grad()
def test(base_model, test_dataloader, args, config, logger=None, target='./vis', seed=0):
    """reference :363-420: for the clouds of ``USEFUL_CATE``, write ``<target>/<taxonomy>_<idx>/gt.txt`` and ``dense_points.txt``
    (np.savetxt, delimiter ';') and ``plot.png`` when matplotlib imports; idx is the sample's index in the loader's order, and the walk
    stops after the first written sample with idx > 1000.  Returns the directories written."""
    from ..utils.draws import Draws
    base_model.eval()
    module = builder._unwrap(base_model)
    device = next(module.parameters()).device
    if config.dataset.test._base_.NAME != 'ShapeNet':
        raise NotImplementedError(f'Train phase do not support {config.dataset.test._base_.NAME}')
    written, row0 = [], 0
    for tax, _, data in test_dataloader:
        B = data.shape[0]
        tax = [_tax(t) for t in tax]
        if any(t in USEFUL_CATE for t in tax):
            points = data.to(device)
            noise = gumbel_noise(module, range(row0, row0 + B), seed, device)
            dense = module(points, temperature=1., hard=True, draws=Draws({"gumbel": noise}))[1].cpu().numpy()
            gt = points.cpu().numpy()
            for r in range(B):
                if tax[r] not in USEFUL_CATE:
                    continue
                idx = row0 + r
                data_path = os.path.join(target, f'{tax[r]}_{idx}')
                os.makedirs(data_path, exist_ok=True)
                np.savetxt(os.path.join(data_path, 'gt.txt'), gt[r], delimiter=';')
                np.savetxt(os.path.join(data_path, 'dense_points.txt'), dense[r], delimiter=';')
                _plot(os.path.join(data_path, 'plot.png'), gt[r], dense[r])
                written.append(data_path)
                if idx > 1000:
                    return written
        row0 += B
    return written


def test_net(args, config, target='./vis'):
    """write the reconstructions of the checkpoint ``args.ckpts`` for the reference's category list (reference :346-361)"""
    logger = get_logger(args.log_name)
    base_model, test_dataloader = _load_for_test(args, config, logger)
    return test(base_model, test_dataloader, args, config, logger=logger, target=target)
