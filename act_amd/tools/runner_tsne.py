"""t-SNE of classifier features (reference: tools/runner_tsne.py:29-142, ``tsne_net``): a pretrained and a finetuned PointTransformer, the
``concat_f`` feature of every test cloud, OA / mAcc of the finetuned model, and the embedding of the correctly classified clouds of each
model as ``./tsne/<name>_pretrained.png`` and ``./tsne/<name>_finetuned.png``.

Device-first differences:
  * the embedding is utils.tsne.TSNE -- the exact objective on the device (csrc/tsne.hip) -- where the reference calls openTSNE; features and
    predictions stay on the device until the plot;
  * ``model.forward_features(points)`` returns (logits, concat_f); the reference calls ``model(points, True)``, which its own forward does
    not accept;
  * the two checkpoints come from ``args.ckpts_pretrained`` / ``args.ckpts_finetuned`` (defaults: the reference's hard-coded paths; ``none``
    skips loading, loudly);
  * the reference's trailing 300-round voting loop is left out: runner_finetune.test offers voting.
"""
import os
import warnings

import torch

from . import builder
from .runner_finetune import accuracy_scores, sampled_batches
from ..utils import tsne_utils
from ..utils.logger import get_logger, print_log
from ..utils.tsne import TSNE

CKPT_PRETRAINED = "model_zoo/ckpt-last-vitb-m0.8-d384-dec2.pth"
CKPT_FINETUNED = "model_zoo/act-hard-ckpt-best-88.21.pth"


def _load(model, path, what, logger):
    if path is None or str(path).lower() in ("none", ""):
        warnings.warn(f"tsne_net: ckpts_{what} is 'none' -- the {what} model is RANDOMLY INITIALISED; its features and its accuracy mean nothing "
                      "beyond a smoke run.", stacklevel=3)
        print_log(f'[TSNE] ckpts_{what}: none -> randomly initialised {what} model', logger=logger)
        return
    model.load_model_from_ckpt(path)


def tsne_net(args, config):
    logger = get_logger(args.log_name)
    print_log('Tester start ... ', logger=logger)
    _, test_dataloader = builder.dataset_builder(args, config.dataset.test)
    pretrained_model = builder.model_builder(config.model_pretrained)
    finetuned_model = builder.model_builder(config.model_finetuned)
    _load(pretrained_model, getattr(args, "ckpts_pretrained", CKPT_PRETRAINED), "pretrained", logger)
    _load(finetuned_model, getattr(args, "ckpts_finetuned", CKPT_FINETUNED), "finetuned", logger)
    dev = torch.device("cuda", args.local_rank % max(1, torch.cuda.device_count()))
    pretrained_model.to(dev)
    finetuned_model.to(dev)
    if args.distributed:
        raise NotImplementedError()
    return tsne(pretrained_model, finetuned_model, test_dataloader, args, config, logger=logger)


def tsne(pretrained_model, finetuned_model, test_dataloader, args, config, logger=None):
    """-> dict(acc, acc_avg, n_correct, files, kl): the accuracies of the finetuned model, the rows embedded, the two files written and the final
    KL divergence of the two embeddings"""
    perplexity = getattr(args, "perplexity", None) or config.get("tsne_perplexity", 25)
    embed = TSNE(perplexity=perplexity, learning_rate="auto", metric="cosine")
    pretrained_model.eval()
    finetuned_model.eval()
    dev = next(finetuned_model.parameters()).device
    feat_p, feat_f, test_pred, test_label = [], [], [], []
    with torch.no_grad():
        for points, label in sampled_batches(test_dataloader, config.npoints, dev):
            _, fp = pretrained_model.forward_features(points)
            logits_f, ff = finetuned_model.forward_features(points)
            feat_p.append(fp)
            feat_f.append(ff)
            test_pred.append(logits_f.argmax(-1).view(-1))
            test_label.append(label.view(-1))
        feat_p, feat_f = torch.cat(feat_p, dim=0), torch.cat(feat_f, dim=0)
        test_pred, test_label = torch.cat(test_pred, dim=0), torch.cat(test_label, dim=0)
        acc, acc_avg = accuracy_scores(test_label, test_pred)
        print_log('[TEST] OA=%.4f  mAcc=%.4f' % (acc, acc_avg), logger=logger)
        correct = test_pred == test_label
        labels = test_label[correct]
        name = getattr(args, "tsne_name", None) or str(config.dataset.test._base_.NAME).lower()
        target = getattr(args, "tsne_dir", None) or "./tsne"
        files, kls = [], []
        for feats, which in ((feat_p, "pretrained"), (feat_f, "finetuned")):
            emb = embed.fit(feats[correct].contiguous())
            kls.append(embed.kl_divergence_)
            print_log('[TSNE] %s: %d points, KL = %.4f' % (which, emb.shape[0], kls[-1]), logger=logger)
            files.append(tsne_utils.plot_tsne(emb, labels, filename=os.path.join(target, f"{name}_{which}.png")))
    return dict(acc=acc, acc_avg=acc_avg, n_correct=int(labels.numel()), files=files, kl=kls)
