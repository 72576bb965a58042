"""Stage-I reconstruction metrics (reference: utils/metrics.py): F-Score@0.01, CDL1, CDL2 (the Chamfer distances with ``ignore_zeros``, x1000),
with the reference's ``Metrics`` surface.  The values come from one ``kernels.recon_eval`` launch per batch instead of open3d KD-tree queries
on the host and two Chamfer calls per cloud; ``Metrics.get`` needs CUDA tensors like every other op of this package."""
import logging

import torch


class Metrics(object):
    # name, direction and the value a Metrics object holds before anything was measured; 'field' / 'scale': where kernels.recon_eval puts the
    # per-cloud value and the factor the reference reports it with
    ITEMS = [
        {'name': 'F-Score', 'enabled': True, 'is_greater_better': True, 'init_value': 0, 'field': 'RECON_FSCORE', 'scale': 1.0},
        {'name': 'CDL1', 'enabled': True, 'is_greater_better': False, 'init_value': 32767, 'field': 'RECON_CDL1', 'scale': 1000.0},
        {'name': 'CDL2', 'enabled': True, 'is_greater_better': False, 'init_value': 32767, 'field': 'RECON_CDL2', 'scale': 1000.0},
    ]

    @classmethod
    def items(cls):
        return [i for i in cls.ITEMS if i['enabled']]

    @classmethod
    def names(cls):
        return [i['name'] for i in cls.items()]

    @classmethod
    def _rows(cls, pred, gt, th=0.01):
        """float64 host rows [B, RECON_FIELDS] of (pred, gt).  The kernel's coarse slot gets the first point of every prediction: its two
        scans are then 2 * N evaluations per cloud and its fields are not used here."""
        from .. import kernels as K
        out = torch.empty(gt.shape[0], K.RECON_FIELDS, dtype=torch.float64, device=gt.device)
        K.recon_eval(pred[:, :1].contiguous(), pred, gt, out, 0, th)
        return out.cpu()

    @classmethod
    def _mean(cls, rows, item):
        from .. import kernels as K
        return float(rows[:, getattr(K, item['field'])].mean()) * item['scale']

    @classmethod
    def get(cls, pred, gt):
        """[F-Score, CDL1, CDL2] of a batch: the mean over its clouds of the per-cloud values.  For one cloud this is the reference's value.
        For a batch the reference averages the F-Score the same way but computes CDL1 / CDL2 over the whole batch WITHOUT removing zero
        points (its ``ignore_zeros`` only acts at batch size 1); here every cloud is evaluated as the reference evaluates a single one."""
        rows = cls._rows(pred, gt)
        return [cls._mean(rows, item) for item in cls.items()]

    @classmethod
    def _get_f_score(cls, pred, gt, th=0.01):
        return cls._mean(cls._rows(pred, gt, th), cls.ITEMS[0])

    @classmethod
    def _get_chamfer_distancel1(cls, pred, gt):
        return cls._mean(cls._rows(pred, gt), cls.ITEMS[1])

    @classmethod
    def _get_chamfer_distancel2(cls, pred, gt):
        return cls._mean(cls._rows(pred, gt), cls.ITEMS[2])

    def __init__(self, metric_name, values):
        """``values``: a list in the order of ``names()``, or a dict by name (names missing from it keep their initial value: checkpoints of
        ``run_net`` hold CDL1 / CDL2 only)"""
        self._items = Metrics.items()
        self.metric_name = metric_name
        if isinstance(values, list):
            self._values = values
        elif isinstance(values, dict):
            known = [item['name'] for item in self._items]
            for k in values:
                if k not in known:
                    logging.warning('Metrics: %r is not one of %s and is dropped' % (k, known))
            self._values = [values.get(item['name'], item['init_value']) for item in self._items]
        else:
            raise TypeError('Metrics takes a list or a dict of values, not %s' % type(values).__name__)

    def state_dict(self):
        return {item['name']: self._values[i] for i, item in enumerate(self._items)}

    def __repr__(self):
        return str(self.state_dict())

    def better_than(self, other):
        if other is None:
            return True
        for i, item in enumerate(self._items):
            if item['name'] == self.metric_name:
                break
        else:
            raise ValueError('Metrics: no metric named %r to compare by' % (self.metric_name,))
        return self._values[i] > other._values[i] if item['is_greater_better'] else self._values[i] < other._values[i]
