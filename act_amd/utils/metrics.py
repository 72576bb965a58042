"""Stage-I reconstruction metrics (reference: utils/metrics.py): F-Score@0.01, CDL1, CDL2 (the Chamfer distances with ``ignore_zeros``, x1000),
with the reference's ``Metrics`` surface.  The values come from one ``kernels.recon_eval`` launch per batch instead of open3d KD-tree queries
on the host and two Chamfer calls per cloud; ``Metrics.get`` needs CUDA tensors like every other op of this package.

``emd_distance`` is the opt-in second reconstruction distance (extensions/emd); it is not one of ``Metrics.ITEMS``."""
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


def emd_distance(pred, gt, eps=None):
    """Earth Mover's Distance of every cloud of a batch, on the scale CDL1 is reported on: (values, info) with values a float64 device tensor
    [B] of mean_i sqrt(dist_i) * 1000 over the one-to-one matching of ``extensions.emd`` (sum of squared distances within N * eps of the
    optimum), and info the int32 device tensor [B] of that solve (rounds used, negative when the round cap was hit).  Nothing is read on the
    host.  ``eps``: None -> ``extensions.emd.DEFAULT_EPS``.

    The matching needs clouds of one size.  When ``pred`` has more points than ``gt`` (Stage-I: dense 2,048 against 1,024) it is first reduced
    to ``gt``'s count by farthest-point sampling from index 0 (``misc.fps``).  That rule is this project's own protocol, not the reference's,
    which has no EMD; fewer points than ``gt`` raise ValueError."""
    from ..extensions.emd import DEFAULT_EPS, emd_cuda
    n, m = pred.shape[1], gt.shape[1]
    if n < m:
        raise ValueError(f"emd_distance: the prediction has {n} points and the ground truth {m}; a prediction is only ever reduced")
    if n > m:
        from .misc import fps
        pred = fps(pred.detach(), m)
    dist, _, info = emd_cuda.forward(pred.detach(), gt, DEFAULT_EPS if eps is None else eps)
    return dist.double().sqrt().mean(dim=1) * 1000.0, info
