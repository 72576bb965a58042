"""Weighted k-nearest-neighbour classifier on device tensors: the probe of Wu et al. 2018 ("Unsupervised Feature Learning via Non-Parametric
Instance Discrimination") that DINO's eval_knn uses.  The k most similar bank rows under the cosine similarity vote for their class with weight
exp(sim / T); no solver, no tolerance, nothing to search.  Search and vote are the kernels of csrc/knn_probe.hip.

Used by tools.runner_pretrain.validate (config key ``knn_val``).
"""
import torch

from .. import _C
from .. import kernels as K


class KNNClassifier:
    """``fit(features float32 [N,D], labels int [N])`` on CUDA tensors keeps the bank; ``classes_`` are the sorted unique labels (a device tensor), as
    LinearSVC's.  ``k``: an int or an ascending list (every list for a smaller k is a prefix of the one for the largest); ``predict`` uses the
    first.  Ties: neighbours towards the lower bank index, classes towards the lower class."""

    def __init__(self, k=20, T=0.07, normalize=True):
        ks = [k] if isinstance(k, int) else list(k)
        if not ks or any(not isinstance(v, int) or isinstance(v, bool) for v in ks) or ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])):
            raise _C.ActHipError(f"KNNClassifier: k must be a positive int or an ascending list of them, got {k!r}")
        if ks[-1] > K.KNN_PROBE_MAX_K:
            raise _C.ActHipError(f"KNNClassifier: k = {ks[-1]} exceeds the supported {K.KNN_PROBE_MAX_K}")
        if len(ks) > K.KNN_PROBE_MAX_KS:
            raise _C.ActHipError(f"KNNClassifier: {len(ks)} values of k (supported: {K.KNN_PROBE_MAX_KS})")
        if not float(T) > 0:
            raise _C.ActHipError(f"KNNClassifier: T must be positive, got {T!r}")
        self.ks, self.T, self.normalize = ks, float(T), bool(normalize)

    @staticmethod
    def _features(x, name):
        if not (torch.is_tensor(x) and x.is_cuda):
            raise _C.ActHipError("act_amd kernels run on the GPU only (got a CPU tensor); there is no CPU fallback")
        if x.dim() != 2 or x.dtype != torch.float32:
            raise _C.ActHipError(f"KNNClassifier.{name}: features must be float32 [N, D], got {tuple(x.shape)} {x.dtype}")
        return x.contiguous()

    @staticmethod
    def _labels(y, n, name):
        if not (torch.is_tensor(y) and y.is_cuda):
            raise _C.ActHipError("act_amd kernels run on the GPU only (got a CPU tensor); there is no CPU fallback")
        if y.dim() != 1 or y.numel() != n or y.dtype.is_floating_point or y.dtype == torch.bool:
            raise _C.ActHipError(f"KNNClassifier.{name}: labels must be {n} integers, got {tuple(y.shape)} {y.dtype}")
        return y.to(torch.int64).contiguous()

    def fit(self, features, labels):
        x = self._features(features, "fit")
        y = self._labels(labels, x.shape[0], "fit")
        classes, inverse = torch.unique(y, return_inverse=True)          # sorted; its length is the one host read of fit
        if classes.numel() > K.KNN_PROBE_MAX_CLASSES:
            raise _C.ActHipError(f"KNNClassifier.fit: {classes.numel()} classes in the labels (supported: 1 .. {K.KNN_PROBE_MAX_CLASSES})")
        self.bank_, self.classes_, self.bank_cls_ = x, classes, inverse.to(torch.int32).contiguous()
        return self

    def _search(self, x, k, exclude_self, name):
        x = self._features(x, name)
        if x.shape[1] != self.bank_.shape[1]:
            raise _C.ActHipError(f"KNNClassifier.{name}: features have width {x.shape[1]}, the bank has {self.bank_.shape[1]}")
        room = self.bank_.shape[0] - bool(exclude_self)
        if k > room:
            raise _C.ActHipError(f"KNNClassifier.{name}: k = {k} exceeds the {room} bank rows a query may select "
                                 f"({self.bank_.shape[0]} rows, exclude_self = {bool(exclude_self)})")
        if exclude_self and x.shape[0] != self.bank_.shape[0]:
            raise _C.ActHipError(f"KNNClassifier.{name}: exclude_self needs the bank itself as the queries, got {x.shape[0]} rows for "
                                 f"{self.bank_.shape[0]}")
        return K.knn_probe_search(x, self.bank_, k, normalize=self.normalize, exclude_self=exclude_self)

    def kneighbors(self, x, exclude_self=False):
        """(sim [N, max k], idx int32 [N, max k]) of the bank rows, best first"""
        return self._search(x, self.ks[-1], exclude_self, "kneighbors")

    def _class_index(self, y):
        """position of every label in classes_, -1 for a label the bank does not have"""
        pos = torch.searchsorted(self.classes_, y).clamp_(max=self.classes_.numel() - 1)
        return torch.where(self.classes_[pos] == y, pos, torch.full_like(pos, -1)).to(torch.int32)

    def predict(self, x, exclude_self=False):
        """labels [N] voted by the first k"""
        sim, idx = self._search(x, self.ks[0], exclude_self, "predict")
        _, pred, _ = K.knn_probe_vote(sim, idx, self.bank_cls_, self.classes_.numel(), self.ks[:1], self.T, want_scores=False)
        return self.classes_[pred[:, 0]]

    def score(self, x, y, ks=None, topk=(1, 5), exclude_self=False):
        """{"knn@k": top-1 accuracy in percent, "knn@k/top5": top-5} for every k of ``ks`` (default: the classifier's); the counts are summed on the
        device in integers and read once"""
        ks = self.ks if ks is None else ([ks] if isinstance(ks, int) else list(ks))
        topk = tuple(topk)
        if not set(topk) <= {1, 5} or not topk:
            raise _C.ActHipError(f"KNNClassifier.score: topk = {topk!r} (supported: 1 and 5)")
        if not ks or any(b <= a for a, b in zip(ks, ks[1:])) or ks[0] < 1 or ks[-1] > K.KNN_PROBE_MAX_K:
            raise _C.ActHipError(f"KNNClassifier.score: ks = {ks!r} must be ascending values in 1 .. {K.KNN_PROBE_MAX_K}")
        sim, idx = self._search(x, ks[-1], exclude_self, "score")
        q_cls = self._class_index(self._labels(y, sim.shape[0], "score"))
        _, _, counts = K.knn_probe_vote(sim, idx, self.bank_cls_, self.classes_.numel(), ks, self.T, q_cls=q_cls, want_scores=False)
        counts = counts.tolist()                                           # the one read
        out = {}
        for j, k in enumerate(ks):
            if 1 in topk:
                out[f"knn@{k}"] = counts[j][0] * 100. / sim.shape[0]
            if 5 in topk:
                out[f"knn@{k}/top5"] = counts[j][1] * 100. / sim.shape[0]
        return out
