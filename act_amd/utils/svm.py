"""Linear SVM on device tensors: what sklearn.svm.LinearSVC() computes (liblinear's L2-regularised L2-loss SVC, C = 1, one-vs-rest, the
intercept regularised as an appended constant feature), solved for all classes together by the batched Newton-CG of csrc/svm.hip.

Used by tools.runner_pretrain.validate (reference: tools/runner_pretrain.py:47-51); sklearn is not needed.
"""
import torch

from .. import _C
from .. import kernels as K


class LinearSVC:
    """``fit(features float32 [N,D], labels int [N])`` on CUDA tensors.  Attributes as sklearn's: ``classes_`` (sorted unique labels, a device
    tensor), ``coef_`` [K,D], ``intercept_`` [K], ``n_iter_`` (most Newton steps any class took).  Two classes keep both one-vs-rest rows (they are
    mirror images), where sklearn keeps one.  ``status_`` [K]: 1 = gradient norm under ``tol``, 2 = ended on no progress, 0 = ``max_newton`` reached."""

    def __init__(self, C=1.0, tol=1e-4, max_newton=60, max_cg=60):
        self.C, self.tol, self.max_newton, self.max_cg = float(C), float(tol), int(max_newton), int(max_cg)

    def fit(self, features, labels):
        if not (torch.is_tensor(features) and torch.is_tensor(labels) and features.is_cuda and labels.is_cuda):
            raise _C.ActHipError("act_amd kernels run on the GPU only (got a CPU tensor); there is no CPU fallback")
        if features.dim() != 2 or features.dtype != torch.float32:
            raise _C.ActHipError(f"LinearSVC.fit: features must be float32 [N, D], got {tuple(features.shape)} {features.dtype}")
        if labels.dim() != 1 or labels.numel() != features.shape[0] or labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise _C.ActHipError(f"LinearSVC.fit: labels must be {features.shape[0]} integers, got {tuple(labels.shape)} {labels.dtype}")
        x = features.contiguous()
        y = labels.to(torch.int64).contiguous()
        classes = torch.unique(y)                       # sorted; its length is the first of the host reads
        k = classes.numel()
        if k < 2 or k > K.SVM_MAX_CLASSES:
            raise _C.ActHipError(f"LinearSVC.fit: {k} classes in the labels (supported: 2 .. {K.SVM_MAX_CLASSES})")
        W = torch.zeros(k, x.shape[1], dtype=torch.float32, device=x.device)
        b = torch.zeros(k, dtype=torch.float32, device=x.device)
        istate, dstate = K.svm_state(k, x.device)
        for _ in range(self.max_newton):
            K.svm_newton(x, y, classes, W, b, istate, dstate, self.C, self.tol, self.max_cg)
            if all(istate[0].tolist()):                 # the one read of an iteration: K flags
                break
        self.classes_, self.coef_, self.intercept_ = classes, W, b
        st = istate.cpu()
        self.status_ = st[0]
        self.n_iter_ = int(st[1].max())
        self.n_cg_ = int(st[2].max())
        self.objective_, self.grad_norm_ = dstate[0], dstate[1]     # at the start of the last iteration each class ran
        return self

    def decision_function(self, features):
        return K.svm_scores(features, self.coef_, self.intercept_)

    def predict(self, features):
        """classes_[argmax of the scores]; ties go to the lowest class index"""
        s = self.decision_function(features)
        top = s.max(dim=1, keepdim=True).values
        cols = torch.arange(s.shape[1], device=s.device).expand_as(s)
        first = torch.where(s == top, cols, torch.full_like(cols, s.shape[1])).min(dim=1).values
        first.clamp_(max=s.shape[1] - 1)                 # a row of NaN scores has no maximum: keep the index inside classes_
        return self.classes_[first]
