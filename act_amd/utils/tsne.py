"""Exact t-SNE on device tensors: the objective openTSNE's ``TSNE(metric="cosine")`` minimises (perplexity-based kNN affinities with
k = min(N - 1, 3 perplexity), early exaggeration, gains and momentum, gradient without the factor 4), with the repulsive term and Z summed over
ALL pairs every iteration by csrc/tsne.hip instead of Barnes-Hut / FFT interpolation.  Deterministic: two fits of one input are bit-identical.

Used by tools.runner_tsne.tsne_net (reference: tools/runner_tsne.py:74-142); openTSNE and sklearn are not needed.
"""
import torch

from .. import _C
from .. import kernels as K


class TSNE:
    """``fit(features float32 [N,D])`` on a CUDA tensor -> embedding float32 [N,2] on the device.  After a fit: ``kl_divergence_`` (float),
    ``affinities_`` (the CSR triple indptr, indices, values of P), ``n_iter_``.  ``learning_rate="auto"`` is max(200, N / 12);
    ``initialization`` is ``"pca"`` or a [N,2] tensor.  Only ``metric="cosine"``; a feature row of zero norm is at distance 1 from every row."""

    def __init__(self, perplexity=30, early_exaggeration=12, early_exaggeration_iter=250, n_iter=500, initial_momentum=0.5, final_momentum=0.8,
                 learning_rate="auto", initialization="pca", metric="cosine"):
        if metric != "cosine":
            raise _C.ActHipError(f"TSNE: metric {metric!r} is not supported (only 'cosine')")
        self.perplexity, self.early_exaggeration = float(perplexity), float(early_exaggeration)
        self.early_exaggeration_iter, self.n_iter = int(early_exaggeration_iter), int(n_iter)
        self.initial_momentum, self.final_momentum = float(initial_momentum), float(final_momentum)
        self.learning_rate, self.initialization, self.metric = learning_rate, initialization, metric

    def fit(self, features):
        if not (torch.is_tensor(features) and features.is_cuda):
            raise _C.ActHipError("act_amd kernels run on the GPU only (got a CPU tensor); there is no CPU fallback")
        if features.dim() != 2 or features.dtype != torch.float32:
            raise _C.ActHipError(f"TSNE.fit: features must be float32 [N, D], got {tuple(features.shape)} {features.dtype}")
        N = features.shape[0]
        if N < 4:
            raise _C.ActHipError(f"TSNE.fit: {N} rows (needs at least 4)")
        if not self.perplexity >= 1:
            raise _C.ActHipError(f"TSNE.fit: perplexity {self.perplexity} (needs >= 1)")
        x = features.contiguous()
        if not bool(torch.isfinite(x).all()):
            raise _C.ActHipError("TSNE.fit: features contain NaN or infinity")
        k = min(N - 1, int(3 * self.perplexity))
        if k > K.TSNE_MAX_NEIGHBORS:
            raise _C.ActHipError(f"TSNE.fit: perplexity {self.perplexity} needs {k} neighbours (supported: {K.TSNE_MAX_NEIGHBORS})")
        init = self.initialization
        if torch.is_tensor(init):
            if not init.is_cuda or tuple(init.shape) != (N, 2) or init.dtype != torch.float32:
                raise _C.ActHipError(f"TSNE.fit: initialization must be a float32 [{N}, 2] tensor on the device")
            Y = init.clone().contiguous()
        elif init == "pca":
            Y = K.tsne_pca_init(x)
        else:
            raise _C.ActHipError(f"TSNE.fit: initialization {init!r} (supported: 'pca' or a tensor)")
        lr = max(200.0, N / 12.0) if self.learning_rate == "auto" else float(self.learning_rate)
        idx, dist = K.tsne_knn_cosine(x, k)
        p = K.tsne_conditional_p(dist, self.perplexity)
        csr = K.tsne_symmetrize(idx, p)
        update, gains = torch.zeros_like(Y), torch.ones_like(Y)
        if self.early_exaggeration_iter > 0:
            K.tsne_steps(csr, Y, update, gains, self.early_exaggeration_iter, self.early_exaggeration, self.initial_momentum, lr)
        if self.n_iter > 0:
            K.tsne_steps(csr, Y, update, gains, self.n_iter, 1.0, self.final_momentum, lr)
        self.affinities_, self.n_iter_, self.learning_rate_ = csr, self.early_exaggeration_iter + self.n_iter, lr
        self.embedding_ = Y
        self.kl_divergence_ = float(K.tsne_kl(csr, Y))
        return Y
