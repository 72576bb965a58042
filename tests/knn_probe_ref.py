"""float64 torch oracle of the weighted k-NN probe (csrc/knn_probe.hip, utils/knn_probe.py): normalise, the FULL similarity matrix, a stable
sort by (-similarity, bank index), the vote.  Everything on the CPU; inputs are the fp32 tensors the device gets, promoted to float64."""
import torch


def normalize(x):
    x = x.double()
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)


def similarities(q, bank, normalize_rows=True, exclude_self=False):
    """float64 [Nq, Nb]; exclude_self puts -inf on the diagonal (so the excluded row sorts last)"""
    q, bank = (normalize(q), normalize(bank)) if normalize_rows else (q.double(), bank.double())
    sim = q @ bank.t()
    if exclude_self:
        assert sim.shape[0] == sim.shape[1]
        sim.fill_diagonal_(float("-inf"))
    return sim


def search(q, bank, k, normalize_rows=True, exclude_self=False):
    """(sim float64 [Nq,k], idx int64 [Nq,k]): larger similarity first, then lower bank index (the stable sort of -sim keeps the index order
    of equal keys)"""
    sim = similarities(q, bank, normalize_rows, exclude_self)
    assert k <= sim.shape[1] - bool(exclude_self)
    s, idx = torch.sort(-sim, dim=1, stable=True)
    return -s[:, :k], idx[:, :k]


def vote(sim, idx, bank_cls, num_classes, ks, T):
    """scores float64 [Nq, len(ks), C]: s_c = sum over ranks r < k with class c of exp(sim_r / T)"""
    cls = bank_cls.long()[idx]
    w = torch.exp(sim.double() / T)
    out = torch.zeros(sim.shape[0], len(ks), num_classes, dtype=torch.float64)
    for j, k in enumerate(ks):
        out[:, j].scatter_add_(1, cls[:, :k], w[:, :k])
    return out


def rank_of(scores, cls):
    """number of classes that beat class cls[i] in scores [N, C] under (larger score, then lower class); 0 = it is the prediction"""
    n, C = scores.shape
    mine = scores[torch.arange(n), cls.long()].unsqueeze(1)
    cols = torch.arange(C).expand(n, C)
    return ((scores > mine) | ((scores == mine) & (cols < cls.long().unsqueeze(1)))).sum(dim=1)


def predict(scores):
    """arg-max of scores [N, C], ties to the lowest class"""
    top = scores.max(dim=1, keepdim=True).values
    cols = torch.arange(scores.shape[1]).expand_as(scores)
    return torch.where(scores == top, cols, torch.full_like(cols, scores.shape[1])).min(dim=1).values


def hits(scores, truth):
    """(top-1 count, top-5 count) of scores [N, C] against class indices truth [N]; a truth outside 0 .. C-1 never hits"""
    ok = (truth >= 0) & (truth < scores.shape[1])
    r = rank_of(scores[ok], truth[ok])
    return int((r == 0).sum()), int((r < 5).sum())


def lattice(n, d, seed, duplicates=0):
    """fp32 [n, d] of integers in [-4, 4]: every dot product is exact in fp32 in any order.  The last ``duplicates`` rows repeat the first ones."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (n, d), generator=g).float()
    if duplicates:
        x[n - duplicates:] = x[:duplicates]
    return x
