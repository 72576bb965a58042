"""``extensions.emd`` of the code bases ACT grew from (Point-BERT, PoinTr; models/dvae.py:302,701 keep the line
``# self.loss_func_emd = emd().cuda()``), backed by act_emd_{fwd,bwd}_f32 (csrc/emd.hip): the Earth Mover's Distance between two clouds of
the same size, i.e. the one-to-one matching a that minimises sum_i |xyz1[i] - xyz2[a(i)]|^2.

The historical module is an approximate auction with a fixed iteration count; it can leave points unassigned and differs from run to run.
This one runs the auction with eps-scaling to its end on the device, one workgroup per pair:

  * ``assignment`` is always a bijection, and all outputs are bit-identical run to run and independent of the batch a pair is solved in;
  * ``sum(dist) <= optimum + N * eps_final`` whenever ``info >= 0`` (exact arithmetic; in float32 every comparison of the auction carries
    at most 3 ulp of the largest cost + price on top of ``eps_final``);
  * ``info`` (int32 [B], ``last_info`` on the modules, never read on the host here) holds the rounds used, negated when ``max_rounds`` was
    hit; then the bidders still unassigned got the objects still free in ascending order and the bound does not hold.

``DEFAULT_EPS`` = 1e-5.  Clouds here are normalised to the unit sphere (datasets' ``pc_norm``): squared distances are at most 4 and the
prices of the auction stay below 16, where a float32 ulp is at most 9.5e-7, so 1e-5 is ten times the rounding of a comparison and the bound
above holds with room.  The slack per point, 1e-5 in squared distance, is a tenth or less of the squared matching distance of a Stage-I
reconstruction (CDL1 x1000 of 10 .. 30, i.e. distances of 0.01 .. 0.03, squares of 1e-4 .. 1e-3).  A smaller value buys accuracy with rounds
(each factor of 4 is one more phase); below about 1e-6 the float32 rounding of the prices dominates and nothing is gained.
For inputs on another scale pass ``eps`` of about 2.5e-6 times the largest squared distance.

``DEFAULT_MAX_ROUNDS`` = 1,000,000 rounds over all phases.  Unit-sphere clouds need about 1,500 rounds at N = 256, 6,000 at 1,024 and 24,000 at
2,048; the cap is there so that no input can keep a kernel running, not to be met.

``solver="wave"`` (act_emd_wave_fwd_f32) is the solver for MANY SMALL pairs, the regime of a Stage-I loss over ``B*G`` group patches of
``group_size`` points: N <= ``wave_max_points()`` = 64, one wavefront per pair, the auction in registers with one bid at a time (Gauss-Seidel,
lowest unassigned bidder first).  For it ``max_rounds`` caps the BIDS, ``info`` counts bids, and the final eps is
``eps_used = max(eps, eps_rel * largest squared distance of the pair)``: group patches live on scales from 0.05 to 1 and no absolute eps fits
them all; ``eps_rel = 2**-18`` is the 2.5e-6 of the paragraph above.  ``sum(dist) <= optimum + N * eps_used`` whenever ``info >= 0``.
The default solver is ``"workgroup"`` for every N: nothing changes for a caller that does not ask for ``"wave"``."""
import torch

from ... import _C

DEFAULT_EPS = 1e-5
DEFAULT_MAX_ROUNDS = 1000000


def max_points():
    """the largest N a pair may have (everything the solve touches lives in the LDS of one compute unit)"""
    return int(_C.lib.act_emd_max_points())


def wave_max_points():
    """the largest N a pair may have with ``solver="wave"`` (one object per lane of a wavefront)"""
    return int(_C.lib.act_emd_wave_max_points())


SOLVERS = ("workgroup", "wave")


def _check_solver(solver, eps_rel):
    if solver not in SOLVERS:
        raise ValueError(f"emd: solver = {solver!r} (supported: {', '.join(map(repr, SOLVERS))})")
    eps_rel = float(eps_rel)
    if not (0.0 <= eps_rel < float("inf")):
        raise ValueError(f"emd: eps_rel = {eps_rel!r} must be finite and not negative")
    if solver == "workgroup" and eps_rel != 0.0:
        raise ValueError('emd: eps_rel is an argument of solver="wave"; the workgroup solver takes an absolute eps only')
    return eps_rel


def _check(xyz1, xyz2):
    for t in (xyz1, xyz2):
        if not torch.is_tensor(t) or t.dim() != 3 or t.shape[-1] != 3:
            raise RuntimeError("emd: expected float32 CUDA tensors of shape [B, N, 3]")
    if xyz1.shape[0] != xyz2.shape[0]:
        raise RuntimeError("emd: batch sizes differ")
    _check_counts(xyz1.shape[1], xyz2.shape[1])
    for t in (xyz1, xyz2):
        if not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError("emd: expected float32 CUDA tensors of shape [B, N, 3] (the kernels run on the GPU only)")


def _check_counts(n1, n2):
    if n1 != n2:
        raise ValueError(f"emd: xyz1 has {n1} points and xyz2 has {n2}; the matching is one-to-one, so the clouds must have the same size")
    if n1 < 1 or n1 > max_points():
        raise ValueError(f"emd: {n1} points per cloud (supported: 1 .. {max_points()})")


class emd_cuda:          # namespace standing in for the compiled ``emd_cuda`` module
    @staticmethod
    def forward(xyz1, xyz2, eps=DEFAULT_EPS, max_rounds=DEFAULT_MAX_ROUNDS, want_evals=False, solver="workgroup", eps_rel=0.0, want_eps=False):
        """-> [dist f32 [B,N], assignment int32 [B,N], info int32 [B]] (+ evals int64 [B], the bids made, with ``want_evals``; + eps_used
        f32 [B] with ``want_eps``).  ``solver="wave"``: N <= ``wave_max_points()``, ``max_rounds`` caps the bids and ``info`` counts them (so
        ``want_evals`` is refused), ``eps_used = max(eps, eps_rel * largest squared distance)`` per pair.  With the workgroup solver
        ``eps_used`` is ``eps``."""
        _check(xyz1, xyz2)
        eps, max_rounds = float(eps), int(max_rounds)
        if not (0.0 < eps < float("inf")) or max_rounds < 1:
            raise ValueError(f"emd: eps = {eps!r} must be positive and finite, max_rounds = {max_rounds!r} at least 1")
        eps_rel = _check_solver(solver, eps_rel)
        xyz1 = xyz1.contiguous(); xyz2 = xyz2.contiguous()
        B, N, _ = xyz1.shape
        dev = xyz1.device
        if solver == "wave":
            if N > wave_max_points():
                raise ValueError(f'emd: solver="wave" takes at most {wave_max_points()} points per cloud, got {N}')
            if want_evals:
                raise ValueError('emd: solver="wave" makes one bid at a time, so info already is the number of bids; want_evals has nothing to add')
        dist = torch.empty(B, N, dtype=torch.float32, device=dev)
        assignment = torch.empty(B, N, dtype=torch.int32, device=dev)
        info = torch.empty(B, dtype=torch.int32, device=dev)
        if solver == "wave":
            eps_used = torch.empty(B, dtype=torch.float32, device=dev) if want_eps else None
            _C.check(_C.lib.act_emd_wave_fwd_f32(_C.ptr(xyz1), _C.ptr(xyz2), B, N, eps, eps_rel, max_rounds, _C.ptr(dist), _C.ptr(assignment),
                                                 _C.ptr(info), _C.ptr(eps_used), _C.stream()), "act_emd_wave_fwd_f32")
            return [dist, assignment, info] + ([eps_used] if want_eps else [])
        evals = torch.empty(B, dtype=torch.int64, device=dev) if want_evals else None
        _C.check(_C.lib.act_emd_fwd_ex_f32(_C.ptr(xyz1), _C.ptr(xyz2), B, N, eps, max_rounds, _C.ptr(dist), _C.ptr(assignment), _C.ptr(info),
                                           _C.ptr(evals), _C.stream()), "act_emd_fwd_ex_f32")
        return [dist, assignment, info] + ([evals] if want_evals else []) + \
            ([torch.full((B,), eps, dtype=torch.float32, device=dev)] if want_eps else [])

    @staticmethod
    def backward(xyz1, xyz2, assignment, grad_dist):
        """-> [gx1, gx2]: gx1[i] = (2 * (xyz1[i] - xyz2[a(i)])) * grad_dist[i], gx2[a(i)] = -gx1[i]"""
        _check(xyz1, xyz2)
        xyz1 = xyz1.contiguous(); xyz2 = xyz2.contiguous()
        B, N, _ = xyz1.shape
        if assignment.dtype != torch.int32 or tuple(assignment.shape) != (B, N) or tuple(grad_dist.shape) != (B, N) \
                or grad_dist.dtype != torch.float32:
            raise RuntimeError("emd: assignment must be int32 [B, N] and grad_dist float32 [B, N]")
        assignment = assignment.contiguous(); g = grad_dist.contiguous()
        gx1 = torch.empty_like(xyz1); gx2 = torch.empty_like(xyz2)
        _C.check(_C.lib.act_emd_bwd_f32(_C.ptr(xyz1), _C.ptr(xyz2), _C.ptr(assignment), _C.ptr(g), B, N, _C.ptr(gx1), _C.ptr(gx2),
                                        _C.stream()), "act_emd_bwd_f32")
        return [gx1, gx2]


class EMDFunction(torch.autograd.Function):
    """(xyz1, xyz2, eps, max_rounds[, info_out, solver, eps_rel]) -> (dist, assignment); ``assignment`` is not differentiable.  The matching is piecewise constant in the
    inputs, so the gradient is that of sum_i g[i] |xyz1[i] - xyz2[a(i)]|^2 with a held fixed.  ``info_out``: a list that receives the solve's
    ``info`` tensor (the modules keep it as ``last_info``)."""
    @staticmethod
    def forward(ctx, xyz1, xyz2, eps=DEFAULT_EPS, max_rounds=DEFAULT_MAX_ROUNDS, info_out=None, solver="workgroup", eps_rel=0.0):
        dist, assignment, info = emd_cuda.forward(xyz1, xyz2, eps, max_rounds, solver=solver, eps_rel=eps_rel)
        if info_out is not None:
            info_out.append(info)
        ctx.save_for_backward(xyz1, xyz2, assignment)
        ctx.mark_non_differentiable(assignment)
        return dist, assignment

    @staticmethod
    def backward(ctx, grad_dist, _grad_assignment):
        xyz1, xyz2, assignment = ctx.saved_tensors
        gx1, gx2 = emd_cuda.backward(xyz1, xyz2, assignment, grad_dist)
        return gx1, gx2, None, None, None, None, None


class emdModule(torch.nn.Module):
    """``emdModule(eps=..., max_rounds=...)``; ``forward(xyz1, xyz2)`` -> (dist [B,N], assignment int32 [B,N]).  The historical call shape
    ``forward(xyz1, xyz2, eps, iters)`` is accepted: ``eps`` is ``eps_final`` and ``iters`` is ``max_rounds`` (not a number of rounds that
    will be run: the solve ends when it is done).  ``last_info``: the ``info`` tensor of the last call (on the device), None before it.
    ``solver="wave"`` with ``eps_rel``: the one-wave-per-pair solver for N <= 64 (module docstring); ``max_rounds`` then caps the bids."""
    def __init__(self, eps=None, max_rounds=None, solver="workgroup", eps_rel=0.0):
        super().__init__()
        self.eps_rel = _check_solver(solver, eps_rel)
        self.solver = solver
        self.eps = DEFAULT_EPS if eps is None else float(eps)
        self.max_rounds = DEFAULT_MAX_ROUNDS if max_rounds is None else int(max_rounds)
        self.last_info = None

    def forward(self, xyz1, xyz2, eps=None, iters=None):
        info = []
        dist, assignment = EMDFunction.apply(xyz1, xyz2, self.eps if eps is None else float(eps),
                                             self.max_rounds if iters is None else int(iters), info, self.solver, self.eps_rel)
        self.last_info = info[0]
        return dist, assignment


emd = emdModule


class EarthMoverDistance(emdModule):
    """mean over all points of the batch of sqrt(dist), the distance (not its square) to the matched point: a differentiable scalar on the
    scale of ChamferDistanceL1.  (The square root has no finite slope at 0: a point that coincides with its match gives a NaN gradient,
    as in ChamferDistanceL1.)"""
    def forward(self, xyz1, xyz2):
        dist, _ = super().forward(xyz1, xyz2)
        return torch.mean(torch.sqrt(dist))
