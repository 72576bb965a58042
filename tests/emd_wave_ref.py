"""numpy restatement of the one-wave-per-pair auction (csrc/emd.hip, emd_wave_kernel; not a test itself): the same steps in the same order
with every operation rounded to float32, so that it returns what the kernel returns bit for bit.  Costs come from tests/emd_ref.py."""
import numpy as np

from tests import emd_ref as R

F = np.float32
INF = F(np.inf)
THETA = F(4.0)


def _next_up(p):
    """the float32 whose bit pattern is that of p plus one (the kernel's integer increment)"""
    return (np.array([p], dtype=np.float32).view(np.int32) + np.int32(1)).view(np.float32)[0]


def solve(x1, x2, eps_final, eps_rel=0.0, max_bids=100000):
    """one pair, x1 / x2 float32 [N, 3], 1 <= N <= 64 -> (assignment int32 [N], dist float32 [N], info int, eps_used float32)"""
    with np.errstate(all="ignore"):
        return _solve(np.asarray(x1, dtype=np.float32), np.asarray(x2, dtype=np.float32), F(eps_final), F(eps_rel), int(max_bids))


def _solve(x1, x2, eps_final, eps_rel, max_bids):
    n = x1.shape[0]
    assert 1 <= n <= 64 and x2.shape == x1.shape and max_bids >= 1
    d = R.sqdist(x1, x2)                                             # float32 [n, n], the kernel's rounding order
    finite = d[~np.isnan(d)]
    dmax = F(max(F(0.0), finite.max())) if finite.size else F(0.0)   # 1. fmaxf drops NaN
    eps_used = F(eps_rel * dmax)                                     # 2. one rounded product ...
    eps_used = eps_final if np.isnan(eps_used) else max(eps_final, eps_used)     # ... and fmaxf
    eps, first = eps_used, F(dmax * F(0.25))                         # 3. the ladder
    for _ in range(64):
        if not eps < first:
            break
        eps = F(eps * THETA)
    price = np.zeros(n, dtype=np.float32)
    owner = np.full(n, -1, dtype=np.int64)
    assign = np.full(n, -1, dtype=np.int64)
    bids, capped = 0, False
    while True:                                                      # 4. one phase: everything unassigned, prices kept
        owner[:] = -1
        assign[:] = -1
        while True:
            un = np.nonzero(assign < 0)[0]
            if un.size == 0:
                break
            if bids >= max_bids:                                     # 6. the cap, before every bid
                capped = True
                break
            bids += 1
            i = int(un[0])                                           # 5. the lowest unassigned bidder
            u = d[i] + price                                         # float32, one rounded sum per object
            m1 = F(np.fmin.reduce(u))
            eq = np.nonzero(u == m1)[0]
            jb = int(eq[0]) if eq.size else 0                        # 7. nothing compares equal: object 0
            rest = u.copy()
            rest[jb] = INF
            m2 = F(np.fmin.reduce(rest))                             # +inf when n == 1
            p = price[jb]
            bid = F(F(p + F(m2 - m1)) + eps) if m2 < INF else F(p + eps)
            if not bid > p:
                bid = _next_up(p)
            prev = owner[jb]
            price[jb] = bid
            owner[jb] = i
            assign[i] = jb
            if prev >= 0:
                assign[prev] = -1
        if capped or not eps > eps_used:
            break
        eps = max(F(eps / THETA), eps_used)
    if capped:                                                       # unassigned bidders take the free objects, both ascending
        free = [j for j in range(n) if owner[j] < 0]
        for i, j in zip([i for i in range(n) if assign[i] < 0], free):
            assign[i] = j
            owner[j] = i
    a = assign.astype(np.int32)
    return a, d[np.arange(n), a].astype(np.float32), (-bids if capped else bids), F(eps_used)


def solve_batch(x1, x2, eps_final, eps_rel=0.0, max_bids=100000):
    """[B, N, 3] each -> (assignment int32 [B, N], dist float32 [B, N], info int32 [B], eps_used float32 [B])"""
    out = [solve(a, b, eps_final, eps_rel, max_bids) for a, b in zip(x1, x2)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32),
            np.array([o[3] for o in out], dtype=np.float32))
