"""numpy restatement for the Earth Mover's Distance tests (not a test itself): the cost matrix in the kernel's rounding order and the exact
assignment optimum over it."""
import numpy as np


def sqdist(x1, x2):
    """float32 [N, N]: d[i, j] = (dx*dx + dy*dy) + dz*dz of x1[i] - x2[j], every product and sum rounded to float32 (csrc/emd.hip, sqdist3)"""
    x1 = np.asarray(x1, dtype=np.float32)
    x2 = np.asarray(x2, dtype=np.float32)
    dx = x1[:, None, 0] - x2[None, :, 0]
    dy = x1[:, None, 1] - x2[None, :, 1]
    dz = x1[:, None, 2] - x2[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def emd_assignment(x1, x2):
    """(optimum, assignment): the minimum over bijections a of sum_i d[i, a(i)], in float64 over the float32-rounded costs of ``sqdist``, by the
    O(N^3) Hungarian method with potentials (shortest augmenting paths, one row at a time; the column scan is vectorised)"""
    c = sqdist(x1, x2).astype(np.float64)
    n = c.shape[0]
    u = np.zeros(n + 1)
    v = np.zeros(n + 1)
    p = np.zeros(n + 1, dtype=np.int64)                   # p[j]: the row matched to column j (1-based, 0 = none)
    way = np.zeros(n + 1, dtype=np.int64)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(n + 1, np.inf)
        used = np.zeros(n + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = c[i0 - 1] - u[i0] - v[1:]
            free = ~used[1:]
            upd = free & (cur < minv[1:])
            minv[1:][upd] = cur[upd]
            way[1:][upd] = j0
            masked = np.where(free, minv[1:], np.inf)
            j1 = int(np.argmin(masked)) + 1
            delta = masked[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[1:][free] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while True:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
            if j0 == 0:
                break
    assignment = np.empty(n, dtype=np.int64)
    assignment[p[1:] - 1] = np.arange(n)
    return float(c[np.arange(n), assignment].sum()), assignment


def emd_optimum(x1, x2):
    return emd_assignment(x1, x2)[0]
