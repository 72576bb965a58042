"""The four gradient identities of the composed mini-PointNet backward (csrc/composite.hip, act_pointnet_bwd_f32) in float64 against autograd of the
sequential form.  Host only: no GPU, no library.

Sequential:  h2 = a1 W2^T + b2;  fg = max over the points of a group of h2;  h3 = h2 W3b^T + gw[group],  gw = fg W3a^T + b3.
With dh3 given, G = dh3^T a1, s3 = colsum(dh3), dfg = group_sum(dh3) W3a and S = dfg scattered to the arg-max rows:
  dW3b = G W2^T + s3 (x) b2     dW2 = W3b^T G + S^T a1     db2 = W3b^T s3 + sum_g dfg[g]     da1 = dh3 W32 + S W2,   W32 = W3b W2."""
import torch


def test_composed_backward_formulas_match_autograd():
    g = torch.Generator().manual_seed(0)
    BG, n = 6, 32
    R = BG * n
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    a1 = torch.relu(rnd(R, 128)).requires_grad_(True)
    W2 = (rnd(256, 128) / 128 ** 0.5).requires_grad_(True)
    b2 = (0.1 * rnd(256)).requires_grad_(True)
    W3 = (rnd(512, 512) / 512 ** 0.5).requires_grad_(True)
    b3 = 0.1 * rnd(512)
    dh3 = rnd(R, 512)

    h2 = a1 @ W2.T + b2
    fg, arg1 = h2.reshape(BG, n, 256).max(1)
    gw = fg @ W3[:, :256].T + b3
    h3 = h2 @ W3[:, 256:].T + gw.repeat_interleave(n, 0)
    h3.backward(dh3)

    with torch.no_grad():
        W3a, W3b = W3[:, :256], W3[:, 256:]
        W32 = W3b @ W2
        # the composed forward is the sequential one
        h3c = a1 @ W32.T + (fg @ W3a.T + (b3 + W3b @ b2)).repeat_interleave(n, 0)
        assert (h3c - h3).abs().max() <= 1e-9
        G = dh3.T @ a1
        s3 = dh3.sum(0)
        dfg = dh3.reshape(BG, n, 512).sum(1) @ W3a
        S = torch.zeros(BG, n, 256, dtype=torch.float64).scatter_(1, arg1.unsqueeze(1), dfg.unsqueeze(1)).reshape(R, 256)
        got = {"dW3b": G @ W2.T + torch.outer(s3, b2), "dW2": W3b.T @ G + S.T @ a1, "db2": W3b.T @ s3 + dfg.sum(0), "da1": dh3 @ W32 + S @ W2}
        want = {"dW3b": W3.grad[:, 256:], "dW2": W2.grad, "db2": b2.grad, "da1": a1.grad}
        for k in got:
            assert (got[k] - want[k]).abs().max() <= 1e-9, (k, (got[k] - want[k]).abs().max().item())
