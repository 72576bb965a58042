"""CPU: the host side of the K-tile-major planes (notebook/x3_ktile.md) -- the index formula against a numpy restatement of the layout, the layout field of
the three plane structs (zero = row-major, so a zero-initialised struct behaves as before), and the plane caches of act_amd.composite: built once, rebuilt when a
weight is written in place or the switch is turned, repacked exactly when the switch is on.  No kernel runs: the device passes are replaced by counters."""
import numpy as np
import pytest
import torch


@pytest.mark.parametrize("rows,cols", [(1, 32), (5, 64), (128, 96), (384, 128)])
def test_index_formula_is_the_layout(rows, cols):
    import act_amd.kernels as K
    src = np.arange(rows * cols).reshape(rows, cols)
    kt = src.reshape(rows, cols // 32, 32).transpose(1, 0, 2).ravel()             # K tile by K tile, the 32-element pieces of all rows side by side
    r, k = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    idx = K.ktile_index(r, k, rows)
    assert np.array_equal(kt[idx], src) and np.array_equal(np.sort(idx.ravel()), np.arange(rows * cols))
    assert np.array_equal(K.ktile_rows(torch.from_numpy(kt), rows, cols).numpy(), src)
    # a thread's 16 bytes: row tid / 4, chunk tid % 4 of one K tile's block of a row tile -> byte 16 tid of that block (the whole-line staging load)
    t, row0, tid = cols // 32 - 1, 0, np.arange(4 * rows)
    assert np.array_equal(K.ktile_index(row0 + tid // 4, t * 32 + (tid % 4) * 8, rows) - K.ktile_index(row0, t * 32, rows), 8 * tid)
    # rows r0 .. of a taller matrix / a column slice at c0: a pointer offset and the K-tile stride of the whole matrix
    total, r0 = rows + 7, 3
    assert np.array_equal(K.ktile_index(r + r0, k, total), K.ktile_index(r0, 0, total) + (k // 32) * total * 32 + r * 32 + k % 32)


def test_layout_field_is_last_and_defaults_to_row_major():
    from act_amd._abi import DgcnnF16x3, PointnetF16x3, VitF16x3
    import act_amd.kernels as K
    assert (K.X3_ROWMAJOR, K.X3_KTILE) == (0, 1)
    for S in (VitF16x3, PointnetF16x3, DgcnnF16x3):
        assert S._fields_[-1][0] == "w_layout" and S().w_layout == K.X3_ROWMAJOR


class _Passes:
    """stand-ins for the device passes the plane builders call, counted"""
    def __init__(self, monkeypatch, kt):
        import act_amd.kernels as K
        self.kt, self.splits, self.repacks = kt, 0, 0
        monkeypatch.setattr(K, "x3_kt", lambda on=None: self.kt)
        monkeypatch.setattr(K, "split_f16x2", self._split)
        monkeypatch.setattr(K, "repack_ktile", self._repack)

    def _split(self, x, scale=1.0, row_scale=None, out=None):
        self.splits += 1
        return torch.stack([x.detach().half(), torch.zeros_like(x, dtype=torch.float16)])

    def _repack(self, planes):
        self.repacks += 1
        return planes.clone()


def _encoder():
    enc = torch.nn.Module()
    enc.second_conv = torch.nn.Sequential(torch.nn.Conv1d(512, 512, 1), torch.nn.BatchNorm1d(512), torch.nn.ReLU(), torch.nn.Conv1d(512, 128, 1))
    return enc


def test_pointnet_plane_cache_rebuilds_on_a_weight_change_and_on_the_switch(monkeypatch):
    import act_amd.composite as CP
    p = _Passes(monkeypatch, kt=True)
    enc = _encoder()
    assert CP._pointnet_f16_planes(enc, 256)[0].w_layout == int(CP.X3_KT_PN) and p.repacks == int(CP.X3_KT_PN)      # as shipped
    monkeypatch.setattr(CP, "X3_KT_PN", True)                                      # the mechanism, whichever way the per-launch figures decided
    p.splits = p.repacks = 0
    s, _ = CP._pointnet_f16_planes(enc, 256)
    assert (p.splits, p.repacks, s.w_layout) == (1, 1, 1)
    s, _ = CP._pointnet_f16_planes(enc, 256)
    assert (p.splits, p.repacks, s.w_layout) == (1, 1, 1)                          # cached
    with torch.no_grad():
        enc.second_conv[3].weight.mul_(1.5)
    s, _ = CP._pointnet_f16_planes(enc, 256)
    assert (p.splits, p.repacks, s.w_layout) == (2, 2, 1)                          # a weight written in place
    p.kt = False
    s, _ = CP._pointnet_f16_planes(enc, 256)
    assert (p.splits, p.repacks, s.w_layout) == (3, 2, 0)                          # the switch turned: row-major planes, the only copy
    p.kt = True
    s, _ = CP._pointnet_f16_planes(enc, 256)
    assert (p.splits, p.repacks, s.w_layout) == (4, 3, 1)


def test_dgcnn_plane_cache_rebuilds_on_a_weight_change_and_on_the_switch(monkeypatch):
    import act_amd.composite as CP
    from act_amd.models.dvae import DGCNN
    p = _Passes(monkeypatch, kt=True)
    torch.manual_seed(0)
    dg = DGCNN(encoder_channel=128, output_channel=1024)
    build = lambda: CP._dgcnn_f16_planes(dg, 128, 64, 4, torch.device("cpu"), head=True, layers=True)[0]
    s = build()
    assert (p.splits, p.repacks, s.w_layout, s.layers) == (4, 4, 1, 1)             # the head and three stacked matrices
    s = build()
    assert (p.splits, p.repacks) == (4, 4)
    with torch.no_grad():
        dg.layer3[0].weight.mul_(1.5)
    s = build()
    assert (p.splits, p.repacks, s.w_layout) == (8, 8, 1)
    p.kt = False
    s = build()
    assert (p.splits, p.repacks, s.w_layout) == (12, 8, 0)
