"""Host: the numpy restatement of the set-abstraction kernels (tests/sa_ref.py) against the reference's recorded outputs
(tests/golden/g25_sa.npz), the C ABI of csrc/sa.hip, and the state-dict layout of models/pointnet2.py.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import sa_ref as R
from tests.conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("act_ball_query_f32", "act_group_rows_fwd_f32", "act_group_rows_bwd_workspace", "act_group_rows_bwd_f32", "act_group_gather_f32",
           "act_group_gather_bwd_f32")


@pytest.fixture(scope="module")
def g():
    return golden("g25_sa")


@pytest.mark.parametrize("tag", ["wide", "dense"])
def test_ball_query_ref_equals_the_reference_on_lattice_clouds(g, tag):
    """on the 1/8 lattice the expanded and the difference form give the same float32 distances, so the reference's query_ball_point is an
    exact oracle (its rule is the inclusive one); the exclusive rule must differ somewhere, i.e. points lie exactly on a sphere"""
    xyz, new_xyz = g[f"{tag}_xyz"], g[f"{tag}_new_xyz"]
    differs = 0
    for qi, (r, ns) in enumerate(zip(g["query_radius"], g["query_nsample"])):
        idx, cnt = R.ball_query(xyz, new_xyz, float(r), int(ns), inclusive=True)
        assert idx.dtype == np.int32 and np.array_equal(idx, g[f"{tag}_idx{qi}"])
        assert cnt.min() >= 1                                           # the centres are cloud points
        idx_x, cnt_x = R.ball_query(xyz, new_xyz, float(r), int(ns), inclusive=False)
        assert np.all(cnt_x <= cnt)
        differs += int((idx_x != idx).any())
    assert differs


@pytest.mark.parametrize("tag", ["wide", "dense"])
def test_group_rows_ref_equals_sample_and_group(g, tag):
    xyz, feat = g[f"{tag}_xyz"], g[f"{tag}_feat"]
    assert np.array_equal(g[f"{tag}_sg_new_xyz"], g[f"{tag}_new_xyz"])
    idx, _ = R.ball_query(xyz, g[f"{tag}_new_xyz"], 0.5, 8, inclusive=True)
    rows = R.group_rows(xyz, g[f"{tag}_new_xyz"], feat, idx)
    want = g[f"{tag}_sg_new_points"]
    assert rows.dtype == np.float32 and np.array_equal(rows, want.reshape(-1, want.shape[-1]))


def test_ball_query_ref_edges():
    xyz = np.zeros((1, 5, 3), np.float32)
    xyz[0, :, 0] = [0, 1, 2, 3, 4]
    q = np.array([[[2, 0, 0], [10, 0, 0]]], np.float32)
    idx, cnt = R.ball_query(xyz, q, 1.0, 4, inclusive=True)
    assert idx[0, 0].tolist() == [1, 2, 3, 1] and cnt[0].tolist() == [3, 0] and idx[0, 1].tolist() == [0, 0, 0, 0]
    idx, cnt = R.ball_query(xyz, q, 1.0, 4, inclusive=False)
    assert idx[0, 0].tolist() == [2, 2, 2, 2] and cnt[0].tolist() == [1, 0]
    idx, cnt = R.ball_query(xyz, q, 1.0, 2, inclusive=True)
    assert idx[0, 0].tolist() == [1, 2] and cnt[0, 0] == 2


def test_group_rows_bwd_ref_is_the_adjoint():
    rs = np.random.RandomState(3)
    B, N, S, ns, D = 2, 11, 4, 3, 5
    idx = rs.randint(0, N - 2, size=(B, S, ns)).astype(np.int32)        # the last two points are never gathered
    xyz, q = rs.randn(B, N, 3).astype(np.float32), rs.randn(B, S, 3).astype(np.float32)
    feat, gr = rs.randn(B, N, D), rs.randn(B * S * ns, 3 + D)
    rows = R.group_rows(xyz, q, feat.astype(np.float32), idx).astype(np.float64)
    d = R.group_rows_bwd(gr, idx, N, D, dtype=np.float64)
    assert np.all(d[:, N - 2:] == 0)
    lhs = (rows[:, 3:] * gr[:, 3:]).sum()
    rhs = (feat.astype(np.float32).astype(np.float64) * d).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    feats_cf = np.ascontiguousarray(feat.transpose(0, 2, 1))
    assert np.array_equal(R.grouping_operation(feats_cf, idx)[1, 2], feat[1][idx[1], 2])


def test_library_exports_and_binding_declares_the_new_symbols():
    import __graft_entry__ as ge
    ge.build()
    from act_amd import _abi
    lib = ctypes.CDLL(os.path.join(ROOT, "act_amd", "lib", "libact_hip.so"))
    header = open(os.path.join(ROOT, "include", "act_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES, name
        assert name + "(" in header, name
    assert _abi.SIGNATURES["act_group_rows_bwd_workspace"][0] is ctypes.c_size_t
    lib.act_group_rows_bwd_workspace.restype = ctypes.c_size_t
    lib.act_group_rows_bwd_workspace.argtypes = [ctypes.c_int] * 4
    assert lib.act_group_rows_bwd_workspace(2, 10, 3, 4) == 4 * (2 * 11 + 2 * 12)
    assert "sa.hip" in os.listdir(os.path.join(ROOT, "act_amd", "csrc"))
    from act_amd import build as B
    assert "-ffp-contract=off" in B.PER_FILE["sa.hip"]


def test_state_dict_layout_is_the_reference(g):
    from tests.golden.make_golden_sa import SA, MSG, SA_ALL, SA_XYZ
    from act_amd.models import pointnet2 as P
    from act_amd.models import semseg
    assert P.PointNetFeaturePropagation is semseg.PointNetFeaturePropagation
    for tag, cls, kw in (("sa", P.PointNetSetAbstraction, SA), ("msg", P.PointNetSetAbstractionMsg, MSG), ("all", P.PointNetSetAbstraction, SA_ALL),
                         ("xyzonly", P.PointNetSetAbstraction, SA_XYZ)):
        sd = cls(**kw).state_dict()
        assert list(sd.keys()) == g[f"{tag}_sd_keys"].tolist(), tag
        assert [",".join(map(str, v.shape)) for v in sd.values()] == g[f"{tag}_sd_shapes"].tolist(), tag
    assert "mlp_convs.0.weight" in g["sa_sd_keys"].tolist() and "conv_blocks.1.0.weight" in g["msg_sd_keys"].tolist()


def test_the_new_surface_refuses_cpu_tensors_and_bad_arguments():
    from act_amd import kernels as K
    from act_amd.pointnet2_ops import pointnet2_utils as pu
    from act_amd.models import pointnet2 as P
    xyz, q = torch.zeros(1, 8, 3), torch.zeros(1, 2, 3)
    with pytest.raises(RuntimeError, match="xyz"):
        pu.ball_query(0.5, 4, xyz, q)
    with pytest.raises(RuntimeError, match="xyz"):
        K.ball_query(xyz, q, 0.5, 4)
    with pytest.raises(RuntimeError, match="features"):
        pu.grouping_operation(torch.zeros(1, 4, 8), torch.zeros(1, 2, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="xyz"):
        P.PointNetSetAbstraction(2, 0.5, 4, 3, [8], False)(xyz.transpose(1, 2), None)
    with pytest.raises(ValueError, match="mlp"):
        P.PointNetSetAbstraction(2, 0.5, 4, 3, [6], False)
