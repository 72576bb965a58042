"""FPS and kNN-group (act_amd/csrc/point_ops.hip) on inputs that TIE, at the ragged tail of every dispatch row, bit for bit against the numpy oracle.
The inputs and their case tables live in tests/point_ops_cases.py; tests/test_point_ops_cases_host.py proves that they tie across lanes / waves, with
the lower index in the higher lane, and across the K-th neighbour.  No tolerance anywhere: indices, distances, neighbourhoods and centres are equal
or the test fails.

Kernel instantiation -> the case that reaches it
  knn_group_kernel<1|2|4>          (63,63) (1,1) (2,2) | (127,16) | (130,64) (254,32)
  knn_tree_kernel<8|16|32|64|128>  (257,9) (390,32) (511,32) | (1022,32) | (2047,32) | (2049,64) (4095,64) | (4097,64) (8190,64)
  knn_group_big_kernel             (8193,8) by N, (130,65) by K
  knn_group2_kernel<8..32, 4>, <64|128, 8>      the same N >= 257 cases in a child process with ACT_KNN_TREE=0
  knn_group_kernel<8..128>                      ... with ACT_KNN_TWO_LEVEL=0 ACT_KNN_TWO_LEVEL_SMALL=0 on top
  fps_kernel<1,4> (200,24) (70,80)  <4,4> (1000,24)  <4,8> (2047,24)  <8,8> (4001,40)  <16,8> (8190,40)
  fps_kernel<16,16> cloud in LDS (10922,40), from global memory (10923,40) (16383,40) (10922,8131) (10500,10500); fps_big_kernel (16390,24)
  fps_kernel<1,16> <2,8> <8,2> <16,1>           ACT_FPS_CFG = 1..4 at N = 300 and 1000"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import point_ops_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 120                     # seconds for one child: interpreter start, 26 launches, 26 numpy references


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    import act_amd._C as C          # fails loudly if libact_hip.so is missing
    assert C.lib.act_arch() == b"gfx950"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ kNN-group
@pytest.mark.parametrize("kind", PC.KNN_KINDS)
@pytest.mark.parametrize("N,K", PC.KNN_CASES)
def test_knn_on_ties(dev, N, K, kind):
    PC.check_knn_case(dev, N, K, kind)


@pytest.mark.parametrize("kind", PC.KNN_KINDS)
@pytest.mark.parametrize("N,K", [(1022, 32), (8190, 64)])
def test_knn_idx_kq_is_the_transpose(dev, N, K, kind):
    from act_amd.knn_cuda import KNN, knn_group
    pts, q, d_ref, i_ref = PC.knn_case(N, K, kind)
    x, y = PC.to_device(pts, dev), PC.to_device(q, dev)
    idx, _, dist = knn_group(x, y, K, want_dist=True, idx_kq=True)
    assert tuple(idx.shape) == (PC.KNN_B, K, PC.KNN_Q) and idx.is_contiguous() and dist.is_contiguous()
    assert np.array_equal(idx.cpu().numpy(), i_ref.transpose(0, 2, 1)) and np.array_equal(dist.cpu().numpy(), d_ref.transpose(0, 2, 1))
    # the module in both layouts (transpose_mode=False takes [B,3,N] and answers [B,k,Q])
    d1, i1 = KNN(k=K, transpose_mode=True)(x, y)
    d2, i2 = KNN(k=K, transpose_mode=False)(x.transpose(1, 2).contiguous(), y.transpose(1, 2).contiguous())
    assert np.array_equal(i1.cpu().numpy(), i_ref) and np.array_equal(d1.cpu().numpy(), d_ref)
    assert torch.equal(i2, i1.transpose(1, 2)) and torch.equal(d2, d1.transpose(1, 2))


@pytest.mark.parametrize("kind", PC.KNN_KINDS)
def test_knn_register_kernel_gives_the_first_64_of_the_rescan_kernel(dev, kind):
    from act_amd.knn_cuda import knn_group
    pts, q, _, _ = PC.knn_case(130, 65, kind)
    assert np.array_equal(PC.knn_case(130, 64, kind)[0], pts)                              # one cloud, two kernels
    x, y = PC.to_device(pts, dev), PC.to_device(q, dev)
    i64, n64, d64 = knn_group(x, y, 64, want_nbr=True, want_dist=True)
    i65, n65, d65 = knn_group(x, y, 65, want_nbr=True, want_dist=True)
    assert torch.equal(i64, i65[..., :64]) and torch.equal(d64, d65[..., :64]) and torch.equal(n64, n65[..., :64, :])


# ------------------------------------------------------------------------------------------------ FPS
def _fps_both(dev, pts, G, skip):
    from act_amd.pointnet2_ops import pointnet2_utils as pu
    x = PC.to_device(pts, dev)
    plain = pu.furthest_point_sample(x, G, skip_near_origin=skip)
    fused, centres = pu.furthest_point_sample_with_centers(x, G, skip_near_origin=skip)
    torch.cuda.synchronize()
    assert plain.dtype == torch.int32 and fused.dtype == torch.int32
    return plain.cpu().numpy(), fused.cpu().numpy(), centres.cpu().numpy()


def _check_fps(dev, pts, ref, G, skip):
    plain, fused, centres = _fps_both(dev, pts, G, skip)
    tag = f"FPS N={pts.shape[1]} G={G} skip={skip}"
    first = lambda got: np.argwhere(got != ref)[:1].tolist()
    assert np.array_equal(plain, ref), f"{tag}: first difference at [cloud, step] {first(plain)}"
    assert np.array_equal(fused, ref), f"{tag} with centres: first difference at [cloud, step] {first(fused)}"
    assert np.array_equal(centres, pts[np.arange(pts.shape[0])[:, None], ref]), f"{tag}: centres are not pts[idx]"


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("N,G", PC.FPS_CASES)
def test_fps_on_ties(dev, N, G, skip):
    pts, ref = PC.fps_case(N, G, skip)
    _check_fps(dev, pts, ref, G, skip)


def test_fps_oversampled_with_dead_points(dev):
    N, G = PC.FPS_OVERSAMPLE
    pts, ref = PC.fps_case(N, G, True)
    _check_fps(dev, pts, ref, G, True)


@pytest.mark.parametrize("N", PC.FPS_CFG_N)
def test_fps_cfg_instantiations_agree_with_the_default(dev, monkeypatch, N):
    """ACT_FPS_CFG (read by the library on every call) = 1..4: <1,16> <2,8> <8,2> <16,1> instead of <4,4>"""
    G = 24
    monkeypatch.delenv("ACT_FPS_CFG", raising=False)
    for skip in (False, True):
        pts, ref = PC.fps_case(N, G, skip)
        default = _fps_both(dev, pts, G, skip)
        assert np.array_equal(default[0], ref)
        for cfg in ("1", "2", "3", "4"):
            monkeypatch.setenv("ACT_FPS_CFG", cfg)
            got = _fps_both(dev, pts, G, skip)
            monkeypatch.delenv("ACT_FPS_CFG")
            for a, b in zip(got, default):
                assert np.array_equal(a, b), f"ACT_FPS_CFG={cfg} N={N} skip={skip}"


@pytest.mark.parametrize("N,G", PC.FPS_CROWDED)
def test_fps_is_not_refused_when_the_indices_crowd_the_cloud_out_of_the_lds(dev, N, G):
    """12 * N bytes fit the 128 KB the cloud may take, cloud + 4 * G + header do not fit the 160 KB of a workgroup: the cloud stays in global memory"""
    pts, ref = PC.fps_crowded_case(N, G)
    _check_fps(dev, pts, ref, G, False)


# ------------------------------------------------------------------------------------------------ the A/B kNN kernels
CHILD_CASES = [c for c in PC.KNN_CASES if c[0] >= 257]
CHILD_ENVS = [{"ACT_KNN_TREE": "0"},                                                        # knn_group2_kernel<P, 4> (P <= 32), <P, 8> (P >= 64)
              {"ACT_KNN_TREE": "0", "ACT_KNN_TWO_LEVEL": "0", "ACT_KNN_TWO_LEVEL_SMALL": "0"}]   # flat knn_group_kernel<P >= 8>


def _child():
    """run by test_ab_knn_kernels_on_ties in a fresh interpreter (the selectors are read once per process)"""
    dev = torch.device("cuda:0")
    for N, K in CHILD_CASES:
        for kind in PC.KNN_KINDS:
            PC.check_knn_case(dev, N, K, kind)
        print(f"case N={N} K={K} ok", flush=True)
    print("child-ok")


def test_ab_knn_kernels_on_ties(dev):
    """one child after the other, each under its own time limit; the first that fails ends the test and nothing more is started on the device"""
    for extra in CHILD_ENVS:
        env = {k: v for k, v in os.environ.items() if not k.startswith("ACT_KNN_")}
        env.update(extra)
        r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_point_ops_edges as T; T._child()"], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        assert r.returncode == 0 and "child-ok" in r.stdout, f"{extra}: exit {r.returncode}\n{r.stdout}\n{r.stderr[-3000:]}"
        assert r.stdout.count("case N=") == len(CHILD_CASES)
