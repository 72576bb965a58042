"""CPU: the host side of the Stage-I reconstruction evaluation -- the ``Metrics`` surface, the per-taxonomy aggregation and its table, the
synthetic dataset's opt-in taxonomy ids, the float64 helper the GPU tests compare against, and the build of the kernel."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import recon_eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_metrics_surface_and_ordering():
    from act_amd.utils.metrics import Metrics
    assert Metrics.names() == ['F-Score', 'CDL1', 'CDL2'] and [i['name'] for i in Metrics.items()] == Metrics.names()
    assert [i['init_value'] for i in Metrics.ITEMS] == [0, 32767, 32767]
    assert [i['is_greater_better'] for i in Metrics.ITEMS] == [True, False, False]
    a, b = Metrics('F-Score', [0.5, 10.0, 3.0]), Metrics('F-Score', [0.4, 9.0, 2.0])
    assert a.better_than(b) and not b.better_than(a) and a.better_than(None)
    a, b = Metrics('CDL1', [0.5, 10.0, 3.0]), Metrics('CDL1', [0.4, 9.0, 4.0])
    assert b.better_than(a) and not a.better_than(b)
    a, b = Metrics('CDL2', [0.5, 10.0, 3.0]), Metrics('CDL2', [0.4, 9.0, 4.0])
    assert a.better_than(b) and not b.better_than(a)
    assert a.state_dict() == {'F-Score': 0.5, 'CDL1': 10.0, 'CDL2': 3.0} and repr(a) == str(a.state_dict())
    d = Metrics('CDL1', {'CDL2': 2.0, 'F-Score': 0.25, 'CDL1': 7.0})
    assert d.state_dict() == {'F-Score': 0.25, 'CDL1': 7.0, 'CDL2': 2.0}
    with pytest.raises(TypeError):
        Metrics('CDL1', 3.0)
    with pytest.raises(ValueError):
        Metrics('EMD', [0, 0, 0]).better_than(a)


def test_metrics_loads_the_cdl_only_dict_of_run_net_checkpoints():
    from act_amd.utils.metrics import Metrics
    from act_amd.tools.runner_autoencoder import Metrics as RunnerMetrics
    saved = RunnerMetrics("CDL1", {"CDL1": 12.5, "CDL2": 0.75}).state_dict()          # what run_net's checkpoints hold
    m = Metrics('CDL1', saved)
    assert m.state_dict() == {'F-Score': 0, 'CDL1': 12.5, 'CDL2': 0.75}
    assert m.better_than(Metrics('CDL1', {})) and Metrics('CDL1', {}).state_dict() == {'F-Score': 0, 'CDL1': 32767, 'CDL2': 32767}
    assert Metrics('CDL1', [0.9, 12.0, 0.7]).better_than(m)


class _Meter:
    """AverageMeter of the reference (utils/AverageMeter.py) for a list of items: running sum and count per item"""

    def __init__(self, n):
        self.s, self.c = [0.0] * n, [0] * n

    def update(self, values):
        for i, v in enumerate(values):
            self.s[i] += v
            self.c[i] += 1

    def avg(self):
        return [s / c for s, c in zip(self.s, self.c)]


def test_aggregation_is_the_references_macro_average():
    from act_amd import kernels as K
    from act_amd.tools.runner_autoencoder import aggregate_rows, results_table
    rs = np.random.RandomState(5)
    ids = ["02691156"] * 5 + ["03001627"] * 3 + ["04379243"]
    ids = [ids[i] for i in rs.permutation(len(ids))]
    rows = rs.rand(len(ids), K.RECON_FIELDS)
    agg = aggregate_rows(rows, ids)
    # transcription of runner_autoencoder.py:255-283
    test_losses, test_metrics, category = _Meter(4), _Meter(3), {}
    for r, t in zip(rows, ids):
        test_losses.update([r[0] * 1000, r[1] * 1000, r[2] * 1000, r[3] * 1000])
        _metrics = [r[K.RECON_FSCORE], r[K.RECON_CDL1] * 1000, r[K.RECON_CDL2] * 1000]
        if t not in category:
            category[t] = _Meter(3)
        category[t].update(_metrics)
    for _, v in category.items():
        test_metrics.update(v.avg())
    np.testing.assert_allclose(agg["losses"], test_losses.avg(), rtol=1e-13)
    np.testing.assert_allclose(agg["overall"], test_metrics.avg(), rtol=1e-13)
    assert list(agg["per_taxonomy"]) == list(category)                                   # order of first appearance, as the reference's dict
    for t, v in category.items():
        assert agg["per_taxonomy"][t][0] == v.c[0] == ids.count(t)
        np.testing.assert_allclose(agg["per_taxonomy"][t][1], v.avg(), rtol=1e-13)
    micro = rows[:, K.RECON_FSCORE].mean()
    assert abs(agg["overall"][0] - micro) > 1e-6                                         # 5 / 3 / 1 samples: macro and micro averages differ
    text = results_table(agg["per_taxonomy"], agg["overall"], synset={"02691156": "airplane", "03001627": "chair"})
    lines = [l for l in text.splitlines() if l.startswith("|")]
    cells = [[c.strip() for c in l.strip("|").split("|")] for l in lines]
    assert cells[0] == ['Taxonomy', '#Sample', 'F-Score', 'CDL1', 'CDL2', 'Category']
    assert [c[0] for c in cells[1:]] == list(category) + ['Overall']
    for c in cells[1:-1]:
        assert c[1] == str(ids.count(c[0])) and c[2:5] == ['%.3f' % v for v in category[c[0]].avg()]
        assert c[5] == {"02691156": "airplane", "03001627": "chair"}.get(c[0], c[0])     # no name known: the taxonomy id
    assert cells[-1] == ['Overall', '--'] + ['%.3f' % v for v in test_metrics.avg()] + ['--']
    with pytest.raises(ValueError):
        aggregate_rows(rows, ids[:-1])


def test_synthetic_taxonomies_are_opt_in():
    from act_amd.datasets.SyntheticDataset import ShapeNet, pc_norm
    from act_amd.utils.config import EasyDict
    base = dict(NAME="ShapeNet", N_POINTS=8192, SYNTHETIC=True, NUM_SAMPLES=12, DATA_PATH="none", PC_PATH="none", subset="test", npoints=64)
    plain = ShapeNet(EasyDict(base))
    for idx in (0, 5, 11):
        tax, mid, pts = plain[idx]
        g = np.random.RandomState(((1234 + 1) * 1000003 + idx) & 0x7FFFFFFF)               # today's generator, restated
        want = pc_norm(g.standard_normal((64, 3))).astype(np.float32)
        assert tax == "synthetic" and mid == f"{idx:06d}" and np.array_equal(pts.numpy(), want)
    spread = ShapeNet(EasyDict(dict(base, NUM_TAXONOMIES=3)))
    assert len(spread) == 12 and sorted({spread[i][0] for i in range(12)}) == ["synthetic00", "synthetic01", "synthetic02"]
    for idx in (0, 5, 11):
        assert spread[idx][1] == plain[idx][1] and torch.equal(spread[idx][2], plain[idx][2])


def test_helper_matches_a_float64_kd_tree():
    from scipy.spatial import cKDTree
    coarse, dense, gt = R.make_clouds(seed=0, B=4)
    for b in range(4):
        for a, c in ((dense[b], gt[b]), (gt[b], dense[b]), (coarse[b], gt[b]), (gt[b], coarse[b])):
            d_tree, _ = cKDTree(c.astype(np.float64)).query(a.astype(np.float64), k=1)
            np.testing.assert_allclose(np.sqrt(R.nn_sq(a, c)), d_tree, rtol=0, atol=1e-12)
    x = np.array([[0, 0, 0], [0.25, -0.25, 0], [1e-3, 0, 0], [0.1, 0.2, -0.3]], np.float32)
    assert R.nonzero_mask(x).tolist() == [False, False, True, bool(np.float32(np.float32(0.1) + np.float32(0.2)) + np.float32(-0.3) != 0)]
    r = R.ref_row(coarse[0], dense[0], np.zeros_like(gt[0]))
    assert np.isnan(r["cdl1"]) and np.isnan(r["cdl2"]) and np.isfinite(r["dense_l1"])


def test_recipe_makes_every_metric_informative():
    """the inputs of the GPU test: F-Score spread over the clouds, borderline threshold decisions rare"""
    coarse, dense, gt = R.make_clouds(seed=0, B=8)
    rows = [R.ref_row(coarse[b], dense[b], gt[b]) for b in range(8)]
    f = [r["fscore"] for r in rows]
    assert min(f) < 0.5 and max(f) > 0.95
    queries = 8 * (dense.shape[1] + gt.shape[1])
    assert sum(r["border_p"] + r["border_r"] for r in rows) <= 1e-4 * queries


def test_kernel_builds_for_gfx950_without_scratch(tmp_path):
    """recon_eval.hip compiles with the project's flags, without register spills or scratch, and is built with contraction off"""
    from act_amd import build as B
    assert B.PER_FILE.get("recon_eval.hip") == ["-ffp-contract=off"] and "recon_eval.hip" in B.sources()
    cmd = [B.hipcc()] + B.COMMON + B.PER_FILE["recon_eval.hip"] + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                                  os.path.join(B.CSRC, "recon_eval.hip"), "-o", str(tmp_path / "recon_eval.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    kernels = re.findall(r"Function Name: (\S*recon_eval_kernel\S*)", r.stderr)
    assert len(kernels) == 2, r.stderr                                                   # resident and tiled
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)] == [0, 0]
    assert [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)] == [0, 0]
    assert all(int(v) <= 256 for v in re.findall(r" VGPRs: (\d+)", r.stderr))


def test_op_refuses_cpu_tensors_and_is_bound():
    import act_amd._C as C
    from act_amd import kernels as K
    assert "act_recon_eval_f32" in C.SIGNATURES and hasattr(C.lib, "act_recon_eval_f32")
    src = open(os.path.join(ROOT, "include", "act_hip.h")).read()
    assert int(re.search(r"#define ACT_RECON_FIELDS (\d+)", src).group(1)) == K.RECON_FIELDS
    with pytest.raises(C.ActHipError):
        K.recon_eval(torch.zeros(1, 4, 3), torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), torch.zeros(1, K.RECON_FIELDS, dtype=torch.float64), 0)
    import act_amd.tools as T
    from act_amd.tools import runner_autoencoder as RA
    assert T.token_val_net is RA.validate_net and T.token_test_net is RA.test_net
