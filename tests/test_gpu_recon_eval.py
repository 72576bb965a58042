"""GPU: Stage-I reconstruction evaluation -- the recon_eval kernel against the float64 helper (tests/recon_eval_ref.py) and against the
existing Chamfer modules, and evaluate / validate_net / test_net of tools/runner_autoencoder.py on a tiny Stage-I model over a file-backed
ShapeNet-55 layout."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import recon_eval_ref as R
from tests.golden.fill import TINY_STAGE2, fill_module

pytestmark = pytest.mark.gpu

TH = 0.01
RTOL = 1e-6          # fp32 sqdist3: <= 3e-7 relative on a squared distance, the same on the minimum, half of it + 6e-8 after the square root;
#                      the means are float64.  About 3e-7 (L2) / 2.1e-7 (L1); 1e-6 leaves a factor of three.


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _run(dev, coarse, dense, gt, th=TH, rows=None, row0=0):
    from act_amd import kernels as K
    B = gt.shape[0]
    out = torch.full((rows if rows is not None else B, K.RECON_FIELDS), -7.0, dtype=torch.float64, device=dev)
    K.recon_eval(torch.from_numpy(coarse).to(dev), torch.from_numpy(dense).to(dev), torch.from_numpy(gt).to(dev), out, row0, th)
    return out


def _check_rows(got, coarse, dense, gt, th=TH):
    """assertions 1 and 2 for every cloud; returns (borderline queries, queries)"""
    from act_amd import kernels as K
    border = queries = 0
    for b in range(gt.shape[0]):
        ref = R.ref_row(coarse[b], dense[b], gt[b], th)
        g = got[b]
        print(f"cloud {b}: hits kernel ({g[K.RECON_PRECISION_HITS]:.0f}, {g[K.RECON_RECALL_HITS]:.0f}) ref ({ref['hits_p']}, {ref['hits_r']}) "
              f"borderline ({ref['border_p']}, {ref['border_r']}) F {g[K.RECON_FSCORE]:.6f} / {ref['fscore']:.6f} "
              f"chamfer rel err {[abs(g[i] - ref[k]) / abs(ref[k]) if ref[k] == ref[k] and ref[k] else 0.0 for i, k in enumerate(R.CHAMFER_KEYS)]}")
        assert abs(g[K.RECON_PRECISION_HITS] - ref["hits_p"]) <= ref["border_p"]
        assert abs(g[K.RECON_RECALL_HITS] - ref["hits_r"]) <= ref["border_r"]
        f = R.fscore_from_counts(g[K.RECON_PRECISION_HITS], g[K.RECON_RECALL_HITS], dense.shape[1], gt.shape[1])
        assert abs(g[K.RECON_FSCORE] - f) <= 1e-12
        for i, k in enumerate(R.CHAMFER_KEYS):
            if np.isnan(ref[k]):
                assert np.isnan(g[i]), (b, k, g[i])
            else:
                assert abs(g[i] - ref[k]) <= RTOL * abs(ref[k]), (b, k, g[i], ref[k])
        assert g[K.RECON_NZ_DENSE] == R.nonzero_mask(dense[b]).sum() and g[K.RECON_NZ_GT] == R.nonzero_mask(gt[b]).sum()
        border += ref["border_p"] + ref["border_r"]
        queries += dense.shape[1] + gt.shape[1]
    return border, queries


def _with_zero_cases(coarse, dense, gt):
    """exact-zero rows in dense and gt, a non-zero point with a zero coordinate sum, and a cloud whose gt is all zeros"""
    coarse, dense, gt = coarse.copy(), dense.copy(), gt.copy()
    dense[1, [3, 700, 2047]] = 0.0
    gt[1, [0, 5, 1000]] = 0.0
    gt[2, 17] = (0.375, -0.375, 0.0)                  # removed by ignore_zeros, as in the reference
    dense[2, 40] = (0.5, -0.25, -0.25)
    gt[3] = 0.0                                        # nothing left after the mask: NaN row for CDL1 / CDL2, no fault
    return coarse, dense, gt


def test_rows_match_the_float64_helper(dev):
    coarse, dense, gt = _with_zero_cases(*R.make_clouds(seed=0, B=64))
    got = _run(dev, coarse, dense, gt).cpu().numpy()
    border, queries = _check_rows(got, coarse, dense, gt)
    assert border <= 1e-4 * queries, (border, queries)                 # condition on the inputs: the borderline cap is not what passes the test
    from act_amd import kernels as K
    f = got[:, K.RECON_FSCORE]
    assert f[4:].min() < 0.5 and f.max() > 0.95                        # neither count is trivially 0 or all
    # the ignore_zeros values differ from the unmasked ones exactly where zeros were planted
    assert got[1, K.RECON_CDL1] != got[1, K.RECON_DENSE_L1] and got[2, K.RECON_CDL2] != got[2, K.RECON_DENSE_L2]
    assert np.array_equal(got[4:, K.RECON_CDL1], got[4:, K.RECON_DENSE_L1]) and np.array_equal(got[4:, K.RECON_CDL2], got[4:, K.RECON_DENSE_L2])
    assert np.isnan(got[3, K.RECON_CDL1]) and np.isnan(got[3, K.RECON_CDL2]) and np.isfinite(got[3, :4]).all()


@pytest.mark.parametrize("B,nc,nd,N", [(1, 512, 2048, 1024), (3, 37, 1000, 513), (2, 512, 8192, 8192), (2, 1030, 8197, 8191)])
def test_other_geometries(dev, B, nc, nd, N):
    """batch of one, odd sizes, a size that takes the tiled path, and the tiled path with ragged tiles (last tile not a multiple of 4, query
    counts that are no multiple of the workgroup, barriers inside the query loop)"""
    rs = np.random.RandomState(11)
    gt = np.stack([R.pc_norm(rs.standard_normal((N, 3))) for _ in range(B)]).astype(np.float32)
    reps = -(-nd // N)
    dense = (np.concatenate([gt] * reps, axis=1)[:, :nd] + 0.004 * rs.standard_normal((B, nd, 3))).astype(np.float32)
    coarse = (gt[:, :nc] + 0.004 * rs.standard_normal((B, nc, 3))).astype(np.float32)
    dense[0, 1] = 0.0
    gt[0, 2] = 0.0
    got = _run(dev, coarse, dense, gt).cpu().numpy()
    border, queries = _check_rows(got, coarse, dense, gt)
    assert border <= 1e-4 * queries, (border, queries)                 # condition on the inputs (a geometry that fails it needs another seed)


def test_rows_match_the_existing_chamfer_modules(dev):
    from act_amd import kernels as K
    from act_amd.extensions.chamfer_dist import ChamferDistanceL1, ChamferDistanceL2
    coarse, dense, gt = _with_zero_cases(*R.make_clouds(seed=0, B=64))               # the clouds of test_rows_match_the_float64_helper
    got = _run(dev, coarse, dense, gt).cpu().numpy()
    c, d, g = (torch.from_numpy(x).to(dev) for x in (coarse, dense, gt))
    l1, l2, z1, z2 = ChamferDistanceL1(), ChamferDistanceL2(), ChamferDistanceL1(ignore_zeros=True), ChamferDistanceL2(ignore_zeros=True)
    for b in range(64):
        s = slice(b, b + 1)
        want = [l1(c[s], g[s]).item(), l2(c[s], g[s]).item(), l1(d[s], g[s]).item(), l2(d[s], g[s]).item()]
        if b != 3:                                     # cloud 3 has no gt point left: the module cannot launch on an empty cloud
            want += [z1(d[s], g[s]).item(), z2(d[s], g[s]).item()]
        for i, w in enumerate(want):
            assert abs(got[b, i] - w) <= RTOL * abs(w), (b, i, got[b, i], w)
    # and the per-point minima are the Chamfer kernel's, bit for bit: L2 from its dist1 / dist2 in float64 is the row's value to an ulp
    from act_amd.extensions.chamfer_dist import chamfer
    d1, d2, _, _ = chamfer.forward(d, g)
    want = d1.double().mean(dim=1) + d2.double().mean(dim=1)
    np.testing.assert_allclose(got[:, K.RECON_DENSE_L2], want.cpu().numpy(), rtol=1e-14)


def test_deterministic_and_rows_outside_untouched(dev):
    from act_amd import kernels as K
    coarse, dense, gt = _with_zero_cases(*R.make_clouds(seed=1, B=8))
    a = _run(dev, coarse, dense, gt, rows=20, row0=5)
    b = _run(dev, coarse, dense, gt, rows=20, row0=5)
    finite = ~torch.isnan(a)
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[finite], b[finite])
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))                       # bit-identical, the NaN row included
    assert (a[:5] == -7.0).all() and (a[13:] == -7.0).all() and not (a[5:13, :11] == -7.0).any()
    c = _run(dev, coarse, dense, gt)
    assert torch.equal(c.view(torch.int64), a[5:13].view(torch.int64))
    with pytest.raises(K._C.ActHipError):
        _run(dev, coarse, dense, gt, rows=10, row0=5)                                   # rows 5..12 do not fit a 10-row buffer
    e = torch.full((4, K.RECON_FIELDS), -7.0, dtype=torch.float64, device=dev)
    K.recon_eval(torch.empty(0, 4, 3, device=dev), torch.empty(0, 8, 3, device=dev), torch.empty(0, 8, 3, device=dev), e, 0)     # B == 0: no-op
    assert (e == -7.0).all()


def test_metrics_get_is_the_mean_of_the_kernels_rows(dev):
    from act_amd import kernels as K
    from act_amd.utils.metrics import Metrics
    coarse, dense, gt = _with_zero_cases(*R.make_clouds(seed=2, B=6))
    keep = [0, 1, 2, 4, 5]                                               # cloud 3 has an empty gt after the mask (NaN)
    rows = _run(dev, coarse[keep], dense[keep], gt[keep]).cpu().numpy()
    d, g = torch.from_numpy(dense[keep]).to(dev), torch.from_numpy(gt[keep]).to(dev)
    want = [rows[:, K.RECON_FSCORE].mean(), 1000 * rows[:, K.RECON_CDL1].mean(), 1000 * rows[:, K.RECON_CDL2].mean()]
    np.testing.assert_allclose(Metrics.get(d, g), want, rtol=1e-14)
    np.testing.assert_allclose([Metrics._get_f_score(d, g), Metrics._get_chamfer_distancel1(d, g), Metrics._get_chamfer_distancel2(d, g)], want,
                               rtol=1e-14)
    # one cloud: the reference's own definition (ignore_zeros acts at batch size 1), against the float64 helper
    ref = R.ref_row(coarse[1], dense[1], gt[1])
    one = Metrics.get(d[1:2], g[1:2])
    assert ref["border_p"] + ref["border_r"] == 0 and abs(one[0] - ref["fscore"]) <= 1e-12
    np.testing.assert_allclose(one[1:], [1000 * ref["cdl1"], 1000 * ref["cdl2"]], rtol=RTOL)
    assert Metrics._get_f_score(d[:1], g[:1], th=0.02) >= Metrics._get_f_score(d[:1], g[:1], th=0.005)
    assert np.isnan(Metrics.get(torch.from_numpy(dense[3:4]).to(dev), torch.from_numpy(gt[3:4]).to(dev))[1])


# ---- evaluate / validate_net / test_net on a tiny Stage-I model -------------------------------------------------------------------------
TAXONOMIES = (("02691156", 5), ("03001627", 3), ("99999999", 1))          # macro and micro averages differ; the last is not in the vis list
NPTS = 128


def _layout(tmp):
    """ShapeNet-55 layout: <tmp>/data/test.txt lists <taxonomy>-<model>.npy under <tmp>/pc"""
    os.makedirs(tmp / "data", exist_ok=True)
    os.makedirs(tmp / "pc", exist_ok=True)
    rs = np.random.RandomState(3)
    names = []
    for tax, n in TAXONOMIES:
        for i in range(n):
            names.append(f"{tax}-m{i:03d}.npy")
            np.save(tmp / "pc" / names[-1], (rs.standard_normal((NPTS, 3)) * (0.5, 1.0, 0.75)).astype(np.float32))
    order = rs.permutation(len(names))                                   # taxonomies interleaved in the list
    with open(tmp / "data" / "test.txt", "w") as f:
        f.write("\n".join(names[i] for i in order) + "\n")
    return [names[i].split("-")[0] for i in order]


def _setup(tmp, dev, bs=4):
    from act_amd.models import build_model_from_cfg
    from act_amd.tools import builder
    from act_amd.utils.config import EasyDict
    ids = _layout(tmp)
    mc = dict(TINY_STAGE2["dvae_config"]); mc["NAME"] = "ACTPromptedDiscreteVAEwithVIT"
    ds = dict(_base_=dict(NAME="ShapeNet", N_POINTS=8192, DATA_PATH=str(tmp / "data"), PC_PATH=str(tmp / "pc")),
              others=dict(subset="test", npoints=NPTS, bs=bs))
    cfg = EasyDict(dataset=dict(test=ds, val=ds), model=mc, consider_metric="CDL1")
    args = argparse.Namespace(log_name="test", use_gpu=True, local_rank=0, distributed=False, num_workers=0, experiment_path=str(tmp),
                              ckpts=str(tmp / "ckpt-eval.pth"))
    torch.manual_seed(0)
    model = fill_module(build_model_from_cfg(cfg.model), "recon.").to(dev)
    _, loader = builder.dataset_builder(args, cfg.dataset.test)
    return model, loader, args, cfg, ids


def _evaluate(model, loader, args, cfg, capture=None, **kw):
    from act_amd.tools import runner_autoencoder as RA
    handle = None
    if capture is not None:
        handle = model.register_forward_hook(lambda mod, a, out: capture.append((a[0].cpu().numpy(), out[0].cpu().numpy(), out[1].cpu().numpy(),
                                                                                 out[5].detach().clone())))
    np.random.seed(0)                                                    # the file-backed dataset draws its point subset from numpy's global state
    try:
        return RA.evaluate(model, loader, 0, args, cfg, **kw)
    finally:
        if handle is not None:
            handle.remove()


def _ref_from_capture(cap):
    gt, coarse, dense = (np.concatenate([c[i] for c in cap]) for i in (0, 1, 2))
    return [R.ref_row(coarse[b], dense[b], gt[b]) for b in range(gt.shape[0])]


def test_evaluate_against_the_helper_on_the_models_own_outputs(dev, tmp_path):
    from act_amd import kernels as K
    model, loader, args, cfg, ids = _setup(tmp_path, dev)
    cap = []
    m = _evaluate(model, loader, args, cfg, capture=cap)
    assert m.taxonomy_ids == ids and m.rows.shape == (9, K.RECON_FIELDS) and not model.training
    refs = _ref_from_capture(cap)
    for b, ref in enumerate(refs):
        g = m.rows[b]
        print(f"sample {b}: hits ({g[6]:.0f}, {g[7]:.0f}) ref ({ref['hits_p']}, {ref['hits_r']}) border ({ref['border_p']}, {ref['border_r']})")
        assert abs(g[K.RECON_PRECISION_HITS] - ref["hits_p"]) <= ref["border_p"] and abs(g[K.RECON_RECALL_HITS] - ref["hits_r"]) <= ref["border_r"]
        for i, k in enumerate(R.CHAMFER_KEYS):
            assert abs(g[i] - ref[k]) <= RTOL * abs(ref[k]), (b, k, g[i], ref[k])
    assert sum(r["border_p"] + r["border_r"] for r in refs) == 0        # condition on the inputs: no borderline decision among the 9 clouds
    # the four losses, the per-taxonomy values and the macro average from the helper's rows
    want_losses = [1000 * np.mean([r[k] for r in refs]) for k in R.CHAMFER_KEYS[:4]]
    np.testing.assert_allclose(m.losses, want_losses, rtol=RTOL)
    per = {}
    for t, r in zip(ids, refs):
        per.setdefault(t, []).append([r["fscore"], 1000 * r["cdl1"], 1000 * r["cdl2"]])
    assert {t: c for t, (c, _) in m.per_taxonomy.items()} == dict(TAXONOMIES)
    for t, v in per.items():
        np.testing.assert_allclose(m.per_taxonomy[t][1], np.mean(v, axis=0), rtol=RTOL, atol=1e-12)
    overall = np.mean([np.mean(v, axis=0) for v in per.values()], axis=0)
    np.testing.assert_allclose(list(m.state_dict().values()), overall, rtol=RTOL, atol=1e-12)
    micro = np.mean([v for vs in per.values() for v in vs], axis=0)
    assert abs(overall[1] - micro[1]) > 1e-6 * micro[1]                  # the macro average is not the micro average here
    assert m.metric_name == "CDL1" and list(m.state_dict()) == ['F-Score', 'CDL1', 'CDL2']
    # a second pass returns identical numbers
    m2 = _evaluate(model, loader, args, cfg)
    assert m2.state_dict() == m.state_dict() and m2.losses == m.losses and np.array_equal(m2.rows, m.rows, equal_nan=True)


def test_evaluate_is_batch_size_invariant(dev, tmp_path):
    from act_amd import kernels as K
    from act_amd.tools import runner_autoencoder as RA
    model, loader, args, cfg, ids = _setup(tmp_path, dev)
    cap1, cap4 = [], []
    m1 = _evaluate(model, loader, args, cfg, capture=cap1, batch_size=1)
    m4 = _evaluate(model, loader, args, cfg, capture=cap4, batch_size=4)
    assert len(cap1) == 9 and len(cap4) == 3 and m1.taxonomy_ids == m4.taxonomy_ids == ids
    assert np.array_equal(np.concatenate([c[0] for c in cap1]), np.concatenate([c[0] for c in cap4]))     # the same clouds in the same order
    noise = RA.gumbel_noise(model, range(9), 0, dev)
    codes1 = (torch.cat([c[3] for c in cap1]) + noise).argmax(-1)
    codes4 = (torch.cat([c[3] for c in cap4]) + noise).argmax(-1)
    flipped = [b for b in range(9) if not torch.equal(codes1[b], codes4[b])]
    print("clouds with a flipped hard gumbel selection between batch sizes 1 and 4:", flipped)
    assert len(flipped) <= 1
    for b in range(9):
        if b in flipped:
            continue
        rel = np.abs(m1.rows[b, :6] - m4.rows[b, :6]) / np.abs(m4.rows[b, :6])
        print(f"sample {b}: relative difference of the six Chamfer values {rel}, hits {m1.rows[b, 6:8]} / {m4.rows[b, 6:8]}")
        assert (rel <= 1e-4).all(), (b, rel)
        # hit counts: outputs that agree to a relative 1e-4 move a distance by at most about 2e-4 of the unit-ball scale in absolute terms
        # (two points); only queries within that band of th can decide differently
        gt, dense = np.concatenate([c[0] for c in cap4])[b], np.concatenate([c[2] for c in cap4])[b]
        band_p = int((np.abs(np.sqrt(R.nn_sq(dense, gt)) - TH) <= 2e-4).sum())
        band_r = int((np.abs(np.sqrt(R.nn_sq(gt, dense)) - TH) <= 2e-4).sum())
        assert abs(m1.rows[b, K.RECON_PRECISION_HITS] - m4.rows[b, K.RECON_PRECISION_HITS]) <= band_p
        assert abs(m1.rows[b, K.RECON_RECALL_HITS] - m4.rows[b, K.RECON_RECALL_HITS]) <= band_r
        # the F-Score of either row is the function of that row's own counts; with equal counts the two are the same number
        for m in (m1, m4):
            f = R.fscore_from_counts(m.rows[b, K.RECON_PRECISION_HITS], m.rows[b, K.RECON_RECALL_HITS], dense.shape[0], gt.shape[0])
            assert abs(m.rows[b, K.RECON_FSCORE] - f) <= 1e-12
        if np.array_equal(m1.rows[b, 6:8], m4.rows[b, 6:8]):
            assert m1.rows[b, K.RECON_FSCORE] == m4.rows[b, K.RECON_FSCORE]


def test_per_batch_part_does_not_synchronise(dev, tmp_path):
    from act_amd import kernels as K
    from act_amd.tools import runner_autoencoder as RA
    model, loader, args, cfg, ids = _setup(tmp_path, dev)
    model.eval()
    np.random.seed(0)
    batches = [data.to(dev) for _, _, data in loader]                    # device-resident batches
    out = torch.zeros(9, K.RECON_FIELDS, dtype=torch.float64, device=dev)
    row0 = 0
    for p in batches:                                                    # warm-up pass (first-use GEMM tuning, allocations)
        RA.eval_batch(model, p, out, row0)
        row0 += p.shape[0]
    warm = out.cpu()
    out.zero_()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        row0 = 0
        for p in batches:
            RA.eval_batch(model, p, out, row0)
            row0 += p.shape[0]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = out.cpu()                                                      # the single read, outside the guarded region
    assert torch.equal(got.view(torch.int64), warm.view(torch.int64)) and torch.isfinite(got[:, :4]).all()


def test_validate_net_and_test_net_from_a_checkpoint(dev, tmp_path):
    from act_amd.tools import builder
    from act_amd.tools import runner_autoencoder as RA
    model, loader, args, cfg, ids = _setup(tmp_path, dev)
    live = _evaluate(model, loader, args, cfg)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    args.ckpts = os.path.join(str(tmp_path), "ckpt-eval.pth")
    builder.save_checkpoint(model, opt, 7, RA.Metrics("CDL1", {"CDL1": 1.0, "CDL2": 2.0}), None, "ckpt-eval", args)
    np.random.seed(0)
    m = RA.validate_net(args, cfg)
    assert m.state_dict() == live.state_dict() and m.losses == live.losses and m.per_taxonomy == live.per_taxonomy
    with pytest.raises(NotImplementedError):
        RA.validate_net(argparse.Namespace(**dict(vars(args), distributed=True)), cfg)
    # test_net: gt.txt / dense_points.txt of the listed categories, readable back bit for bit
    cap = []
    from act_amd.models.dvae import ACTPromptedDiscreteVAEwithVIT        # the model is built inside test_net: hook every module of that class
    h = torch.nn.modules.module.register_module_forward_hook(
        lambda mod, a, out: cap.append((a[0].cpu().numpy(), out[1].cpu().numpy())) if isinstance(mod, ACTPromptedDiscreteVAEwithVIT) else None)
    np.random.seed(0)
    try:
        written = RA.test_net(args, cfg, target=str(tmp_path / "vis"))
    finally:
        h.remove()
    gt, dense, k = {}, {}, 0                                             # sample index -> cloud; a batch without a listed category is not run
    for b0 in range(0, len(ids), 4):
        if any(t in RA.USEFUL_CATE for t in ids[b0:b0 + 4]):
            for r in range(len(ids[b0:b0 + 4])):
                gt[b0 + r], dense[b0 + r] = cap[k][0][r], cap[k][1][r]
            k += 1
    assert k == len(cap)
    want = [f"{t}_{i}" for i, t in enumerate(ids) if t in RA.USEFUL_CATE]
    assert len(want) == 8 and sorted(os.path.basename(w) for w in written) == sorted(want) == sorted(os.listdir(tmp_path / "vis"))
    for name in want:
        i = int(name.split("_")[1])
        back_gt = np.loadtxt(tmp_path / "vis" / name / "gt.txt", delimiter=";").astype(np.float32)
        back_dense = np.loadtxt(tmp_path / "vis" / name / "dense_points.txt", delimiter=";").astype(np.float32)
        assert np.array_equal(back_gt, gt[i]) and np.array_equal(back_dense, dense[i])
        try:
            import matplotlib  # noqa: F401
            assert os.path.getsize(tmp_path / "vis" / name / "plot.png") > 0
        except ImportError:
            pass
    with pytest.raises(NotImplementedError):
        RA.test_net(argparse.Namespace(**dict(vars(args), distributed=True)), cfg, target=str(tmp_path / "vis2"))
