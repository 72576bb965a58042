"""GPU: PointNet++ set abstraction -- the kernels of csrc/sa.hip (ball query, grouped rows and their deterministic backward, channel-first
grouping), the pointnet2_ops surface over them, and models/pointnet2.py against the reference's recorded run (tests/golden/g25_sa.npz).

Ball query is compared index for index: the clouds sit on the 1/8 lattice, where every squared distance is exact in float32 in the expanded
and in the difference form, so tests/sa_ref.py (checked against the reference's query_ball_point on the host) is an exact oracle, points
on the sphere included.  Sizes are the smallest that take each path of the kernels: one past a 64-lane step, one past the LDS chunk (1024
points), a ragged last workgroup (4 queries per workgroup), one past an adjacency chunk (2048 entries) and more than one 256-point block."""
import numpy as np
import pytest
import torch

from tests import sa_ref as R
from tests.conftest import golden
from tests.golden.fill import fill_module
from tests.test_gpu_dense import TOL, _rel

pytestmark = pytest.mark.gpu

CHUNK = 1024                    # SA_BQ_CHUNK of csrc/sa.hip
RADIUS = 0.75                   # r^2 = 36/64: (6,0,0)/8 and (4,4,2)/8 lie exactly on the sphere


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def K(dev):
    import act_amd.kernels as K
    return K


@pytest.fixture(scope="module")
def pu(dev):
    from act_amd.pointnet2_ops import pointnet2_utils as pu
    return pu


@pytest.fixture(scope="module")
def g():
    return golden("g25_sa")


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)


def _check_bq(K, dev, xyz, q, radius, ns):
    """both radius rules against the restatement: idx and cnt with torch.equal"""
    out = []
    for inclusive in (True, False):
        want_idx, want_cnt = R.ball_query(xyz, q, radius, ns, inclusive)
        idx, cnt = K.ball_query(_d(xyz, dev), _d(q, dev), radius, ns, inclusive=inclusive, want_cnt=True)
        assert idx.dtype == torch.int32 and cnt.dtype == torch.int32
        assert torch.equal(cnt.cpu(), torch.from_numpy(want_cnt)), (inclusive, ns)
        assert torch.equal(idx.cpu(), torch.from_numpy(want_idx)), (inclusive, ns)
        assert torch.equal(K.ball_query(_d(xyz, dev), _d(q, dev), radius, ns, inclusive=inclusive), idx)
        out.append((want_idx, want_cnt))
    return out


# ---- ball query ---------------------------------------------------------------------------------------------------------------------------
def _lattice_case(N, S, seed):
    """B = 3 clouds on the 1/8 lattice in [-1, 1]; the queries are cloud points (as FPS picks them); for N >= 2 the last point of every
    cloud is planted exactly on the sphere of query 0"""
    rs = np.random.RandomState(seed)
    xyz = R.lattice_cloud(rs, 3, N, -1.0, 1.0)
    q = np.stack([xyz[b, rs.randint(0, N, size=S)] for b in range(3)])
    if N >= 2:
        q[:, 0] = xyz[:, 0]
        xyz[:, N - 1] = q[:, 0] + np.array([RADIUS, 0, 0], np.float32)
    return xyz, q


BQ_CASES = [(1, 1, 1), (1, 7, 5), (63, 7, 5), (64, 1, 64), (64, 7, 1), (65, 7, 200), (130, 7, 64), (130, 1, 1), (130, 7, 200),
            (CHUNK + 1, 7, 5), (CHUNK + 1, 1, 64), (CHUNK + 1, 7, 200)]


@pytest.mark.parametrize("N,S,ns", BQ_CASES)
def test_ball_query_equals_the_restatement(K, dev, N, S, ns):
    xyz, q = _lattice_case(N, S, 100 + N + 7 * S + ns)
    _check_bq(K, dev, xyz, q, RADIUS, ns)
    if N >= 2:                                                          # a point on the sphere: the two rules see different hit sets
        full_in, full_ex = (R.ball_query(xyz, q, RADIUS, N, inc)[1] for inc in (True, False))
        assert (full_in > full_ex).any()


@pytest.mark.parametrize("tag", ["wide", "dense"])
def test_ball_query_equals_the_reference_run(K, pu, dev, g, tag):
    xyz, q = g[f"{tag}_xyz"], g[f"{tag}_new_xyz"]
    for qi, (r, ns) in enumerate(zip(g["query_radius"], g["query_nsample"])):
        idx = K.ball_query(_d(xyz, dev), _d(q, dev), float(r), int(ns), inclusive=True)
        assert torch.equal(idx.cpu(), torch.from_numpy(g[f"{tag}_idx{qi}"]))
        up = pu.ball_query(float(r), int(ns), _d(xyz, dev), _d(q, dev))                    # upstream's rule: the exclusive one
        assert torch.equal(up.cpu(), torch.from_numpy(R.ball_query(xyz, q, float(r), int(ns), False)[0]))


def test_ball_query_cut_inside_a_ballot_and_all_coincident(K, dev):
    """all N points coincide with the query: N hits.  nsample 5 / 100 cut the hits in the middle of the first / second 64-lane ballot,
    nsample 200 > N keeps all 130 and pads with the first"""
    xyz = np.full((3, 130, 3), 0.25, np.float32)
    q = np.full((3, 2, 3), 0.25, np.float32)
    for ns, kept in ((5, 5), (100, 100), (200, 130)):
        (idx, cnt), _ = _check_bq(K, dev, xyz, q, 0.5, ns)
        assert cnt.tolist() == [[kept, kept]] * 3 and idx[0, 0, :kept].tolist() == list(range(kept)) and (idx[0, 0, kept:] == 0).all()


def test_ball_query_hits_across_chunks_and_a_query_without_hits(K, dev):
    """the hits of query 0 sit at indices 3, CHUNK + 6, 2 CHUNK + 12, 2 CHUNK + 13: its nsample-th hit lies two chunks after its first;
    query 1 reaches nothing: a row of zeros and cnt 0"""
    N = 2 * CHUNK + 52
    hits = [3, CHUNK + 6, 2 * CHUNK + 12, 2 * CHUNK + 13]
    xyz = np.full((3, N, 3), 2.0, np.float32)
    xyz[:, hits] = np.array([0.125, -0.25, 0.5], np.float32)
    xyz[:, hits[1], 0] += 0.5                                           # exactly on the sphere of radius 0.5
    q = np.zeros((3, 2, 3), np.float32)
    q[:, 0] = [0.125, -0.25, 0.5]
    q[:, 1] = [-2.0, -2.0, -2.0]
    for ns in (1, 3, 4, 5):
        (idx_in, cnt_in), (idx_ex, cnt_ex) = _check_bq(K, dev, xyz, q, 0.5, ns)
        assert idx_in[1, 0].tolist() == (hits + [3] * ns)[:max(ns, 4)][:ns] and cnt_in[1].tolist() == [min(ns, 4), 0]
        assert (idx_in[:, 1] == 0).all() and (idx_ex[:, 1] == 0).all()
        assert cnt_ex[1, 0] == min(ns, 3)


def test_ball_query_on_a_random_float_cloud(K, dev):
    """no lattice: compare with float64 distances, leaving out the queries that have a point within 1e-6 (relative) of the radius, where the
    float32 test may legitimately fall on the other side; at most 1 % of the queries may be left out"""
    rs = np.random.RandomState(7)
    B, N, S, ns, radius = 2, 700, 100, 16, np.float32(0.3)
    xyz = rs.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    q = np.stack([xyz[b, rs.choice(N, S, replace=False)] for b in range(B)])
    d = np.sqrt(((q[:, :, None, :].astype(np.float64) - xyz[:, None, :, :].astype(np.float64)) ** 2).sum(-1))
    r = float(radius)
    unsafe = (np.abs(d - r) <= 1e-6 * r).any(-1)                        # [B,S]
    print("[sa] random cloud: %d of %d queries excluded" % (unsafe.sum(), unsafe.size))
    assert unsafe.mean() <= 0.01
    want = np.zeros((B, S, ns), np.int32)
    want_cnt = np.zeros((B, S), np.int32)
    for b in range(B):
        for s in range(S):
            h = np.flatnonzero(d[b, s] < r)[:ns]
            want_cnt[b, s] = len(h)
            want[b, s, :len(h)] = h
            want[b, s, len(h):] = h[0]
    for inclusive in (True, False):
        idx, cnt = K.ball_query(_d(xyz, dev), _d(q, dev), r, ns, inclusive=inclusive, want_cnt=True)
        keep = torch.from_numpy(~unsafe)
        assert torch.equal(idx.cpu()[keep], torch.from_numpy(want)[keep]) and torch.equal(cnt.cpu()[keep], torch.from_numpy(want_cnt)[keep])


# ---- grouping -------------------------------------------------------------------------------------------------------------------------------
B_, N_, S_, NS_ = 2, 300, 50, 50                # E = 2500: one past an adjacency chunk; N = 300: two 256-point blocks


@pytest.fixture(scope="module")
def grp():
    """shared grouping problem: half of the entries fall on ten points (heavy repetition), points 280.. are never gathered"""
    rs = np.random.RandomState(11)
    idx = rs.randint(0, 280, size=(B_, S_, NS_))
    heavy = rs.rand(B_, S_, NS_) < 0.5
    idx[heavy] = rs.randint(0, 10, size=int(heavy.sum())) * 29
    spread = rs.randint(0, 280, size=(B_, S_, NS_))                      # the float comparisons: ~9 rows per point
    xyz = rs.standard_normal((B_, N_, 3)).astype(np.float32)
    q = rs.standard_normal((B_, S_, 3)).astype(np.float32)
    return dict(idx=idx.astype(np.int32), spread=spread.astype(np.int32), xyz=xyz, q=q, rs=rs)


def _torch_rows(xyz, q, feat, idx, use_xyz):
    bi = torch.arange(idx.shape[0])[:, None, None]
    parts = []
    if use_xyz:
        parts.append(xyz[bi, idx.long()] - q[:, :, None, :])
    if feat is not None:
        parts.append(feat[bi, idx.long()])
    return torch.cat(parts, dim=-1).reshape(idx.numel(), -1)


@pytest.mark.parametrize("D,use_xyz", [(0, True), (5, True), (5, False), (64, True), (67, False)])
def test_group_rows_forward_equals_torch_indexing(K, dev, grp, D, use_xyz):
    rs = np.random.RandomState(20 + D)
    xyz, q, idx = (torch.from_numpy(grp[k]) for k in ("xyz", "q", "idx"))
    feat = torch.from_numpy(rs.standard_normal((B_, N_, D)).astype(np.float32)) if D else None
    want = _torch_rows(xyz, q, feat, idx, use_xyz)
    got = K.group_rows(xyz.to(dev), q.to(dev), None if feat is None else feat.to(dev), idx.to(dev), use_xyz=use_xyz)
    assert got.shape == (B_ * S_ * NS_, (3 if use_xyz else 0) + D) and torch.equal(got.cpu(), want)
    got64 = K.group_rows(xyz.to(dev), q.to(dev), None if feat is None else feat.to(dev), idx.to(dev).long(), use_xyz=use_xyz)
    assert torch.equal(got64, got)


def _rows_grad(K, dev, grp, idx, feat, cot, use_xyz):
    f = feat.to(dev).requires_grad_(True)
    rows = K.group_rows(torch.from_numpy(grp["xyz"]).to(dev), torch.from_numpy(grp["q"]).to(dev), f, idx.to(dev), use_xyz=use_xyz)
    (gf,) = torch.autograd.grad(rows, f, cot.to(dev))
    return gf.cpu()


def _index_add64(cot_feat, idx, N):
    """cot_feat [B, E, D] float64 -> [B, N, D]"""
    out = torch.zeros(idx.shape[0], N, cot_feat.shape[-1], dtype=torch.float64)
    for b in range(idx.shape[0]):
        out[b].index_add_(0, idx[b].reshape(-1).long(), cot_feat[b])
    return out


@pytest.mark.parametrize("D,use_xyz", [(5, True), (64, False), (67, True)])
def test_group_rows_backward(K, dev, grp, D, use_xyz):
    X = 3 if use_xyz else 0
    rs = np.random.RandomState(30 + D)
    feat = torch.from_numpy(rs.standard_normal((B_, N_, D)).astype(np.float32))
    E = S_ * NS_
    # integer-valued cotangents: every partial sum is an integer below 2^24, so any order is exact
    idx = torch.from_numpy(grp["idx"])
    cot = torch.from_numpy(rs.randint(-8, 9, size=(B_ * E, X + D)).astype(np.float32))
    want = _index_add64(cot.double().view(B_, E, X + D)[:, :, X:], idx, N_)
    got = _rows_grad(K, dev, grp, idx, feat, cot, use_xyz)
    assert torch.equal(got.double(), want)
    assert (got[:, 280:] == 0).all() and np.bincount(grp["idx"][0].ravel()).max() > 100       # untouched points; one point gathered > 100 times
    # random floats: bit-identical twice in a row, and within 1e-6 (relative to the largest entry) of a float64 index_add_
    idx = torch.from_numpy(grp["spread"])
    cot = torch.from_numpy(rs.standard_normal((B_ * E, X + D)).astype(np.float32))
    got = _rows_grad(K, dev, grp, idx, feat, cot, use_xyz)
    again = _rows_grad(K, dev, grp, idx, feat, cot, use_xyz)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    want = _index_add64(cot.double().view(B_, E, X + D)[:, :, X:], idx, N_)
    rel = _rel(got, want)
    print("[sa] group_rows backward D=%d: rel err vs float64 = %.3e" % (D, rel))
    assert rel <= 1e-6
    assert np.array_equal(got.numpy(), R.group_rows_bwd(cot.numpy(), idx.numpy(), N_, D, use_xyz))       # the kernel's own order, bit for bit


def test_grouping_operation_forward_and_backward(K, pu, dev, grp):
    rs = np.random.RandomState(40)
    C, E = 6, S_ * NS_
    feats = torch.from_numpy(rs.standard_normal((B_, C, N_)).astype(np.float32))
    idx = torch.from_numpy(grp["idx"])
    want = torch.stack([feats[b][:, idx[b].long()] for b in range(B_)])
    f = feats.to(dev).requires_grad_(True)
    out = pu.grouping_operation(f, idx.to(dev))
    assert out.shape == (B_, C, S_, NS_) and torch.equal(out.cpu(), want)
    cot = torch.from_numpy(rs.randint(-8, 9, size=(B_, C, S_, NS_)).astype(np.float32))
    (gf,) = torch.autograd.grad(out, f, cot.to(dev))
    want_g = _index_add64(cot.double().view(B_, C, E).transpose(1, 2), idx, N_).transpose(1, 2)
    assert torch.equal(gf.cpu().double(), want_g) and (gf[:, :, 280:] == 0).all()
    idx = torch.from_numpy(grp["spread"])
    cot = torch.from_numpy(rs.standard_normal((B_, C, S_, NS_)).astype(np.float32))
    grads = []
    for _ in range(2):
        f = feats.to(dev).requires_grad_(True)
        grads.append(torch.autograd.grad(pu.grouping_operation(f, idx.to(dev)), f, cot.to(dev))[0].cpu())
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))
    want_g = _index_add64(cot.double().view(B_, C, E).transpose(1, 2), idx, N_).transpose(1, 2)
    rel = _rel(grads[0], want_g)
    print("[sa] grouping_operation backward: rel err vs float64 = %.3e" % rel)
    assert rel <= 1e-6


def test_query_and_group_and_group_all_are_their_compositions(K, pu, dev, g):
    xyz, q, feat = (_d(g[k], dev) for k in ("dense_xyz", "dense_new_xyz", "dense_feat"))
    feats = feat.transpose(1, 2).contiguous()                           # [B, C, N]
    idx = pu.ball_query(0.5, 8, xyz, q)
    gx = pu.grouping_operation(xyz.transpose(1, 2).contiguous(), idx) - q.transpose(1, 2).unsqueeze(-1)
    gf = pu.grouping_operation(feats, idx)
    assert torch.equal(pu.QueryAndGroup(0.5, 8)(xyz, q, feats), torch.cat([gx, gf], dim=1))
    assert torch.equal(pu.QueryAndGroup(0.5, 8, use_xyz=False)(xyz, q, feats), gf)
    assert torch.equal(pu.QueryAndGroup(0.5, 8)(xyz, q), gx)
    # the row form holds the same numbers: [B*S*ns, 3+C] against [B, 3+C, S, ns]
    rows = K.group_rows(xyz, q, feat, idx)
    assert torch.equal(rows.view(3, 7, 8, 7).permute(0, 3, 1, 2), torch.cat([gx, gf], dim=1))
    ga = pu.GroupAll()(xyz, None, feats)
    assert ga.shape == (3, 7, 1, 96) and torch.equal(ga[:, :3, 0], xyz.transpose(1, 2)) and torch.equal(ga[:, 3:, 0], feats)
    assert torch.equal(pu.GroupAll(use_xyz=False)(xyz, None, feats), feats.unsqueeze(2))
    assert torch.equal(pu.GroupAll()(xyz, None), xyz.transpose(1, 2).unsqueeze(2))


# ---- modules ------------------------------------------------------------------------------------------------------------------------------------
def _module(tag, dev):
    from tests.golden.make_golden_sa import SA, MSG, SA_ALL, SA_XYZ
    from act_amd.models import pointnet2 as P
    cls, kw = {"sa": (P.PointNetSetAbstraction, SA), "msg": (P.PointNetSetAbstractionMsg, MSG), "all": (P.PointNetSetAbstraction, SA_ALL),
               "xyzonly": (P.PointNetSetAbstraction, SA_XYZ)}[tag]
    return fill_module(cls(**kw), f"g25.{tag}.").to(dev).train()


@pytest.mark.parametrize("tag", ["sa", "msg", "all", "xyzonly"])
def test_modules_equal_the_reference_run(dev, g, tag):
    """train-mode outputs, running statistics and every gradient within the project's bar of the reference's float32 run; then eval mode with
    the updated statistics; a second train-mode pass is bit-identical"""
    model = _module(tag, dev)
    xyz = _d(g["xyz"], dev).transpose(1, 2)
    pts = None if tag == "xyzonly" else _d(g["points"], dev).transpose(1, 2).clone().requires_grad_(True)
    kw = {} if tag == "all" else dict(fps_idx=_d(g["fps_idx"], dev))
    new_xyz, out = model(xyz, pts, **kw)
    assert new_xyz.shape == g[f"{tag}.new_xyz"].shape and out.shape == g[f"{tag}.out"].shape
    assert torch.equal(new_xyz.cpu(), torch.from_numpy(g[f"{tag}.new_xyz"]))
    errs = {"out": _rel(out, torch.from_numpy(g[f"{tag}.out"]))}
    if f"{tag}_cot" in g.files:                                         # the two layers whose gradients the fixture records (see make_golden_sa.py)
        (out * _d(g[f"{tag}_cot"], dev)).sum().backward()
        for n, p in model.named_parameters():
            errs["grad." + n] = _rel(p.grad, torch.from_numpy(g[f"{tag}.grad.{n}"]))
        errs["grad_points"] = _rel(pts.grad, torch.from_numpy(g[f"{tag}.grad_points"]))
    assert ("grad_points" in errs) == (tag in ("sa", "msg"))
    for n, b in model.named_buffers():
        if n.endswith("running_mean") or n.endswith("running_var"):
            errs["buf." + n] = _rel(b, torch.from_numpy(g[f"{tag}.buf.{n}"]))
    model.eval()
    with torch.no_grad():
        errs["out_eval"] = _rel(model(xyz, pts, **kw)[1], torch.from_numpy(g[f"{tag}.out_eval"]))
    print("[sa] %s: worst %s = %.3e" % (tag, max(errs, key=errs.get), max(errs.values())))
    assert max(errs.values()) < TOL, errs
    model.train()
    with torch.no_grad():
        again = model(xyz, pts, **kw)[1]
    assert torch.equal(again.view(torch.int32), out.detach().view(torch.int32))


def test_reference_state_dict_loads_strictly_and_default_fps_starts_at_zero(dev, g, pu):
    from tests.golden.fill import fill_tensor
    model = _module("msg", dev)
    sd = {k: fill_tensor("other." + k, [int(x) for x in s.split(",") if x]) if not k.endswith("num_batches_tracked") else torch.tensor(3)
          for k, s in zip(g["msg_sd_keys"].tolist(), g["msg_sd_shapes"].tolist())}
    sd = {k: v.abs() + 0.5 if k.endswith("running_var") else v for k, v in sd.items()}
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(model.conv_blocks[1][0].weight.cpu(), sd["conv_blocks.1.0.weight"])
    xyz = _d(g["xyz"], dev).transpose(1, 2)
    pts = _d(g["points"], dev).transpose(1, 2)
    model.eval()
    with torch.no_grad():
        new_xyz, out = model(xyz, pts)
        fps = pu.furthest_point_sample(xyz.transpose(1, 2).contiguous(), 16, skip_near_origin=False)
        new_xyz2, out2 = model(xyz, pts, fps_idx=fps)
    assert (fps[:, 0] == 0).all() and torch.equal(new_xyz[:, :, 0], xyz[:, :, 0])
    assert torch.equal(new_xyz, new_xyz2) and torch.equal(out, out2)


# ---- errors: raised on the host, with the operand named, before any launch --------------------------------------------------------------------------
def test_errors_name_the_operand(K, pu, dev):
    from act_amd.models import pointnet2 as P
    xyz, q = torch.zeros(1, 8, 3, device=dev), torch.zeros(1, 2, 3, device=dev)
    with pytest.raises(RuntimeError, match="new_xyz"):
        K.ball_query(xyz, q.cpu(), 0.5, 4)
    with pytest.raises(RuntimeError, match="xyz.*float32"):
        K.ball_query(xyz.double(), q, 0.5, 4)
    with pytest.raises(RuntimeError, match="nsample"):
        K.ball_query(xyz, q, 0.5, 0)
    with pytest.raises(RuntimeError, match="nsample"):
        pu.ball_query(0.5, 0, xyz, q)
    with pytest.raises(RuntimeError, match="new_xyz"):
        K.ball_query(xyz, torch.zeros(2, 2, 3, device=dev), 0.5, 4)
    idx = torch.zeros(1, 2, 4, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="feat"):
        K.group_rows(xyz, q, torch.zeros(1, 8, 5), idx)
    with pytest.raises(RuntimeError, match="idx"):
        K.group_rows(xyz, q, None, idx.float())
    with pytest.raises(RuntimeError, match="features"):
        pu.grouping_operation(torch.zeros(1, 5, 8, device=dev).half(), idx)
    sa = P.PointNetSetAbstraction(2, 0.5, 4, 3 + 5, [8], False).to(dev)
    with pytest.raises(RuntimeError, match="in_channel"):
        sa(xyz.transpose(1, 2), torch.zeros(1, 4, 8, device=dev))
    with pytest.raises(RuntimeError, match="in_channel"):
        sa(xyz.transpose(1, 2), None)
    with pytest.raises(RuntimeError, match="points"):
        sa(xyz.transpose(1, 2), torch.zeros(1, 5, 8))
    with pytest.raises(RuntimeError, match="xyz"):
        sa(xyz.transpose(1, 2).double(), torch.zeros(1, 5, 8, device=dev))
