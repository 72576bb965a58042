"""CPU: the host side of GEMM tuning.  kernels.gemm_candidates, the pure enumeration behind gemm_tune, lists exactly what the enumeration it was
factored out of listed; kernels.gemm_config takes one decision for the per-kernel and the composite path.

tests/golden/gemm_candidates.json was written from the in-line enumeration of gemm_tune as it stood before the split (the loop in front of
`if given is not None`), over the grid of _cases() below: one sha256 over every list of the grid, in order, plus the lists of every
_EVERY-th case in full so that a mismatch can be looked at.  Order matters: a tie in the timing goes to the first candidate.
"""
import hashlib
import itertools
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_candidates.json")
_EVERY = 97


def _cases():
    """(ak, bk, M, N, K, workspace bytes, max_split): all four layouts x M, N x K, then every shape of the shipped tune table; each with the
    product's workspace and a small one (so the partial-sums bound bites) and with split-K uncapped and capped at 4"""
    dims = (48, 64, 128, 384, 1024, 8192)
    shapes = [(ak, bk, M, N, K) for ak, bk in itertools.product((0, 1), repeat=2) for M in dims for N in dims
              for K in (96, 256, 1024, 1536, 8192, 65536, 262144)]
    with open(os.path.join(ROOT, "act_amd", "gemm_tune_gfx950.json")) as f:
        shapes += sorted(tuple(int(v) for v in k.split(",")) for k in json.load(f)["configs"])
    return [s + (ws, ms) for s in shapes for ws in (160 << 20, 16 << 20) for ms in (0, 4)]


def _line(case, cands):
    return ",".join(map(str, case)) + ":" + ";".join("%d,%d" % tuple(c) for c in cands) + "\n"


def digest(enum):
    """enum(ak, bk, M, N, K, ws_bytes, max_split) -> list of (tile, splits)  =>  the fixture's content"""
    h, sample, total = hashlib.sha256(), {}, 0
    cases = _cases()
    for i, case in enumerate(cases):
        line = _line(case, enum(*case))
        h.update(line.encode())
        total += line.count(",") - 6
        if i % _EVERY == 0:
            sample[str(i)] = line.strip()
    return {"cases": len(cases), "candidates": total, "sha256": h.hexdigest(), "sample": sample}


def test_gemm_candidates_equal_the_recorded_enumeration():
    import act_amd.kernels as K
    with open(GOLDEN) as f:
        want = json.load(f)
    got = digest(lambda ak, bk, M, N, Kd, ws, ms: K.gemm_candidates(bool(ak), bool(bk), M, N, Kd, ws, ms))
    assert want["cases"] == got["cases"] >= 4 * 4 * 36 * 7 and want["candidates"] > 10 * want["cases"]
    bad = [(i, got["sample"][i], want["sample"][i]) for i in want["sample"] if got["sample"][i] != want["sample"][i]]
    assert not bad, bad[:3]
    assert got["candidates"] == want["candidates"] and got["sha256"] == want["sha256"]


def test_gemm_candidates_need_no_tensor_and_feed_gemm_tune():
    """a function of integers only (it runs here, without a device), and the enumeration gemm_tune times"""
    import inspect
    import act_amd.kernels as K
    assert list(inspect.signature(K.gemm_candidates).parameters) == ["ak", "bk", "M", "N", "K", "ws_bytes", "max_split"]
    c = K.gemm_candidates(True, False, 1024, 384, 1536, 160 << 20, 0)
    assert c[0] == (1, 1) and all(isinstance(t, int) and isinstance(s, int) and s >= 1 for t, s in c)
    assert "gemm_candidates(ak, bk, M, N, K, ws.numel() * 4, _MAX_SPLIT)" in inspect.getsource(K.gemm_tune)


def test_gemm_config_is_one_decision_for_both_host_paths(monkeypatch):
    """kernels.gemm_config on the host alone (the timing, the capture query and the operands are stand-ins; the C-side table is host memory):
    what gemm() gets through _gemm_config and what composite.ensure_tuned gets through _tune_shape, case by case"""
    import ctypes
    import types
    import torch
    import act_amd.kernels as K
    import act_amd.composite as CP
    dev, timed, capturing = types.SimpleNamespace(index=0), [], [False]
    monkeypatch.setattr(K, "first_use_config", lambda a, b, ak, bk, M, N, Kd, ws: (timed.append((tuple(a.shape), tuple(b.shape), ws)), (31, 2))[1])
    monkeypatch.setattr(K, "workspace", lambda device, *a, **k: "current stream's")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: capturing[0])
    monkeypatch.setattr(torch, "randn", lambda shape, dtype=None, device=None: torch.empty(shape, device="meta"))
    monkeypatch.setattr(K, "_GEMM_CACHE", {})
    monkeypatch.setattr(K, "_NEW_TUNED", {})

    def c_side(*key):
        t, s = ctypes.c_int(), ctypes.c_int()
        return (t.value, s.value) if K.lib.act_gemm_tune_get(*key, ctypes.byref(t), ctypes.byref(s)) == 0 else None

    def operand(*shape):
        return types.SimpleNamespace(shape=shape, device=dev)

    nt, nn = (1, 1, 1000, 512, 4096), (1, 0, 1000, 512, 4096)
    assert nt not in K._GEMM_TABLE and nn not in K._GEMM_TABLE
    try:
        # below the cut-off, and the skinny TN exemption: the cost model, nothing timed or recorded
        assert K.gemm_config(1, 1, 8, 8, 8, dev) == (0, 0) and K.gemm_config(0, 0, 4, 4096, 65536, dev) == (0, 0)
        # stream capture: undecided -- gemm() runs the cost model, the composite asks again later, nothing is recorded
        capturing[0] = True
        assert K.gemm_config(*nt, dev) is None and CP._tune_shape(*nt, dev) is False
        assert K._gemm_config(operand(1000, 4096), operand(512, 4096), True, True, 1000, 512, 4096, "ws") == (0, 0)
        assert not timed and not K._GEMM_CACHE and not K._NEW_TUNED and c_side(*nt) is None
        capturing[0] = False
        # shapes only: timed on operands made here, cached, recorded, published
        assert CP._tune_shape(*nt, dev) is True and timed == [((1000, 4096), (512, 4096), "current stream's")]
        assert K._GEMM_CACHE[nt + (0,)] == K._NEW_TUNED[nt] == c_side(*nt) == (31, 2)
        assert K.gemm_config(*nt, dev) == (31, 2) and len(timed) == 1
        # the C-side table cleared: gemm() keeps its cached decision without crossing the FFI, the composite path publishes it again
        CP.reset_tuning()
        assert c_side(*nt) is None and K.gemm_config(*nt, dev) == (31, 2) and c_side(*nt) is None
        assert CP._tune_shape(*nt, dev) is True and c_side(*nt) == (31, 2) and len(timed) == 1
        # operands given: timed on them with the caller's workspace, published for the composites
        assert K._gemm_config(operand(1000, 4096), operand(4096, 512), True, False, 1000, 512, 4096, "caller's") == (31, 2)
        assert timed[1] == ((1000, 4096), (4096, 512), "caller's") and c_side(*nn) == K._NEW_TUNED[nn] == (31, 2)
        # a shape of the shipped table: cached, never timed, no gap reported
        listed = next(k for k in K._GEMM_TABLE if k[2] * k[3] * k[4] >= 1 << 24 and (k[0] or k[1] or min(k[2], k[3]) > 8))
        assert K.gemm_config(*listed, dev) == K._GEMM_TABLE[listed] == K._GEMM_CACHE[listed + (0,)] == c_side(*listed)
        assert len(timed) == 2 and listed not in K._NEW_TUNED
        # a configuration already in the C-side table is left as it is
        K.lib.act_gemm_tune_set(1, 1, 2000, 512, 4096, 11, 1)
        assert CP._tune_shape(1, 1, 2000, 512, 4096, dev) is True and c_side(1, 1, 2000, 512, 4096) == (11, 1) and len(timed) == 2
    finally:
        CP.reset_tuning()                                       # the C-side table back to the shipped entries


# the tile table of csrc/gemm.hip, written out: id -> (BM, BN, layouts as bits 2 * a_kmajor + b_kmajor); 15 = all four, 8 = NT, 4 = NN, 5 = NN and TN
_TILES = {1: (128, 128, 15), 2: (128, 64, 15), 3: (64, 64, 15), 4: (128, 128, 15), 5: (128, 64, 15), 6: (64, 64, 15),
          7: (128, 128, 15), 8: (128, 64, 15), 9: (64, 64, 15), 10: (128, 128, 8), 11: (128, 64, 8), 12: (64, 64, 8),
          13: (128, 128, 5), 14: (64, 128, 4), 15: (64, 64, 4), 16: (128, 64, 4), 17: (128, 128, 8), 18: (128, 64, 8),
          20: (128, 128, 8), 21: (128, 64, 8), 30: (128, 128, 8), 31: (128, 64, 8), 32: (64, 64, 8),
          33: (128, 128, 5), 34: (64, 128, 4), 35: (64, 64, 4), 36: (128, 64, 4)}
# need: 0 any shape, 1 full or M tail, 2 full only; + 4: the 32-bit in-tile offset bound of the hand-scheduled loops
_NEED = {**{t: 0 for t in range(1, 7)}, **{t: 1 for t in range(7, 17)}, **{t: 2 for t in (17, 18, 20, 21)}, **{t: 5 for t in range(30, 37)}}


def _tile_info(lib, tile):
    import ctypes
    v = [ctypes.c_int(-9) for _ in range(4)]
    rc = lib.act_gemm_tile_info(tile, *[ctypes.byref(x) for x in v])
    assert rc in (0, 1)
    return tuple(x.value for x in v) if rc == 0 else None


def test_tile_info_is_the_table_and_nothing_else():
    import act_amd.kernels as K
    got = {t: _tile_info(K.lib, t) for t in range(-4, 130)}
    assert {t for t, v in got.items() if v is not None} == set(_TILES) == set(range(1, 19)) | {20, 21} | set(range(30, 37))
    assert {t: got[t][:3] for t in _TILES} == _TILES and {t: got[t][3] for t in _TILES} == _NEED
    assert K.lib.act_gemm_tile_info(13, None, None, None, None) == 0                  # every out-pointer is optional
    try:
        for t in (-1, 19, 22, 29, 37, 64):
            assert got[t] is None and K.lib.act_gemm_tune_set(1, 1, 1000, 512, 4096, t, 1) == -1      # ACT_E_BADARG
        assert K.lib.act_gemm_tune_get(1, 1, 1000, 512, 4096, None, None) == 1         # nothing was stored
        for t in [0] + sorted(_TILES):
            assert K.lib.act_gemm_tune_set(1, 1, 1000, 512, 4096, t, 1) == 0
    finally:
        import act_amd.composite as CP
        CP.reset_tuning()


def test_every_proposed_candidate_is_admitted_for_its_layout():
    import act_amd.kernels as K
    layouts = {t: _tile_info(K.lib, t)[2] for t in _TILES}
    seen = set()
    for ak, bk, M, N, Kd, ws, ms in _cases():
        for t, _ in K.gemm_candidates(bool(ak), bool(bk), M, N, Kd, ws, ms):
            seen.add(t)
            assert t in layouts and layouts[t] & (1 << (2 * ak + bk)), (t, ak, bk, M, N, Kd)
    assert seen
