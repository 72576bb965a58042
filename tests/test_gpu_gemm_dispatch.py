"""GPU: a fingerprint of the GEMM dispatcher (act_sgemm_ex_f32: tile id + layout + shape -> return code and kernel).

tests/golden/gemm_dispatch.json was recorded with `python -m tests.test_gpu_gemm_dispatch --record` from the commit BEFORE the tile table
replaced the id arithmetic in csrc/gemm.hip (that commit plus this file alone), so equality with it says: every known tile id, in every
layout, still refuses what it refused and still writes the bits it wrote.  Per (id, layout) the fixture holds the return codes of _CASES
in order and one sha256 over the case lines `name:rc:sha256(C bytes)[:sha256(aux bytes)]`.

The case list is literal (it does not ask the library which ids exist): the smallest shapes at which each rule of the dispatcher can flip.
Every product is far below the autotuner's cut-off and goes to the C entry directly, so nothing is timed."""
import ctypes
import hashlib
import itertools
import json
import os

import pytest
import torch

from tests.golden.fill import fill_tensor

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_dispatch.json")

IDS = [0] + list(range(1, 19)) + [20, 21] + list(range(30, 37))             # 0 = the cost model; the others name a kernel
UNKNOWN = (-1, 19, 22, 29, 37, 64)
LAYOUTS = list(itertools.product((0, 1), repeat=2))                        # (a_kmajor, b_kmajor)
_WS_BYTES = 4 << 20                                                        # fixed: the cost model of id 0 looks at it
_SENTINEL = -7.5

# (name, M, N, K, operand A variant, splits, workspace?, activation or None)
_CASES = [
    ("full", 256, 256, 64, "plain", 1, True, None),
    ("mtail", 200, 256, 64, "plain", 1, True, None),
    ("n192", 256, 192, 64, "plain", 1, True, None),
    ("k80", 256, 256, 80, "plain", 1, True, None),
    ("ragged", 130, 70, 33, "plain", 1, True, None),
    ("unaligned", 256, 256, 64, "shift1", 1, True, None),
    ("padded", 256, 256, 64, "pad4", 1, True, None),
    ("split2", 256, 256, 2048, "plain", 2, True, None),
    ("split3", 256, 256, 2048, "plain", 3, True, None),
    ("split2_nows", 256, 256, 2048, "plain", 2, False, None),
] + [("%s_act%d" % (name, act), M, 256, 64, "plain", 1, True, act) for name, M in (("full", 256), ("mtail", 200)) for act in range(5)]


class _Inputs:
    """operands by (shape, layout), made once and shared by every id"""

    def __init__(self):
        self.cache = {}

    def get(self, name, *shape):
        key = (name,) + shape
        if key not in self.cache:
            self.cache[key] = fill_tensor("dispatch.%s.%s" % (name, "x".join(map(str, shape))), shape, "code").cuda()
        return self.cache[key]

    def operand_a(self, rows, cols, variant):
        """-> (tensor that owns the memory, device pointer, leading dimension)"""
        key = ("A", rows, cols, variant)
        if key not in self.cache:
            a = self.get("a", rows, cols)
            if variant == "shift1":                                        # starts one float into its allocation
                buf = torch.zeros(rows * cols + 4, device="cuda")
                buf[1:1 + rows * cols] = a.reshape(-1)
                self.cache[key] = (buf, buf.data_ptr() + 4, cols)
            elif variant == "pad4":                                        # leading dimension = row length + 4
                buf = torch.zeros(rows, cols + 4, device="cuda")
                buf[:, :cols] = a
                self.cache[key] = (buf, buf.data_ptr(), cols + 4)
            else:
                self.cache[key] = (a, a.data_ptr(), cols)
        return self.cache[key]


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _run_case(lib, stream, inp, ws, tile, ak, bk, case):
    name, M, N, Kd, variant, splits, with_ws, act = case
    _, a_ptr, lda = inp.operand_a(*((M, Kd) if ak else (Kd, M)), variant)
    b = inp.get("b", *((N, Kd) if bk else (Kd, N)))
    c = torch.full((M, N), _SENTINEL, device="cuda")
    epi, aux = None, None
    if act is not None:
        from act_amd._abi import GemmEpilogue
        bias, res = inp.get("bias", N), inp.get("res", M, N)
        aux = inp.get("aux", M, N).clone() if act in (3, 4) else torch.full((M, N), _SENTINEL, device="cuda")   # gelu' / relu mask read it
        epi = ctypes.byref(GemmEpilogue(alpha=1.0, act=act, accumulate=0, rows_per_scale=0, ldr=N, ldaux=N, res_row_div=0,
                                        bias=bias.data_ptr(), rowscale=None, res=res.data_ptr(), aux=aux.data_ptr()))
    rc = lib.act_sgemm_ex_f32(ak, bk, M, N, Kd, a_ptr, lda, b.data_ptr(), b.stride(0), c.data_ptr(), N, epi,
                              ws.data_ptr() if with_ws else None, _WS_BYTES if with_ws else 0, tile, splits, stream())
    torch.cuda.synchronize()
    line = "%s:%d:%s" % (name, rc, _sha(c)) + (":" + _sha(aux) if aux is not None else "")
    return rc, line


def fingerprint():
    """{"id,ak,bk": {"rc": [...], "sha256": ...}} over IDS x LAYOUTS x _CASES"""
    import act_amd.kernels as K
    inp, ws, out = _Inputs(), torch.empty(_WS_BYTES // 4, device="cuda"), {}
    for tile in IDS:
        for ak, bk in LAYOUTS:
            h, rcs = hashlib.sha256(), []
            for case in _CASES:
                rc, line = _run_case(K.lib, K.stream, inp, ws, tile, ak, bk, case)
                rcs.append(rc)
                h.update((line + "\n").encode())
            out["%d,%d,%d" % (tile, ak, bk)] = {"rc": rcs, "sha256": h.hexdigest()}
    return out


def test_every_known_tile_id_dispatches_as_recorded():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = fingerprint()
    assert len(want) == len(IDS) * len(LAYOUTS) == 28 * 4
    assert got == want, sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))


def test_an_id_that_names_no_kernel_is_refused():
    import act_amd.kernels as K
    inp, ws = _Inputs(), torch.empty(_WS_BYTES // 4, device="cuda")
    assert [_run_case(K.lib, K.stream, inp, ws, t, 1, 1, _CASES[0])[0] for t in UNKNOWN] == [-1] * len(UNKNOWN)      # ACT_E_BADARG


if __name__ == "__main__":
    import sys
    assert sys.argv[1:] == ["--record"], "usage: python -m tests.test_gpu_gemm_dispatch --record"
    with open(GOLDEN, "w") as f:
        json.dump(fingerprint(), f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
