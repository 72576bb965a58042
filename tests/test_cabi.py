"""CPU: the C-ABI library loads and exports every symbol include/act_hip.h declares, and the ctypes binding (act_amd/_abi.py, applied once by
act_amd/_C.py) agrees with the header prototype by prototype and struct by struct (no compute calls)."""
import os
import re
import ctypes
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    src = open(os.path.join(ROOT, "include", "act_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(act_[a-z0-9_]+)\s*\(", _header())))


# ---- a small parser of the header: prototypes and typedef'd structs (regex over the comment-stripped text, no C compiler) ----------------
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "long long": ctypes.c_longlong, "uint64_t": ctypes.c_uint64, "unsigned": ctypes.c_uint}
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}


def _is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def _matches(ctype_text, t):
    """does the ctypes type t have the kind of the C type?  pointer: anything with * or act_stream_t; else one of _SCALARS (ctypes aliases
    types of equal size and signedness -- size_t and uint64_t here -- so identity is the comparison)"""
    if "*" in ctype_text or "act_stream_t" in ctype_text:
        return _is_pointer(t)
    return t is _SCALARS[" ".join(ctype_text.replace("const", " ").split())]      # KeyError: a C type this test has not been taught


def _prototypes():
    """name -> (return type, [parameter type, ...]) as C text"""
    out = {}
    for ret, name, params in re.findall(r"^\s*(int|size_t|const char\s*\*)\s+(act_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header(), flags=re.M):
        params = [] if params.strip() == "void" else [re.sub(r"\s*\b\w+\s*$", "", q.strip()) for q in params.split(",")]
        assert name not in out and all(params), (name, params)
        out[name] = (ret.replace(" ", "").replace("constchar", "const char"), params)
    return out


def _structs():
    """typedef name -> [(field name, C type text with a * per pointer level of the declarator, array length or 0), ...]; splits multi-declarator
    lines (`const float *a, *b;`, `int ldr, ldaux;`) and arrays (`const float* stacked[4];`)"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(act_[a-z0-9_]+_t)\s*;", _header(), flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *rest = decl.split(",")
            m = re.match(r"^(.*?)((?:\*\s*)*)(\w+)\s*(?:\[(\d+)\])?$", first.strip(), flags=re.S)
            base = m.group(1).strip()
            fields.append((m.group(3), base + m.group(2).strip(), int(m.group(4) or 0)))
            for r in rest:
                m = re.match(r"^((?:\*\s*)*)(\w+)\s*(?:\[(\d+)\])?$", r.strip())
                fields.append((m.group(2), base.rstrip("* ") + m.group(1).strip(), int(m.group(3) or 0)))
        out[name] = fields
    return out


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "act_amd", "lib", "libact_hip.so"))
    names = _declared()
    assert len(names) >= 10
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    lib.act_arch.restype = ctypes.c_char_p
    assert lib.act_arch() == b"gfx950" and lib.act_version() >= 100


def test_binding_declares_every_symbol():
    # act_amd._C alone covers the header (a fresh interpreter: this process may have imported the other modules already) ...
    code = ("import sys, act_amd._C as C; assert 'act_amd.kernels' not in sys.modules and 'act_amd.composite' not in sys.modules; "
            "print('\\n'.join(sorted(C.SIGNATURES)))")
    alone = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout.split()
    assert alone == _declared()
    # ... and importing the modules that call it declares nothing more and re-declares nothing
    import act_amd._C as C
    import act_amd.kernels  # noqa: F401
    import act_amd.composite  # noqa: F401
    assert set(_declared()) <= set(C.SIGNATURES), sorted(set(_declared()) - set(C.SIGNATURES))
    assert sorted(C.SIGNATURES) == _declared()
    for name, (restype, argtypes) in C.SIGNATURES.items():
        fn = getattr(C.lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_binding_agrees_with_every_prototype_of_the_header():
    """return type and, in order, the kind of every parameter of every function: a size_t declared as int truncates a workspace size, a
    long long declared as int a row count"""
    import act_amd._C as C
    protos = _prototypes()
    assert sorted(protos) == _declared() == sorted(C.SIGNATURES) and len(protos) > 100
    bad = []
    for name, (ret, params) in protos.items():
        restype, argtypes = C.SIGNATURES[name]
        if restype is not _RETURNS[ret]:
            bad.append((name, "returns " + ret, restype.__name__))
        if len(argtypes) != len(params):
            bad.append((name, "%d parameters" % len(params), len(argtypes)))
        bad += [(name, "parameter %d: %s" % (i, q), t.__name__) for i, (q, t) in enumerate(zip(params, argtypes)) if not _matches(q, t)]
    assert not bad, bad


def test_struct_mirrors_agree_with_the_header():
    """field names in the header's order, and the kind of every field, for every typedef'd struct of the header"""
    from act_amd import _abi
    import act_amd.kernels as K
    import act_amd.composite as CP
    structs = _structs()
    assert set(structs) == set(_abi.STRUCTS) and len(structs) >= 12
    assert structs["act_gemm_epilogue_t"][4:6] == [("ldr", "int", 0), ("ldaux", "int", 0)]                    # (the parser splits declarator lists ...
    assert structs["act_gemm_fx_t"][1] == ("a_shift", "const float*", 0) and structs["act_dgcnn_t"][11] == ("stacked", "const float*", 4)     # ... and arrays)
    for name, fields in structs.items():
        mirror = _abi.STRUCTS[name]._fields_
        assert [f[0] for f in mirror] == [f[0] for f in fields], name
        for (fname, t), (_, ctext, length) in zip(mirror, fields):
            if length:
                assert issubclass(t, ctypes.Array) and t._length_ == length, (name, fname)
                t = t._type_
            assert _matches(ctext, t), (name, fname, ctext, t)
    # the names the callers build the structs by
    assert K.GemmEpilogue is _abi.GemmEpilogue and K.GemmTnProblem is _abi.GemmTnProblem
    for n in ("BlockParams", "BlockDims", "BlockStack", "PrefixVit", "VitBf16x3", "PointnetParams", "PointnetGrads", "PointnetDims", "Dgcnn", "GemmFx"):
        assert getattr(CP, n) is getattr(_abi, n), n


def test_ops_refuse_cpu_tensors():
    import pytest
    import torch
    import act_amd._C as C
    from act_amd.pointnet2_ops import pointnet2_utils as pu
    from act_amd.knn_cuda import KNN
    with pytest.raises(RuntimeError):
        pu.furthest_point_sample(torch.zeros(1, 16, 3), 4)
    with pytest.raises(RuntimeError):
        KNN(4, True)(torch.zeros(1, 16, 3), torch.zeros(1, 2, 3))
    with pytest.raises(C.ActHipError):
        C.ptr(torch.zeros(3))


def test_generated_asm_loops_header_is_current():
    """act_amd/csrc/gemm_nt_asm_loop.h (the hand-scheduled K loops, ~12k lines of inline assembly) is GENERATED by csrc/gen_nt_asm.py and committed:
    the committed header must be exactly what the committed generator emits, and every loop must keep its register / LDS budget (VGPRs <= 256 so two
    workgroups share a CU, LDS offsets within the 16-bit ds immediates)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "act_amd", "csrc", "gen_nt_asm.py")
    spec = importlib.util.spec_from_file_location("gen_nt_asm", path)
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    with open(os.path.join(root, "act_amd", "csrc", "gemm_nt_asm_loop.h")) as f:
        assert f.read() == gen.render(), "run python act_amd/csrc/gen_nt_asm.py"
    names = set()
    for c in gen.VARIANTS:
        assert c.total <= 256 and 2 * c.STAGE + (8192 if c.affine else 0) <= 80 * 1024, (c.name(), c.total, c.STAGE)
        assert 2 * c.STAGE <= 65536                                   # every ds offset fits the 16-bit immediate
        assert c.name() not in names
        names.add(c.name())
    assert {"nt_asm_loop_4x4", "nt_asm_loop_4x2", "nt_asm_loop_2x2", "nn_asm_loop_4x4", "tn_asm_loop_4x4", "tn_asm_loop_4x4_asum"} <= names
