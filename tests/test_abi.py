"""CPU: the C-ABI library builds/loads, exports every symbol include/vallex_hip.h and include/vallex_hip_dev.h declare, and the product path
fails loudly (no CPU fallback, no oracle import) when there is no GPU."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import vallex_amd
    return vallex_amd.load_library()


def test_header_symbols_exported(lib):
    from vallex_amd._capi import DEV_SYMBOLS, SYMBOLS
    for header, syms in (("vallex_hip.h", SYMBOLS), ("vallex_hip_dev.h", DEV_SYMBOLS)):
        hdr = open(os.path.join(ROOT, "include", header)).read()
        hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
        declared = set(re.findall(r"\b(vx_[a-z_]+)\s*\(", hdr))
        assert declared == set(syms), header
        for s in declared:
            assert hasattr(lib, s), s
    # the drop-in boundary carries no measurement entry
    assert not [s for s in SYMBOLS if s.startswith(("vx_bench", "vx_prof"))]


def test_struct_layout_matches_header():
    import ctypes as C
    from vallex_amd._capi import vx_batch, vx_config, vx_sampling
    # every descriptor starts with struct_size (ABI guard, include/vallex_hip.h)
    assert vx_config.struct_size.offset == vx_batch.struct_size.offset == vx_sampling.struct_size.offset == 0
    assert vx_config.cu_mask.offset == 10 * 4 and vx_config.arith.offset == 18 * 4 and C.sizeof(vx_config) == 19 * 4
    assert vx_batch.text_ids.offset == 8 and vx_batch.text_lens.offset == 32 and C.sizeof(vx_batch) == 64
    assert vx_sampling.uniforms.offset == 16 and vx_sampling.seed.offset == 32 and vx_sampling.best_of.offset == 48
    assert C.sizeof(vx_sampling) == 64


def test_header_struct_fields_match_binding():
    """field names and order of the three descriptor structs in include/vallex_hip.h == the ctypes binding"""
    from vallex_amd._capi import vx_batch, vx_config, vx_sampling
    hdr = open(os.path.join(ROOT, "include", "vallex_hip.h")).read()
    for st in (vx_config, vx_batch, vx_sampling):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (st.__name__, st.__name__), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*;", body)
        assert names == [f[0] for f in st._fields_], (st.__name__, names)


def test_abi_version_and_struct_size_guard(lib):
    """a caller compiled against an older / shorter struct is rejected with VX_EINVAL instead of being read past its end"""
    import ctypes as C
    from vallex_amd._capi import ABI_VERSION, VX_EINVAL, vx_config
    hdr = open(os.path.join(ROOT, "include", "vallex_hip.h")).read()
    assert int(re.search(r"#define VX_ABI_VERSION (\d+)", hdr).group(1)) == ABI_VERSION == lib.vx_abi_version()
    ctx = C.c_void_p()
    short = vx_config(C.sizeof(vx_config) - 4, 2, 1, 8, 8, 8, 1, 0, 0, 0)          # e.g. the ABI-3 struct without `arith`
    assert lib.vx_create(0, C.byref(short), C.byref(ctx)) == VX_EINVAL
    assert b"struct_size" in lib.vx_last_error(None)


def test_integration_md_stub_matches_binding():
    """the ctypes structs a maintainer would paste from INTEGRATION.md have the binding's exact layout"""
    import ctypes as C
    from vallex_amd import _capi
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = max(re.findall(r"```python\n(.*?)```", md, re.S), key=len)
    classes = re.findall(r"(class vx_\w+\(C\.Structure\):.*?)(?=\nclass |\n\ndef |\ndef )", block, re.S)
    assert len(classes) == 3, len(classes)
    ns = {"C": C}
    exec("\n".join(classes), ns)
    for name in ("vx_config", "vx_batch", "vx_sampling"):
        mine, theirs = getattr(_capi, name), ns[name]
        assert C.sizeof(mine) == C.sizeof(theirs), name
        assert [(f[0], getattr(mine, f[0]).offset) for f in mine._fields_] == \
               [(f[0], getattr(theirs, f[0]).offset) for f in theirs._fields_], name


def test_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import vallex_amd
    with pytest.raises(vallex_amd.VallexHipError):
        vallex_amd.Engine(num_layers=2)


def test_product_never_imports_oracle():
    code = ("import sys, vallex_amd\nfrom vallex_amd.utils import generation\nfrom vallex_amd.models import vallex\n"
            "assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules), 'oracle imported'\n")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
    for dp, _, fs in os.walk(os.path.join(ROOT, "vall-e-x_amd")):
        for f in fs:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f


def test_library_sources_never_abort_the_host_process():
    """a C-ABI library reports VX_E* and a message; it must not contain abort() / exit() / assert() in host code paths (round 3
    had five abort() calls in launchers: a split count that was not compiled in killed the caller)"""
    import glob
    bad = []
    for f in glob.glob(os.path.join(ROOT, "vall-e-x_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "vall-e-x_amd", "csrc", "*.h")):
        src = re.sub(r"//.*", "", open(f).read())
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        for m in re.finditer(r"(?<![A-Za-z_])(abort|exit|_Exit|quick_exit|assert)\s*\(", src):
            if m.group(1) == "assert" and "static_assert" in src[max(0, m.start() - 7):m.end()]:
                continue
            bad.append((os.path.basename(f), m.group(0)))
    assert not bad, bad


def test_dev_dec_attn_prototype_matches_binding(lib):
    """the header's prototype of vx_dev_dec_attn and the ctypes signature agree argument by argument (17 of them)"""
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "vallex_hip_dev.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"\bint vx_dev_dec_attn\((.*?)\);", hdr, re.S).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["vx_ctx* ctx", "int32_t nrows", "int32_t Tmax", "int32_t qkv_balanced", "int32_t skp", "const int32_t* ctx_len",
                    "const int32_t* active", "const int32_t* slot_order", "float* kc", "float* vc", "const float* qkv", "const float* x_in",
                    "const float* resid", "float* out", "float* xp_att", "float* part_ml", "int32_t* geom"], args
    kinds = {"vx_ctx*": C.c_void_p, "int32_t": C.c_int32, "const int32_t*": C.POINTER(C.c_int32), "int32_t*": C.POINTER(C.c_int32),
             "float*": C.POINTER(C.c_float), "const float*": C.POINTER(C.c_float)}
    want = [kinds[a.rsplit(" ", 1)[0]] for a in args]
    assert lib.vx_dev_dec_attn.restype is C.c_int and len(lib.vx_dev_dec_attn.argtypes) == 17
    assert list(lib.vx_dev_dec_attn.argtypes) == want


def test_dev_dec_op_prototype_matches_binding(lib):
    """the header's prototype of vx_dev_dec_op and the ctypes signature agree argument by argument (13 of them), and the op / weight
    codes of the header are the binding's"""
    import ctypes as C
    from vallex_amd._capi import DEV_OPS, DEV_WEIGHTS
    raw = open(os.path.join(ROOT, "include", "vallex_hip_dev.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    proto = re.search(r"\bint vx_dev_dec_op\((.*?)\);", hdr, re.S).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["vx_ctx* ctx", "int32_t op", "int32_t variant", "int32_t layer", "int32_t nrows", "const int32_t* tok", "const int32_t* pos",
                    "const float* x", "const float* slabs", "float* resid", "float* out", "float* h", "float* xp"], args
    kinds = {"vx_ctx*": C.c_void_p, "int32_t": C.c_int32, "const int32_t*": C.POINTER(C.c_int32), "float*": C.POINTER(C.c_float),
             "const float*": C.POINTER(C.c_float)}
    want = [kinds[a.rsplit(" ", 1)[0]] for a in args]
    assert lib.vx_dev_dec_op.restype is C.c_int and len(lib.vx_dev_dec_op.argtypes) == 13
    assert list(lib.vx_dev_dec_op.argtypes) == want
    ops = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VX_DEV_OP_(\w+) (\d+)", hdr)}
    assert ops == DEV_OPS
    wts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VX_DEV_W_(\w+) (\d+)", hdr)}
    assert wts == {"IN": DEV_WEIGHTS["in_proj"], "OUT": DEV_WEIGHTS["out_proj"], "L2": DEV_WEIGHTS["linear2"], "PRED": DEV_WEIGHTS["predict"]}


def _proto_matches(lib, name, want_args):
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "vallex_hip_dev.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"\bint %s\((.*?)\);" % name, hdr, re.S).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == want_args, args
    kinds = {"vx_ctx*": C.c_void_p, "int32_t": C.c_int32, "const int32_t*": C.POINTER(C.c_int32), "int32_t*": C.POINTER(C.c_int32),
             "float*": C.POINTER(C.c_float), "const float*": C.POINTER(C.c_float), "uint16_t*": C.POINTER(C.c_uint16),
             "int64_t*": C.POINTER(C.c_int64)}
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == [kinds[a.rsplit(" ", 1)[0]] for a in args]
    return hdr


def test_dev_gemm_prototype_matches_binding(lib):
    """the header's prototype of vx_dev_gemm and the ctypes signature agree argument by argument (26 of them); flags and sentinels too"""
    from vallex_amd import _capi
    hdr = _proto_matches(lib, "vx_dev_gemm", [
        "vx_ctx* ctx", "int32_t kernel", "int32_t flags", "int32_t M", "int32_t N", "int32_t K", "const float* A", "int32_t rowsA", "int32_t lda",
        "const int32_t* gather", "const float* W", "int32_t w_src", "int32_t w_layer", "int32_t w_shift", "const float* bias", "const float* resid",
        "int32_t rowsR", "int32_t ldr", "const int32_t* resid_rows", "const float* colscale", "int32_t act", "float* C", "int32_t rowsC",
        "uint16_t* planes", "uint16_t* a_planes", "int32_t* info"])
    assert len(lib.vx_dev_gemm.argtypes) == 26
    assert int(re.search(r"#define VX_DEV_GEMM_OUT_PLANES (\d+)", hdr).group(1)) == _capi.DEV_GEMM_OUT_PLANES
    assert int(re.search(r"#define VX_DEV_GEMM_INPLACE (\d+)", hdr).group(1)) == _capi.DEV_GEMM_INPLACE
    assert int(re.search(r"#define VX_DEV_SENTINEL_H (0x[0-9A-Fa-f]+)", hdr).group(1), 16) == _capi.DEV_SENTINEL_H
    assert sorted(_capi.DEV_GEMM_KERNELS.values()) == [0, 1, 2, 3, 4, 10, 11, 12, 13, 14, 15, 20, 21]
    assert sorted(_capi.DEV_GEMM_WSRC.values()) == list(range(1, 9))


def test_dev_layernorm_prototype_matches_binding(lib):
    """the header's prototype of vx_dev_layernorm and the ctypes signature agree argument by argument (13 of them)"""
    _proto_matches(lib, "vx_dev_layernorm", [
        "vx_ctx* ctx", "int32_t rows", "int32_t C", "int32_t ldx", "const float* x", "const float* g", "const float* b", "const float* ada_w",
        "const float* ada_b", "float* y", "int32_t rowsY", "uint16_t* planes", "int32_t* range_flag"])
    assert len(lib.vx_dev_layernorm.argtypes) == 13


def test_dev_wave_op_prototype_matches_binding(lib):
    """the header's prototype of vx_dev_wave_op and the ctypes signature agree argument by argument (14 of them); the op codes and the
    64-bit sentinel of the code buffer are the binding's"""
    from vallex_amd import _capi
    hdr = _proto_matches(lib, "vx_dev_wave_op", [
        "vx_ctx* ctx", "int32_t op", "const int32_t* dims", "const float* a", "const float* b", "const float* w", "const float* bias",
        "const int32_t* ia", "const int32_t* ib", "float* out", "float* out2", "float* out3", "int64_t* codes", "int32_t* geom"])
    assert len(lib.vx_dev_wave_op.argtypes) == 14
    ops = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VX_DEV_WAVE_(\w+) (\d+)", hdr)}
    assert ops == _capi.DEV_WAVE_OPS and sorted(ops.values()) == list(range(12))
    assert int(re.search(r"#define VX_DEV_SENTINEL_L \((-\d+)LL\)", hdr).group(1)) == _capi.DEV_SENTINEL_L
    assert "vx_dev_wave_op" in _capi.DEV_SYMBOLS


def test_dev_seam_op_prototype_matches_binding(lib):
    """the header's prototype of vx_dev_seam_op and the ctypes signature agree argument by argument (15 of them); the op codes, the
    word offsets of the state block and the int sentinel are the binding's"""
    from vallex_amd import _capi
    hdr = _proto_matches(lib, "vx_dev_seam_op", [
        "vx_ctx* ctx", "int32_t op", "const int32_t* dims", "const float* fa", "const float* fb", "const float* fc", "const float* fd",
        "const int32_t* ia", "const int32_t* ib", "const int32_t* ic", "const int32_t* id", "float* out", "float* out2", "float* out3",
        "int32_t* iout"])
    assert len(lib.vx_dev_seam_op.argtypes) == 15
    st = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VX_DEV_SEAM_ST_(\w+) (\d+)", hdr)}
    assert st == _capi.DEV_SEAM_STATE
    ops = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VX_DEV_SEAM_(?!ST_)(\w+) (\d+)", hdr)}
    assert ops == _capi.DEV_SEAM_OPS and sorted(ops.values()) == list(range(15))
    assert int(re.search(r"#define VX_DEV_SENTINEL_I \((-\d+)\)", hdr).group(1)) == _capi.DEV_SENTINEL_I
    assert "vx_dev_seam_op" in _capi.DEV_SYMBOLS
