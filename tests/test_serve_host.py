"""CPU: the binding side of the serving session (vx_serve_*) -- additive entry points that keep ABI version 6, the ctypes request
layout, and the argument checks that run before any GPU work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import vallex_amd  # noqa: F401  (registers the package under an importable name)
from vallex_amd._capi import ABI_VERSION, SERVE_DONE_FN, SYMBOLS, ServeSession, vx_request
from vallex_amd.models.vallex import VALLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vx_serve_open", "vx_serve_submit", "vx_serve_run", "vx_serve_close")


def _header():
    with open(os.path.join(ROOT, "include", "vallex_hip.h")) as f:
        return f.read()


def test_header_declares_the_session_and_the_binding_lists_it():
    h = _header()
    assert "typedef struct vx_serve vx_serve;" in h
    assert re.search(r"\bint vx_serve_open\(vx_ctx\* ctx, const vx_sampling\* s, vx_serve\*\* out\);", h)
    assert re.search(r"\bint vx_serve_submit\(vx_serve\* srv, const vx_batch\* rows, const vx_request\* req, int64_t\* ids_out\);", h)
    assert re.search(r"\bint vx_serve_run\(vx_serve\* srv, int32_t max_steps, vx_serve_done_fn on_done, void\* user,", h)
    assert re.search(r"\bint vx_serve_close\(vx_serve\* srv\);", h)
    assert "typedef void (*vx_serve_done_fn)(void* user, int64_t request_id, const int64_t* codes" in h
    for e in ENTRIES:
        assert e in SYMBOLS, e
    assert re.search(r"#define VX_ABI_VERSION 6\b", h) and ABI_VERSION == 6


def test_request_layout_matches_header():
    body = re.search(r"typedef struct vx_request \{(.*?)\} vx_request;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == [f[0] for f in vx_request._fields_]
    assert [(f[0], getattr(vx_request, f[0]).offset) for f in vx_request._fields_] == [
        ("struct_size", 0), ("best_of", 4), ("length_penalty", 8), ("return_worst", 12), ("seed", 16), ("uniforms", 24),
        ("uniforms_steps", 32)]
    assert C.sizeof(vx_request) == 40
    assert SERVE_DONE_FN._argtypes_ == (C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_int32)


def test_request_checks_fire_before_gpu_work():
    with pytest.raises(ValueError, match="best_of"):
        ServeSession.check_request(best_of=0)
    with pytest.raises(ValueError, match="best_of"):
        ServeSession.check_request(best_of=-2)
    with pytest.raises(ValueError, match="best_of"):
        ServeSession.check_request(best_of=6, rows=4)
    with pytest.raises(ValueError, match="uniforms"):
        ServeSession.check_request(best_of=3, uniforms=np.zeros((40, 2), np.float32))
    with pytest.raises(ValueError, match="uniforms"):
        ServeSession.check_request(best_of=3, uniforms=np.zeros(40, np.float32))
    u = ServeSession.check_request(best_of=1, uniforms=np.zeros(40))
    assert u.shape == (40, 1) and u.dtype == np.float32 and u.flags.c_contiguous
    assert ServeSession.check_request(best_of=5) is None


def test_valle_serve_refuses_session_wide_best_of_before_gpu_work():
    m = VALLE(1024, 16, 2, norm_first=True, add_prenet=False, prefix_mode=1, share_embedding=True, nar_scale_factor=1.0,
              prepend_bos=True, num_quantizers=8)
    for kw in (dict(best_of=5), dict(seed=3), dict(length_penalty=0.5), dict(return_worst=True), dict(uniforms=np.zeros(4))):
        with pytest.raises(ValueError, match="per request"):
            m.serve(**kw)
    assert m._engine is None


def test_serve_source_is_built():
    from vallex_amd import _build
    assert "serve.hip" in _build.SOURCES and "serve.hip" in _build.ENGINE_TUS
    src = open(os.path.join(ROOT, "vall-e-x_amd", "csrc", "serve.hip")).read()
    assert "__global__" in src and "serve_uniforms_kernel" in src
