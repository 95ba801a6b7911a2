"""CPU: per-request logit filters of the serving session -- the additive entry point vx_serve_submit_filtered (ABI version stays
6), the vx_request_filters layout against the ctypes binding, the bound symbols, the range checks that run before any GPU work and
the Python signatures."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import vallex_amd  # noqa: F401  (registers the package under an importable name)
from vallex_amd import _capi
from vallex_amd._capi import ABI_VERSION, DEV_SYMBOLS, SYMBOLS, ServeSession

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name="vallex_hip.h", strip_comments=False):
    with open(os.path.join(ROOT, "include", name)) as f:
        h = f.read()
    return re.sub(r"/\*.*?\*/", "", h, flags=re.S) if strip_comments else h


def test_header_declares_the_struct_and_the_entry_point():
    h = _header(strip_comments=True)
    assert "typedef struct vx_request_filters {" in h
    assert re.search(r"\bint vx_serve_submit_filtered\(vx_serve\* srv, const vx_batch\* rows, const vx_request\* req,\s*"
                     r"const vx_request_sampling\* smp\s*,\s*const vx_request_filters\* flt\s*, int64_t\* ids_out\);", h)
    assert re.search(r"#define VX_ABI_VERSION 6\b", h) and ABI_VERSION == 6
    assert "top_p" in _header()                          # the contract paragraph and the struct speak of it
    d = _header("vallex_hip_dev.h", strip_comments=True)
    assert re.search(r"\bint vx_dev_sample_filtered\(vx_ctx\* ctx, int32_t n, const int32_t\* cfg, const float\* fcfg, "
                     r"const float\* ffilt, const int32_t\* ifilt,\s*const int32_t\* hist, int32_t hist_stride, ", d)


def test_request_filters_layout_matches_header():
    st = _capi.vx_request_filters
    body = re.search(r"typedef struct vx_request_filters \{(.*?)\} vx_request_filters;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == [f[0] for f in st._fields_]
    assert re.findall(r"(u?int32_t|float)\s+\w+\s*;", body) == ["uint32_t", "float", "float", "int32_t", "int32_t"]
    assert [(f[0], getattr(st, f[0]).offset) for f in st._fields_] == [
        ("struct_size", 0), ("top_p", 4), ("repetition_penalty", 8), ("repetition_window", 12), ("min_frames", 16)]
    assert [f[1] for f in st._fields_] == [C.c_uint32, C.c_float, C.c_float, C.c_int32, C.c_int32]
    assert C.sizeof(st) == 20


def test_new_names_are_bound():
    assert "vx_serve_submit_filtered" in SYMBOLS and "vx_dev_sample_filtered" in DEV_SYMBOLS
    assert len(SYMBOLS) == len(set(SYMBOLS)) and len(DEV_SYMBOLS) == len(set(DEV_SYMBOLS))
    lib = _capi.load_library()
    assert lib.vx_serve_submit_filtered.restype is C.c_int and len(lib.vx_serve_submit_filtered.argtypes) == 6
    assert lib.vx_dev_sample_filtered.restype is C.c_int and len(lib.vx_dev_sample_filtered.argtypes) == 14
    assert callable(_capi.Engine.dev_sample_filtered)
    assert ServeSession.FILTERS == ("top_p", "repetition_penalty", "repetition_window", "min_frames")


def test_filter_checks_fire_before_gpu_work():
    for v in (0.0, -0.5, 1.0001, 2.0, float("nan"), float("inf"), 1e-50):
        with pytest.raises(ValueError, match="top_p"):
            ServeSession.check_request(top_p=v)
    for v in (0.0, -1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="repetition_penalty"):
            ServeSession.check_request(repetition_penalty=v)
    for v in (-1, 1.5, "3", True):
        with pytest.raises(ValueError, match="repetition_window"):
            ServeSession.check_request(repetition_window=v)
        with pytest.raises(ValueError, match="min_frames"):
            ServeSession.check_request(min_frames=v)
    for kw in (dict(top_p=1.0, repetition_penalty=1.0, repetition_window=0, min_frames=0),
               dict(top_p=0.05, repetition_penalty=1.3, repetition_window=np.int32(64), min_frames=np.int64(12)),
               dict(top_p=np.float32(0.9), repetition_penalty=0.8), dict(top_p=None, repetition_penalty=None, repetition_window=None,
                                                                         min_frames=None)):
        assert ServeSession.check_request(**kw) is None
    # the calls of the earlier rounds keep working, positionally too
    assert ServeSession.check_request(1, None, 4, 10, 0.7, 5) is None
    assert ServeSession.check_request(uniforms=np.zeros(8, np.float32), text_len=4, force_eos_at=7).shape == (8, 1)


def test_server_submit_signatures():
    from vallex_amd.models.vallex import Server
    from vallex_amd.utils.generation import AudioServer
    p = inspect.signature(Server.submit).parameters
    for k in ServeSession.FILTERS:
        assert p[k].default is None, k
    p = inspect.signature(AudioServer.submit).parameters
    assert [p[k].default for k in ServeSession.FILTERS] == [1.0, 1.0, 0, 0]
    assert p["top_k"].default == -100 and p["temperature"].default == 1.0
    p = inspect.signature(ServeSession.check_request).parameters
    assert list(p)[:8] == ["best_of", "uniforms", "rows", "top_k", "temperature", "force_eos_at", "text_len", "max_new"]


def test_sampler_source_carries_the_filter_record():
    src = open(os.path.join(ROOT, "vall-e-x_amd", "csrc", "serve_sample.hip")).read()
    assert "row_flt" in src and "top_p" in src and "unstable" in src        # the header comment states the tie difference
    ctx = open(os.path.join(ROOT, "vall-e-x_amd", "csrc", "engine_ctx.h")).read()
    assert re.search(r"constexpr int SERVE_UTAB = 13;", ctx) and "const int* row_flt;" in ctx


def test_serve_bench_takes_the_filter_options():
    src = open(os.path.join(ROOT, "tools", "serve_bench.py")).read()
    for opt in ("--top-p", "--repetition-penalty", "--repetition-window", "--min-frames"):
        assert opt in src, opt
