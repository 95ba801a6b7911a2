"""CPU: per-request sampling and cancellation of the serving session -- the additive entry points vx_serve_submit_ex /
vx_serve_cancel (ABI version stays 6), the vx_request_sampling layout, and the request checks that run before any GPU work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import vallex_amd  # noqa: F401  (registers the package under an importable name)
from vallex_amd._capi import ABI_VERSION, SYMBOLS, ServeSession, vx_request_sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(strip_comments=False):
    with open(os.path.join(ROOT, "include", "vallex_hip.h")) as f:
        h = f.read()
    return re.sub(r"/\*.*?\*/", "", h, flags=re.S) if strip_comments else h


def test_header_declares_the_struct_and_the_entry_points():
    h = _header(strip_comments=True)
    assert "typedef struct vx_request_sampling {" in h
    assert re.search(r"\bint vx_serve_submit_ex\(vx_serve\* srv, const vx_batch\* rows, const vx_request\* req,\s*"
                     r"const vx_request_sampling\* smp\s*, int64_t\* ids_out\);", h)
    assert re.search(r"\bint vx_serve_cancel\(vx_serve\* srv, int64_t request_id, int32_t\* state\s*\);", h)
    # vx_serve_submit's own declaration is unchanged, and so is the ABI version
    assert re.search(r"\bint vx_serve_submit\(vx_serve\* srv, const vx_batch\* rows, const vx_request\* req, int64_t\* ids_out\);", h)
    assert re.search(r"#define VX_ABI_VERSION 6\b", h) and ABI_VERSION == 6


def test_request_sampling_layout_matches_header():
    body = re.search(r"typedef struct vx_request_sampling \{(.*?)\} vx_request_sampling;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == [f[0] for f in vx_request_sampling._fields_]
    assert re.findall(r"(u?int32_t|float)\s+\w+\s*;", body) == ["uint32_t", "int32_t", "float", "int32_t"]
    assert [(f[0], getattr(vx_request_sampling, f[0]).offset) for f in vx_request_sampling._fields_] == [
        ("struct_size", 0), ("top_k", 4), ("temperature", 8), ("force_eos_at", 12)]
    assert [f[1] for f in vx_request_sampling._fields_] == [C.c_uint32, C.c_int32, C.c_float, C.c_int32]
    assert C.sizeof(vx_request_sampling) == 16


def test_new_names_are_bound():
    for e in ("vx_serve_submit_ex", "vx_serve_cancel"):
        assert e in SYMBOLS, e
    assert len(SYMBOLS) == len(set(SYMBOLS))
    assert ServeSession.CANCEL_STATES == {0: None, 1: "waiting", 2: "decoding"}


def test_sampling_checks_fire_before_gpu_work():
    for t in (0.0, -1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="temperature"):
            ServeSession.check_request(temperature=t)
    for f in (-2, -100, 1.5, True):
        with pytest.raises(ValueError, match="force_eos_at"):
            ServeSession.check_request(force_eos_at=f)
    for k in (10.0, 2.5, "10", True):
        with pytest.raises(ValueError, match="top_k"):
            ServeSession.check_request(top_k=k)
    # accepted: the reference's values, numpy integers, None = the session's value
    for kw in (dict(top_k=-100, temperature=1.0, force_eos_at=-1), dict(top_k=np.int32(10), temperature=0.6, force_eos_at=0),
               dict(top_k=1, temperature=1.7, force_eos_at=np.int64(30)), dict(top_k=None, temperature=None, force_eos_at=None)):
        assert ServeSession.check_request(**kw) is None


def test_draws_must_cover_the_requests_own_cap():
    # text of 4 ids: the reference's cap is 16 x 4 = 64 frames -> 65 draws; force_eos_at = 7 -> 8 draws; max_new = 20 -> 21 draws
    with pytest.raises(ValueError, match="uniforms"):
        ServeSession.check_request(uniforms=np.zeros(64, np.float32), text_len=4)
    assert ServeSession.check_request(uniforms=np.zeros(65, np.float32), text_len=4).shape == (65, 1)
    with pytest.raises(ValueError, match="uniforms"):
        ServeSession.check_request(uniforms=np.zeros(7, np.float32), text_len=4, force_eos_at=7)
    assert ServeSession.check_request(uniforms=np.zeros(8, np.float32), text_len=4, force_eos_at=7).shape == (8, 1)
    with pytest.raises(ValueError, match="uniforms"):
        ServeSession.check_request(best_of=3, uniforms=np.zeros((20, 3), np.float32), text_len=4, max_new=20)
    assert ServeSession.check_request(best_of=3, uniforms=np.zeros((21, 3), np.float32), text_len=4, max_new=20).shape == (21, 3)
    # force_eos_at = 0: one draw (the forced EOS is the first sample); -1: no cap of its own
    assert ServeSession.check_request(uniforms=np.zeros(1, np.float32), text_len=4, force_eos_at=0).shape == (1, 1)
    with pytest.raises(ValueError, match="uniforms"):
        ServeSession.check_request(uniforms=np.zeros(8, np.float32), text_len=4, force_eos_at=-1)


def test_server_submit_signatures():
    import inspect

    from vallex_amd.models.vallex import Server
    from vallex_amd.utils.generation import AudioServer
    p = inspect.signature(Server.submit).parameters
    assert p["top_k"].default is None and p["temperature"].default is None and p["force_eos_at"].default is None
    p = inspect.signature(AudioServer.submit).parameters
    assert p["top_k"].default == -100 and p["temperature"].default == 1.0


def test_per_row_sampler_source_is_built():
    from vallex_amd import _build
    assert "serve_sample.hip" in _build.SOURCES and "serve_sample.hip" in _build.ENGINE_TUS
    src = open(os.path.join(ROOT, "vall-e-x_amd", "csrc", "serve_sample.hip")).read()
    assert "__global__" in src and "serve_sample_kernel" in src and "row_smp" in src
