"""CPU: the binding side of the continuous schedule (vx_infer_continuous) -- an additive entry point that keeps ABI version 6, and
the argument checks that run before any GPU work."""
import os
import re

import numpy as np
import pytest

import vallex_amd  # noqa: F401  (registers the package under an importable name)
from vallex_amd._capi import ABI_VERSION, SYMBOLS, Engine
from vallex_amd.models.vallex import VALLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "vallex_hip.h")) as f:
        return f.read()


def test_header_declares_the_entry_and_the_binding_lists_it():
    h = _header()
    assert re.search(r"\bint vx_infer_continuous\(vx_ctx\* ctx, const vx_batch\* b, const vx_sampling\* s, vx_row_done_fn on_row,", h)
    assert "typedef void (*vx_row_done_fn)(void* user, int32_t row, const int64_t* codes" in h
    assert "vx_infer_continuous" in SYMBOLS


def test_abi_version_stays_6():
    assert ABI_VERSION == 6
    assert re.search(r"#define VX_ABI_VERSION 6\b", _header())


def _model():
    # no weights and no engine: the checks must fire before the engine (and the GPU) is touched
    return VALLE(1024, 16, 2, norm_first=True, add_prenet=False, prefix_mode=1, share_embedding=True, nar_scale_factor=1.0,
                 prepend_bos=True, num_quantizers=8)


def _row():
    return dict(text=np.array([1, 2, 3], np.int32), prompt=np.zeros((4, 8), np.int32), enroll=1, prompt_language="en",
                text_language="en")


def test_continuous_best_of_is_refused_before_gpu_work():
    m = _model()
    with pytest.raises(ValueError, match="best_of"):
        m.inference_batch([_row()], continuous=True, best_of=2)
    assert m._engine is None
    with pytest.raises(ValueError, match="best_of"):
        Engine.check_continuous(best_of=3, continuous=True)


def test_on_row_needs_continuous():
    m = _model()
    with pytest.raises(ValueError, match="on_row"):
        m.inference_batch([_row()], on_row=lambda r, c: None)
    assert m._engine is None
    Engine.check_continuous(best_of=1, continuous=True, on_row=lambda r, c: None)      # the valid combination passes
