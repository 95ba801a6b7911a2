"""CPU: the binding side of batched best_of -- injected uniforms are [steps][batch x best_of] (column r*best_of + j = beam j of row
r), and the ABI version says that a best_of call may carry more than one row."""
import os
import re

import numpy as np
import pytest

import vallex_amd  # noqa: F401  (registers the package under an importable name)
from vallex_amd._capi import ABI_VERSION, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sampling(n, uniforms, best_of):
    return Engine._sampling(n, -100, 1.0, uniforms, 0, None, 8, best_of=best_of)


def test_uniforms_are_batch_times_best_of_columns():
    s, u = _sampling(4, np.zeros((10, 12), np.float32), 3)
    assert s.uniforms_steps == 10 and s.best_of == 3 and u.shape == (10, 12)
    with pytest.raises(AssertionError, match=r"\[steps\]\[4 x 3\]"):
        _sampling(4, np.zeros((10, 3), np.float32), 3)      # the batch-1 shape is not enough for four rows
    s, _ = _sampling(1, np.zeros((10, 5), np.float32), 5)   # batch 1: [steps][best_of], as before
    assert s.uniforms_steps == 10
    s, _ = _sampling(4, np.zeros((10, 4), np.float32), 1)   # no beams: [steps][batch], as before
    assert s.uniforms_steps == 10


def test_header_abi_version_is_6():
    hdr = open(os.path.join(ROOT, "include", "vallex_hip.h")).read()
    assert int(re.search(r"#define VX_ABI_VERSION (\d+)", hdr).group(1)) == 6 == ABI_VERSION
