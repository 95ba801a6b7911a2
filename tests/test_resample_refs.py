"""CPU: the references the device resampler is tested against (tests/_resample_refs.py) are themselves held to the geometry table of
the fifteen rate pairs, to the torch resampler of the enrolment path (resample_sinc_hann) under the derived fma bound, and to the exact
impulse response; and the ABI lists the new entries."""
import math

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _resample_refs as R
from vallex_amd.utils import prompt_making as PM

PAIRS = sorted(R.PAIRS)


def test_geometry_is_the_table():
    for (orig, new), want in R.PAIRS.items():
        assert R.geometry(orig, new) == want, (orig, new)
        t = R.taps(orig, new)
        assert t.shape == (want[1], want[3]) and t.dtype == np.float32 and np.isfinite(t).all()


@pytest.mark.parametrize("orig,new", PAIRS)
def test_torch_resampler_is_within_the_fma_bound_of_float64(orig, new):
    o, n, width, K = R.geometry(orig, new)
    tp = R.taps(orig, new)
    worst = 0.0
    for i, L in enumerate(R.lengths(orig, new)):
        x = R.noise(L, 1000 + i)
        got = PM.resample_sinc_hann(x[None], orig, new)[0]
        y, a = R.resample_ref64(x, tp, o, n, width)
        assert got.shape == y.shape == (math.ceil(n * L / o),) == (R.out_len(orig, new, L),)
        err, bd = np.abs(got.astype(np.float64) - y), R.bound(a, K)
        worst = max(worst, float((err / np.maximum(bd, 1e-300)).max()))
        assert (err <= bd).all(), (L, float(err.max()), float(bd.min()))
    print(f"{orig} -> {new}: worst error {worst:.2f} of the bound")


@pytest.mark.parametrize("orig,new", PAIRS)
def test_impulse_gives_back_the_taps(orig, new):
    """x = 1.0 at sample m: output i n + p is taps[p][m + width - i o] bit for bit (one product with 1.0, zeros elsewhere), 0 where no
    tap applies -- through the float64 reference and through the torch resampler"""
    o, n, width, K = R.geometry(orig, new)
    tp = R.taps(orig, new)
    L = 2 * K
    for m in sorted({0, o - 1, K, L - 1}):
        x = np.zeros(L, np.float32)
        x[m] = 1.0
        T = R.out_len(orig, new, L)
        q = np.arange(T)
        j = m + width - (q // n) * o
        want = np.where((j >= 0) & (j < K), tp[q % n, np.clip(j, 0, K - 1)], np.float32(0))
        y, _ = R.resample_ref64(x, tp, o, n, width)
        np.testing.assert_array_equal(y.astype(np.float32), want)
        np.testing.assert_array_equal(PM.resample_sinc_hann(x[None], orig, new)[0], want)


def test_ulp_distance():
    a = np.array([1.0, -1.0, 0.0, 1e-45], np.float32)
    assert R.ulp_diff(a, a).tolist() == [0, 0, 0, 0]
    assert R.ulp_diff(np.float32([1.0]), np.nextafter(np.float32([1.0]), np.float32(2))).tolist() == [1]
    assert R.ulp_diff(np.float32([0.0]), np.float32([-0.0])).tolist() == [0]
    assert R.ulp_diff(np.float32([1e-45]), np.float32([-1e-45])).tolist() == [2]


def test_abi_lists_the_resampler():
    import inspect
    from vallex_amd import _build, _capi
    from vallex_amd.utils import generation as G
    assert "vx_resample" in _capi.SYMBOLS
    assert {"vx_dev_resample_taps", "vx_dev_resample_window"} <= set(_capi.DEV_SYMBOLS)
    assert "resample.hip" in _build.SOURCES and "resample.hip" in _build.ENGINE_TUS
    for f in ("resample", "dev_resample_taps", "dev_resample_window"):
        assert callable(getattr(_capi.Engine, f))
    for fn in (_capi.Engine.vocos_decode, _capi.Engine.encodec_decode, _capi.Engine.encodec_encode):
        assert inspect.signature(fn).parameters["sample_rate"].default == 24000
    for fn in (G.generate_audio, G.generate_audio_batch, G.generate_audio_from_long_text, G.AudioServer.__init__):
        assert inspect.signature(fn).parameters["sample_rate"].default is None
    assert callable(PM.device_resampler) and PM.resampler is None
    hdr = open(_capi.os.path.join(_capi.os.path.dirname(_capi._HERE), "include", "vallex_hip.h")).read()
    dev = open(_capi.os.path.join(_capi.os.path.dirname(_capi._HERE), "include", "vallex_hip_dev.h")).read()
    assert f"#define VX_RESAMPLE_WINDOW (1 << {_capi.RESAMPLE_WINDOW.bit_length() - 1})" in hdr
    assert f"#define VX_DEV_RESAMPLE_WINDOW_MIN {_capi.DEV_RESAMPLE_WINDOW_MIN}" in dev


def test_builtin_resampler_stays_the_torch_path():
    """resampler is None with torch importable: the enrolment path keeps the torch restatement"""
    assert PM._builtin_resampler() is PM.resample_sinc_hann


def test_without_torch_the_builtin_is_the_device_path(monkeypatch):
    """where torch cannot be imported (that case used to raise) the enrolment path resamples on the device"""
    import sys
    monkeypatch.setitem(sys.modules, "torch", None)                  # `import torch` now raises ImportError
    assert PM._builtin_resampler() is PM.device_resampler
    with pytest.raises(RuntimeError, match="preload_models"):        # ... which needs a loaded model
        from vallex_amd.utils import generation as G
        monkeypatch.setattr(G, "model", None)
        PM.device_resampler(np.zeros((1, 8), np.float32), 16000, 24000)
