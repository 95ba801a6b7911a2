"""CPU: the numpy restatement of vx_finish's contract (tests/_finish_refs.py), which the device and the host code are compared with,
is itself held to a sequential Python loop, to the S16 rule's half-way and clamp cases and to the span formulas at their edges; the
inputs of the GPU tests keep every frame away from the silence threshold; the symbols, source lists, header constants and `finish=`
arguments are present."""
import inspect
import math
import re
import struct

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _finish_refs as R


@pytest.mark.parametrize("F", R.FRAMES)
def test_frame_energies_equal_a_sequential_loop(F):
    x = R.rows(F)[6].copy()                                # 4801 samples: ten or more frames, a partial last one
    x[5], x[F + 1], x[F + 2], x[2 * F] = np.nan, np.inf, -np.inf, np.float32(-0.0)
    e, p, z = R.frames(x, F)
    assert len(e) == len(p) == len(z) == -(-4801 // F)
    for f in range(len(e)):
        acc, pk, nz = 0.0, 0.0, 0
        for v in x[f * F: (f + 1) * F]:
            v = float(v)
            if not math.isfinite(v):
                nz += 1
                v = 0.0
            acc += v * v                                   # a Python float is a double; the square of an fp32 value is exact in it
            pk = max(pk, abs(v))
        assert struct.pack("<d", acc) == struct.pack("<d", float(e[f])), f
        assert np.float32(pk) == p[f] and nz == z[f], f
    assert z.sum() == 3 and np.signbit(p).sum() == 0


def test_s16_rule_half_way_cases_and_clamp():
    v = np.float32([0.5 / 32768, -0.5 / 32768, 1.5 / 32768, 2.5 / 32768])
    out, clipped = R.apply(v, 0, 4, 1.0, pcm16=True)
    assert out.dtype == np.int16 and out.tolist() == [0, 0, 2, 2] and clipped == 0          # round half to even
    out, clipped = R.apply(np.float32([1.0, 0.99999, -1.0, -1.00002, 0.5]), 0, 5, 1.0, pcm16=True)
    assert out.tolist() == [32767, 32767, -32768, -32768, 16384] and clipped == 3           # -1.0 is representable: not clipped
    out, clipped = R.apply(np.float32([1.0, -1.0, 1.0000001, np.nan, np.inf]), 0, 5, 1.0)
    assert out.tolist() == [1.0, -1.0, np.float32(1.0000001), 0.0, 0.0] and clipped == 1    # fp32: |v| > 1; non-finite in, 0 out


def test_span_edges():
    F = 16
    none = np.zeros(5, bool)
    assert R.span(70, F, none, 0, 3) == (0, 70)
    for trim in (1, 2, 3):
        assert R.span(70, F, none, trim, 3) == (0, 0)                   # no active frame: nothing is kept on a trimmed side
    a = np.array([0, 1, 1, 0, 0], bool)
    assert R.span(70, F, a, 0, 4) == (0, 70)
    assert R.span(70, F, a, 1, 4) == (12, 70) and R.span(70, F, a, 2, 4) == (0, 52) and R.span(70, F, a, 3, 4) == (12, 52)
    assert R.span(70, F, a, 3, 1000) == (0, 70)                         # keep past either end
    last = np.array([0, 0, 0, 0, 1], bool)                              # the partial last frame [64, 70)
    assert R.span(70, F, last, 3, 0) == (64, 70) and R.span(70, F, last, 3, 2) == (62, 70)
    first = np.array([1, 0, 0, 0, 0], bool)
    assert R.span(70, F, first, 3, 5) == (0, 21)
    assert R.span(0, F, np.zeros(0, bool), 3, 5) == (0, 0) and R.span(0, F, np.zeros(0, bool), 0, 5) == (0, 0)


def test_gain_and_tables():
    assert R.gain(R.NONE, -1.0, 20.0, 0.5, 0.01, True) == 1 and R.gain(R.PEAK, -1.0, 20.0, 0.5, 0.01, False) == 1
    assert R.gain(R.PEAK, -1.0, 20.0, 0.0, 0.0, True) == 1 and R.gain(R.RMS, -1.0, 20.0, 0.5, 0.0, True) == 1
    assert R.gain(R.PEAK, 0.0, 20.0, 0.5, 0.01, True) == np.float32(2) and R.gain(R.RMS, 0.0, 20.0, 0.5, 0.01, True) == np.float32(10)
    assert R.gain(R.RMS, 0.0, 6.0, 0.5, 1e-8, True) == np.float32(math.pow(10.0, float(np.float32(6.0)) / 20.0))      # the cap
    assert R.gain(R.PEAK, -6.0, 20.0, 0.25, 0.01, True).dtype == np.float32
    t = R.fade_table(7)
    assert t.dtype == np.float32 and len(t) == 7 and (np.diff(t) > 0).all() and 0 < t[0] and t[-1] < 1
    assert t[3] == np.float32(0.5) and np.allclose(t + t[::-1], 1.0, atol=1e-7)                  # the smoothstep is odd about 1/2
    assert len(R.fade_table(0)) == 0
    x = np.ones(10, np.float32)
    out, _ = R.apply(x, 0, 10, 1.0, fade_in=7, fade_out=7)
    want = np.ones(10, np.float32)
    want[:7] *= t
    want[3:] = want[3:] * t[::-1]                                       # both where they overlap (samples 3 .. 6)
    np.testing.assert_array_equal(out, want)
    out, _ = R.apply(x[:4], 0, 4, 1.0, fade_in=100, fade_out=100)     # a row shorter than the fades uses the part it reaches
    t100 = R.fade_table(100)
    np.testing.assert_array_equal(out, (np.ones(4, np.float32) * t100[:4]) * t100[:4][::-1])


def test_measure_on_a_known_row():
    F = 16
    x = np.zeros(70, np.float32)
    x[16:48] = 0.5
    x[20] = np.nan
    i = R.measure(x, F, silence_db=-40.0, trim=3, keep=2, level_mode=R.PEAK, level_db=0.0)
    assert (i["begin"], i["end"], i["active_frames"], i["nonfinite"], i["clipped"]) == (14, 50, 2, 1, 0)
    assert i["peak"] == np.float32(0.5) and i["gain"] == np.float32(2) and i["mean_square"] == 31 * 0.25 / 32
    out, j = R.finish(x, F, trim=3, keep=2, level_mode=R.PEAK, level_db=0.0, pcm16=True)
    assert j["clipped"] == 31 and out.tolist() == [0, 0] + [32767] * 4 + [0] + [32767] * 27 + [0, 0]


@pytest.mark.parametrize("F", R.FRAMES)
def test_inputs_keep_away_from_the_threshold(F):
    """every frame of every input of the decision-dependent GPU tests: |log2(e_f / (thr2 n_f))| >= 0.25, so that a last-bit difference
    of pow cannot flip a frame"""
    rows = R.rows(F)
    assert [len(r) for r in rows] == R.lengths(F)
    worst = min(R.margin(r, F, -40.0) for r in rows)
    print(f"frame {F}: worst |log2(e / (thr2 n))| = {worst:.2f}")
    assert worst >= 0.25
    big = R.measure(rows[-1], F, trim=3)
    assert 0 < big["begin"] <= 2500 and 13001 - 3100 <= big["end"] < 13001 and big["active_frames"] > 0


def test_abi_lists_the_output_stage():
    from vallex_amd import _build, _capi
    from vallex_amd.utils import generation as G
    from vallex_amd.utils import prompt_making as PM
    assert "vx_finish" in _capi.SYMBOLS
    assert {"vx_dev_finish_frames", "vx_dev_finish_window"} <= set(_capi.DEV_SYMBOLS)
    assert "finish.hip" in _build.SOURCES and "finish.hip" in _build.ENGINE_TUS and "finish_host.h" in _build.ENGINE_HEADERS
    for f in ("finish", "measure", "dev_finish_frames", "dev_finish_window"):
        assert callable(getattr(_capi.Engine, f))
    sig = inspect.signature(_capi.Engine.finish).parameters
    assert list(sig)[1:] == ["wavs", "frame", "silence_db", "trim", "keep", "level_mode", "level_db", "max_gain_db", "fade_in", "fade_out",
                             "pcm16"]
    assert {k: sig[k].default for k in R.DEFAULTS} == R.DEFAULTS
    for fn in (_capi.Engine.vocos_decode, _capi.Engine.encodec_decode, G.generate_audio, G.generate_audio_batch,
               G.generate_audio_from_long_text, G.AudioServer.__init__):
        assert inspect.signature(fn).parameters["finish"].default is None
    for fn in (PM.make_prompt, PM.tokenize_audio):
        assert inspect.signature(fn).parameters["trim_db"].default is None
    f = G.Finish()
    assert f.frame is None and {k: getattr(f, k) for k in R.DEFAULTS} == R.DEFAULTS
    with pytest.raises(Exception):
        f.trim = 1                                                      # frozen
    root = _capi.os.path.dirname(_capi._HERE)
    hdr = open(_capi.os.path.join(root, "include", "vallex_hip.h")).read()
    dev = open(_capi.os.path.join(root, "include", "vallex_hip_dev.h")).read()
    assert f"#define VX_FINISH_WINDOW (1 << {_capi.FINISH_WINDOW.bit_length() - 1})" in hdr
    assert f"#define VX_DEV_FINISH_WINDOW_MIN {_capi.DEV_FINISH_WINDOW_MIN}" in dev
    for name, val in (("VX_PCM_F32", _capi.PCM_F32), ("VX_PCM_S16", _capi.PCM_S16), ("VX_LEVEL_NONE", _capi.LEVEL_NONE),
                      ("VX_LEVEL_PEAK", _capi.LEVEL_PEAK), ("VX_LEVEL_RMS", _capi.LEVEL_RMS)):
        assert re.search(rf"#define {name}\s+{val}\b", hdr), name
    assert "#define VX_ABI_VERSION 6 " in hdr
    # the ctypes structs have the header's fields, in order
    for st in (_capi.vx_finish_opts, _capi.vx_wave_info):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (st.__name__, st.__name__), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == [f[0] for f in st._fields_], (st.__name__, names)
    assert _capi.C.sizeof(_capi.vx_finish_opts) == 44 and _capi.C.sizeof(_capi.vx_wave_info) == 40
    assert _capi.vx_wave_info.mean_square.offset == 32


def test_trim_db_needs_a_loaded_model(monkeypatch):
    from vallex_amd.utils import generation as G
    from vallex_amd.utils import prompt_making as PM
    monkeypatch.setattr(G, "model", None)
    with pytest.raises(RuntimeError, match="preload_models"):
        PM.trim_silence(np.zeros((1, 480), np.float32), -40.0)
