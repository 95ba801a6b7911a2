"""CPU: the numpy restatement of vx_stretch's contract (tests/_stretch_refs.py), which the device and the host code are compared with,
is itself held to a sequential Python loop, to the tie rule, to the self-match at speed 1, to what a time-stretch is for (the length
changes, the pitch and the level do not) and to its edges; `stretched_sample` follows a hand-written table; the symbols, source
lists, header constants, struct layout and `speed=` arguments are present."""
import ctypes as C
import inspect
import math
import os
import re
import struct
from fractions import Fraction

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _stretch_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(v):
    return struct.pack("<d", float(v))


def test_candidate_sums_equal_a_sequential_loop():
    H, D = 16, 5
    rng = np.random.default_rng(1)
    x = (0.3 * rng.standard_normal(3 * H + 2 * D)).astype(np.float32)
    x[3], x[9], x[20], x[22], x[30] = np.nan, np.inf, -np.inf, np.float32(-0.0), np.float32(1e-41)
    y = R.clean(x)
    assert np.isfinite(y).all() and y[3] == 0 and y[9] == 0 and y[20] == 0 and np.signbit(y[22]) and y[30] != 0
    n1 = R.nominal(1, 4, 5, H)                            # frame 1 at 4/5: the template is y[H .. 2H), the region starts at n_1 - D
    row = R._Row(x)
    t = row.take(H, H)
    c, e = R.frame_sums(row.take(n1 - D, 2 * D + H), t)
    assert len(c) == len(e) == 2 * D + 1
    for i in range(2 * D + 1):
        cs, es = 0.0, 0.0
        for j in range(H):
            s = n1 + (i - D) + j
            a = float(y[s]) if 0 <= s < len(y) else 0.0     # a Python float is a double; a product of two fp32 values is exact in it
            cs += a * float(y[H + j])
            es += a * a
        assert _bits(cs) == _bits(c[i]) and _bits(es) == _bits(e[i]), i
    out, pos, cost = R.stretch(x, 4, 5, H, D)
    Dd = e - 2.0 * c
    assert pos[1] == n1 + R.pick(Dd, D) - D and _bits(cost[1]) == _bits(Dd[R.pick(Dd, D)])


def test_tie_rule():
    assert R.pick(np.array([1.0, 0.0, 0.0, 0.0, 1.0]), 2) == 2          # the smallest |d|
    assert R.pick(np.array([0.0, 1.0, 2.0, 1.0, 0.0]), 2) == 0          # then the negative d
    assert R.pick(np.array([0.0, -0.0, 5.0]), 1) == 1                   # -0.0 == 0.0: a tie
    H, D = 240, 150
    out, pos, cost = R.stretch(np.zeros(4801, np.float32), 4, 5, H, D)
    assert len(out) == 6002 and not out.any() and not cost.any()
    assert pos.tolist() == [R.nominal(k, 4, 5, H) for k in range(len(pos))]


def test_speed_one_general_path_copies():
    H, D = 240, 150
    x = (0.1 * np.random.default_rng(0).standard_normal(4801)).astype(np.float32)
    out, pos, cost = R.stretch(x, 1, 1, H, D, shortcut=False)
    assert pos.tolist() == [k * H for k in range(21)]                   # the self-match wins
    np.testing.assert_array_equal(out.view(np.uint32), x.view(np.uint32))
    assert cost[0] == 0 and (cost[1:] < 0).all()                        # D = -(the template's energy) at a perfect match
    out2, pos2, _ = R.stretch(x, 3, 3, H, D)                            # the shortcut, from an unreduced speed
    np.testing.assert_array_equal(out2.view(np.uint32), x.view(np.uint32))
    assert pos2.tolist() == pos.tolist()


@pytest.mark.parametrize("f", [200.0, 137.0])
@pytest.mark.parametrize("speed", [(1, 2), (4, 5), (5, 4), (3, 2), (2, 1)])
def test_rate_changes_pitch_does_not(f, speed):
    sr, H, D = 24000, 240, 150
    num, den = speed
    x = (0.5 * np.sin(2 * np.pi * f * np.arange(sr) / sr)).astype(np.float32)
    out, pos, _ = R.stretch(x, num, den, H, D)
    assert len(out) == -(-sr * den // num)
    core = out[2 * H: len(out) - 4 * H].astype(np.float64)
    spec = np.abs(np.fft.rfft(core * np.hanning(len(core))))
    peak = np.fft.rfftfreq(len(core), 1.0 / sr)[int(np.argmax(spec))]
    rms = math.sqrt(float(np.mean(core ** 2)))
    print(f"f {f} speed {num}/{den}: peak {peak:.3f} Hz (bin {sr / len(core):.3f} Hz), rms {rms:.6f}")
    assert abs(peak - f) <= sr / len(core)
    assert abs(rms - 0.35355) <= 0.005 * 0.35355


@pytest.mark.parametrize("H", R.HOPS)
def test_edges(H):
    n = 0
    for L in (0, 1, H - 1, H, H + 1, 3 * H + 7):
        rng = np.random.default_rng(L)
        x = (0.2 * rng.standard_normal(L)).astype(np.float32)
        if L > 2:
            x[L // 2], x[0] = np.nan, np.inf
        for D in (0, 5, 150):
            for num, den in R.SPEEDS:
                out, pos, cost = R.stretch(x, num, den, H, D)
                Lout = -(-L * den // num)
                assert len(out) == Lout and len(pos) == len(cost) == -(-Lout // H)
                assert np.isfinite(out).all() and np.isfinite(cost).all()
                nk = np.array([k * H * num // den for k in range(len(pos))], np.int64)
                assert (np.abs(pos - nk) <= D).all() and (len(pos) == 0 or pos[0] == 0)
                m = min(H, Lout)                                   # frame 0 is the input (zeros behind its end)
                np.testing.assert_array_equal(out[:m], np.concatenate([R.clean(x), np.zeros(H, np.float32)])[:m])
                n += 1
    assert n == 6 * 3 * 7


def test_lengths_in_python_integers():
    for L in (0, 1, 4801, 2 ** 31 - 1):
        assert R.out_len(L, 1, 2) == 2 * L and R.out_len(L, 2, 1) == (L + 1) // 2 and R.out_len(L, 6, 4) == -(-2 * L // 3)
    assert R.nominal(2 ** 28, 1000, 999, 16) == 2 ** 32 * 1000 // 999 and R.reduce_speed(32766, 16383) == (2, 1)
    assert R.frames(4801, 4, 5, 240) == 26 and R.frames(0, 4, 5, 240) == 0


def test_stretched_sample():
    from vallex_amd.utils.alignment import stretched_sample
    pos, hop = [0, 190, 385, 570], 240                    # four hops at about 4/5: 960 output samples
    assert stretched_sample(pos, hop, 0) == 0 and stretched_sample(pos, hop, 100) == 100
    assert stretched_sample(pos, hop, 189) == 189 and stretched_sample(pos, hop, 190) == 240        # hop 1 takes over at its position
    assert stretched_sample(pos, hop, 384) == 240 + 194 and stretched_sample(pos, hop, 385) == 480
    assert stretched_sample(pos, hop, 600) == 750
    assert stretched_sample(pos, hop, 5000) == 959 and stretched_sample(pos, hop, -3) == 0          # clamped to the output
    assert stretched_sample(pos, hop, 5000, out_len=950) == 949
    got = stretched_sample(pos, hop, np.array([[0, 190], [600, 5000]]))
    assert got.dtype == np.int64 and got.tolist() == [[0, 240], [750, 959]]
    assert stretched_sample([0, 200, 150, 400], 100, 160) == 210 and stretched_sample([0, 200, 150, 400], 100, 149) == 149   # not rising
    assert isinstance(stretched_sample(pos, hop, 7), int)
    out, p, _ = R.stretch((0.1 * np.random.default_rng(3).standard_normal(2000)).astype(np.float32), 5, 4, 240, 150)
    assert (np.diff(stretched_sample(p, 240, np.arange(0, 2000, 320), out_len=len(out))) >= 0).all()


def test_symbols_sources_constants_and_arguments_are_present():
    from vallex_amd import _build, _capi
    from vallex_amd.utils import generation
    assert "vx_stretch" in _capi.SYMBOLS and {"vx_dev_stretch_window", "vx_dev_stretch_costs"} <= set(_capi.DEV_SYMBOLS)
    assert "stretch.hip" in _build.SOURCES and "stretch.hip" in _build.ENGINE_TUS and "stretch_host.h" in _build.ENGINE_HEADERS
    pub = open(os.path.join(ROOT, "include", "vallex_hip.h")).read()
    dev = open(os.path.join(ROOT, "include", "vallex_hip_dev.h")).read()
    assert re.search(r"#define VX_STRETCH_WINDOW \(1 << 23\)", pub) and _capi.STRETCH_WINDOW == 1 << 23
    assert re.search(r"#define VX_ABI_VERSION 6\b", pub) and _capi.ABI_VERSION == 6
    m = re.search(r"#define VX_DEV_STRETCH_WINDOW_MIN (\d+)", dev)
    assert m and int(m.group(1)) == _capi.DEV_STRETCH_WINDOW_MIN >= 2 * 300 + 3 * 441
    body = re.search(r"typedef struct vx_stretch_opts \{(.*?)\} vx_stretch_opts;", pub, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == ["struct_size", "speed_num", "speed_den", "hop", "search"] == [f[0] for f in _capi.vx_stretch_opts._fields_]
    assert C.sizeof(_capi.vx_stretch_opts) == 20
    for word in ("Samples.", "Lengths.", "Nominal positions.", "Frame 0.", "Search, for k >= 1.", "Crossfade.", "Positions.", "Speed 1.",
                 "Exactness.", "State."):
        assert word in pub, word
    for fn in (_capi.Engine.vocos_decode, _capi.Engine.encodec_decode, generation.generate_audio, generation.generate_audio_batch,
               generation.generate_audio_from_long_text, generation.AudioServer.__init__):
        assert inspect.signature(fn).parameters["speed"].default is None, fn
    sig = inspect.signature(_capi.Engine.stretch).parameters
    assert list(sig)[1:] == ["wavs", "speed", "hop", "search", "sample_rate", "return_positions"]
    assert sig["hop"].default is None and sig["search"].default is None and sig["sample_rate"].default == 24000
    assert hasattr(_capi.Engine, "dev_stretch_window") and hasattr(_capi.Engine, "dev_stretch_costs")
    o = _capi.Engine._stretch_opts(1.25, None, None, 24000)
    assert (o.speed_num, o.speed_den, o.hop, o.search) == (5, 4, 240, 150)
    o = _capi.Engine._stretch_opts(Fraction(4, 5), 441, 0, 24000)
    assert (o.speed_num, o.speed_den, o.hop, o.search) == (4, 5, 441, 0)
    o = _capi.Engine._stretch_opts((6, 4), None, None, 16000)
    assert (o.speed_num, o.speed_den, o.hop, o.search) == (6, 4, 160, 100)
    assert _capi.Engine._stretch_opts(0.8, None, None, 24000).speed_den == 5
