"""CPU: the equaliser's contract without a GPU -- the binding and the header, vx_eq_design against the cookbook in numpy, vx_eq_plan's
warm-up W against the numpy restatement (tests/_eq_refs.py) and its refusals, the truncation bound the W rule buys, the identity
section, Eq.response against what the restatement does to a sine, and the `eq=` keywords of the generation layer on stub engines.
Every test but the design one computes with the library's coefficients, so the two libms never matter again."""
import inspect
import math
import os
import re
import types

import numpy as np
import pytest

import vallex_amd
from tests import _eq_refs as R
from vallex_amd import _capi
from vallex_amd._capi import Engine
from vallex_amd.utils import generation as G
from vallex_amd.utils import prompt_making as PM
from vallex_amd.utils.generation import Eq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24                     # half an fp32 ulp of a value in [1, 2): the rounding of x to fp32 moves it by at most U |x|


def _lib_sections(specs, rate):
    return np.stack([Engine.eq_design(k, f, q, g, rate) for k, f, q, g in specs])


@pytest.fixture(scope="module")
def filters():
    """the six filters of the contract's table with the library's coefficients: (name, sections, W of the restatement)"""
    out = []
    for name, rate, specs in R.FILTERS:
        s = _lib_sections(specs, rate)
        out.append((name, s, R.warm(s)))
    return out


def test_binding_header_and_keywords_agree():
    hdr = open(os.path.join(ROOT, "include", "vallex_hip.h")).read()
    dev = open(os.path.join(ROOT, "include", "vallex_hip_dev.h")).read()
    body = re.search(r"typedef struct vx_eq_info \{(.*?)\} vx_eq_info;", hdr, re.S).group(1)
    names = [n for decl in re.findall(r"\w+\s+([^;]+);", body) for n in re.findall(r"\w+", decl)]
    assert names == [f[0] for f in _capi.vx_eq_info._fields_] == ["warm", "nonfinite", "nonfinite_out", "peak"]
    assert int(re.search(r"#define VX_ABI_VERSION (\d+)", hdr).group(1)) == _capi.ABI_VERSION == 6
    assert int(re.search(r"#define VX_EQ_MAX_SECTIONS (\d+)", hdr).group(1)) == _capi.EQ_MAX_SECTIONS == R.MAX_SECTIONS == 8
    assert int(re.search(r"#define VX_EQ_WARM_MAX (\d+)", hdr).group(1)) == _capi.EQ_WARM_MAX == R.WARM_MAX == 65536
    step = int(re.search(r"#define VX_EQ_STEP (\d+)", hdr).group(1))
    assert Engine.eq_plan(R.IDENTITY) == (32, step) and step % 32 == 0
    assert int(re.search(r"#define VX_EQ_WINDOW \(1 << (\d+)\)", hdr).group(1)) == 23 and _capi.EQ_WINDOW == 1 << 23
    assert int(re.search(r"#define VX_DEV_EQ_WINDOW_MIN (\d+)", dev).group(1)) == _capi.DEV_EQ_WINDOW_MIN
    for k, v in _capi.EQ_KINDS.items():
        assert int(re.search(r"#define VX_EQ_%s (\d+)" % k.replace("_", "").upper(), hdr).group(1)) == v == R.KINDS[k]
    assert {"vx_eq", "vx_eq_design", "vx_eq_plan", "vx_eq_last_error"} <= set(_capi.SYMBOLS) and "vx_dev_eq_window" in _capi.DEV_SYMBOLS
    lib = vallex_amd.load_library()
    for name in ("vx_eq", "vx_eq_design", "vx_eq_plan", "vx_eq_last_error", "vx_dev_eq_window"):
        assert getattr(lib, name)
    sig = inspect.signature(Engine.eq).parameters
    assert list(sig)[1:] == ["wavs", "sections", "sample_rate", "return_info"] and sig["sample_rate"].default == 24000
    for fn in (G.generate_audio, G.generate_audio_batch, G.generate_audio_from_long_text, G.AudioServer.__init__, PM.tokenize_audio,
               PM.make_prompt, Engine.vocos_decode, Engine.encodec_decode):
        assert inspect.signature(fn).parameters["eq"].default is None, fn


@pytest.mark.parametrize("rate", [8000, 16000, 24000, 48000])
def test_design_is_the_cookbooks(rate):
    """every kind against the cookbook formulas in numpy; relative 1e-12 is the margin for two libms (sin, cos, pow, sqrt)"""
    n = 0
    for kind in R.KINDS:
        for f0, q, g in ((20.0, 0.7071, 6.0), (80.0, 0.5, -12.0), (1000.0, 8.0, 24.0), (0.2 * rate, 1.3066, -3.0), (0.49 * rate, 0.3, 0.5)):
            got, want = Engine.eq_design(kind, f0, q, g, rate), R.design(kind, rate, f0, q, g)
            assert got.shape == (5,) and got.dtype == np.float64
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=str((kind, rate, f0, q, g)))
            np.testing.assert_array_equal(got, Engine.eq_design(R.KINDS[kind], f0, q, g, rate))      # by number as by name
            assert R.check(got) is None, (kind, rate, f0, q, g)           # a designed section is stable
            n += 1
    assert n == 35
    # the cookbook's own words on a case with round numbers: the high-pass at a quarter of the rate, Q 1/2 -> (1/4)(1 - z^-1)^2
    np.testing.assert_allclose(Engine.eq_design("highpass", rate / 4.0, 0.5, 0.0, rate), [0.25, -0.5, 0.25, 0.0, 0.0], rtol=0, atol=1e-15)


def test_design_refusals_name_the_field():
    for field, args in (("f0", ("highpass", 12000.0, 0.7071, 0.0, 24000)), ("f0", ("highpass", 13000.0, 0.7071, 0.0, 24000)),
                        ("f0", ("peak", 0.0, 1.0, 0.0, 24000)), ("f0", ("peak", float("nan"), 1.0, 0.0, 24000)),
                        ("q", ("lowpass", 100.0, 0.0, 0.0, 24000)), ("q", ("lowpass", 100.0, -1.0, 0.0, 24000)),
                        ("q", ("lowpass", 100.0, float("inf"), 0.0, 24000)), ("gain_db", ("peak", 100.0, 1.0, 24.5, 24000)),
                        ("gain_db", ("low_shelf", 100.0, 1.0, float("nan"), 24000)), ("sample_rate", ("notch", 100.0, 1.0, 0.0, 7999)),
                        ("sample_rate", ("notch", 100.0, 1.0, 0.0, 192001)), ("kind", (7, 100.0, 1.0, 0.0, 24000)),
                        ("kind", (-1, 100.0, 1.0, 0.0, 24000)), ("kind", ("allpass", 100.0, 1.0, 0.0, 24000))):
        with pytest.raises(ValueError, match=field):
            Engine.eq_design(*args)
    assert Engine.eq_design("peak", 100.0, 1.0, 24.0, 8000).shape == (5,) and Engine.eq_design("peak", 100.0, 1.0, -24.0, 192000).shape == (5,)
    lib = vallex_amd.load_library()
    assert lib.vx_eq_design(0, 24000, 80.0, 0.7, 0.0, None) == _capi.VX_EINVAL and b"c is NULL" in lib.vx_eq_last_error()


def test_warm_equals_the_restatement_on_the_six_filters(filters):
    got = {name: Engine.eq_plan(s)[0] for name, s, _ in filters}
    assert got == {name: W for name, _, W in filters}
    assert all(W % 32 == 0 and 0 < W <= R.WARM_MAX for W in got.values())
    # the table of the contract's note, reproduced: orientation, the line above is the test
    assert got == {"rumble": 1120, "highpass 20 Hz at 48 kHz": 8960, "telephone": 608, "presence": 64, "low shelf 100 Hz +6 dB": 1088,
                   "peak 1 kHz Q 8 -12 dB": 544}
    assert Engine.eq_plan(Eq.rumble())[0] == 1120 and Engine.eq_plan(Eq.telephone())[0] == 608 and Engine.eq_plan(Eq.presence())[0] == 64
    assert Engine.eq_plan(Eq.rumble(), 48000)[0] > 1120                    # an Eq is resolved at the rate of the call


def test_plan_refusals_carry_a_message():
    rate, (k, f, q, g) = R.HUM_NOTCH
    notch = Engine.eq_design(k, f, q, g, rate)
    assert R.check(notch) is None
    with pytest.raises(ValueError, match="memory is too long"):
        Engine.eq_plan(notch)
    with pytest.raises(ValueError, match="too long"):
        R.warm(notch)
    with pytest.raises(ValueError, match="too long"):
        Engine.eq_plan(Eq.notch(50.0, 100.0))
    ok = Engine.eq_design("highpass", 80.0)
    for bad, want in ((np.array([1.0, 0.0, 0.0, 0.0, 1.0]), "section 0 is unstable"), (np.array([1.0, 0.0, 0.0, 0.0, -1.0]), "section 0 is unstable"),
                      (np.array([1.0, 0.0, 0.0, 1.5, 0.5]), "section 0 is unstable"), (np.array([1.0, 0.0, 0.0, -1.5, 0.5]), "section 0 is unstable"),
                      (np.stack([ok, [1.0, 0.0, 0.0, 0.0, 1.0]]), "section 1 is unstable"),
                      (np.array([1.0, np.nan, 0.0, 0.0, 0.0]), "section 0: coefficient 1"), (np.stack([ok, [1.0, 0.0, 0.0, 0.0, np.inf]]), "section 1: coefficient 4"),
                      (np.zeros((0, 5)), "nsections 0"), (np.tile(ok, (9, 1)), "nsections 9")):
        assert (R.check(bad) or "").startswith(want), (bad, R.check(bad))
        with pytest.raises(ValueError, match=want):
            Engine.eq_plan(bad)
    assert Engine.eq_plan(np.tile(ok, (8, 1)))[0] > 1120                   # eight are taken
    with pytest.raises(ValueError, match="more|at most"):
        Eq.rumble() + Eq.telephone() + Eq.telephone()
    with pytest.raises(ValueError, match="f0"):
        Eq.highpass(12000.0).sections(24000)
    with pytest.raises(ValueError, match="q"):
        Eq.highpass(100.0, 0.0)
    with pytest.raises(ValueError, match="no section"):
        Engine.eq_plan(Eq())
    lib = vallex_amd.load_library()
    assert lib.vx_eq_plan(None, 1, None, None) == _capi.VX_EINVAL and b"NULL" in lib.vx_eq_last_error()


def test_truncation_bound_on_the_six_filters(filters):
    """|restatement - unbounded recursion| <= 2^-24 peak(x) + 2^-24 |unbounded|: the first term is the truncation bound peak(x) T(W)
    of the contract, the second the one rounding of the output to fp32 (half an ulp of y is at most 2^-24 |y|)"""
    x = R.noise_row(12000, seed=33, dc=0.3)
    S = Engine.eq_plan(R.IDENTITY)[1]
    peak = float(np.abs(x).max())
    worst = 0.0
    for name, s, W in filters:
        got, info = R.eq(x, s, W, S)
        want = R.full(x, s)
        d = np.abs(got.astype(np.float64) - want)
        bound = U * peak + U * np.abs(want)
        assert (d <= bound).all(), (name, float((d / bound).max()))
        assert info["nonfinite"] == info["nonfinite_out"] == 0 and info["warm"] == W
        worst = max(worst, float(d.max()) / peak)
    assert worst < 2 * U                                                  # of the input peak, output rounding included


def test_identity_returns_the_input_bits():
    x = R.noise_row(1000, seed=7, dc=0.1)
    x[[0, 255, 256, 600, 999]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    W, S = Engine.eq_plan(R.IDENTITY)
    got, info = R.eq(x, R.IDENTITY, W, S)
    want = np.where(np.isfinite(x), x, np.float32(0))
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert info == dict(warm=32, nonfinite=5, nonfinite_out=0, peak=np.abs(want).max())
    two, _ = R.eq(x, np.tile(R.IDENTITY, (2, 1)), W, S)
    np.testing.assert_array_equal(two.view(np.uint32), want.view(np.uint32))


PRESET_FREQS = {"rumble": (20.0, 80.0, 300.0, 1000.0, 8000.0), "telephone": (100.0, 300.0, 1000.0, 3400.0, 6000.0),
                "presence": (200.0, 1000.0, 3000.0, 8000.0, 11000.0)}


@pytest.mark.parametrize("preset", sorted(PRESET_FREQS))
def test_response_is_what_the_restatement_does_to_a_sine(preset):
    """Eq.response(f) against the amplitude sqrt(ys^2 + yc^2) of what the restatement gives a sine and a cosine of amplitude A at f,
    at every sample from W on.  The margin, derived: an output at n >= W is the steady state A |H| sin(..) up to (1) the truncation,
    at most A T(W) <= 2^-24 A (the contract's bound: the samples zeroed in front of the lane's start, or in front of the row, lie at
    least W back); (2) the fp32 rounding of the sine, at most 2^-24 A per input sample, which the filter passes with a gain of at most
    T(0) = sum |h|; (3) the one rounding of the output, at most 2^-24 |y| <= 2^-24 A |H|.  Each of ys, yc is therefore within
    d = 2^-24 A (1 + T(0) + |H|) of its steady state, and the amplitude within sqrt(2) d (the length of the error vector).  1e-12 A
    covers the double roundoff of the recursion itself, nine orders above it."""
    eq = getattr(Eq, preset)()
    s = eq.sections(24000)
    W, S = Engine.eq_plan(s)
    A, n = 0.5, np.arange(W + 2 * S + 7, dtype=np.float64)
    H = eq.response(PRESET_FREQS[preset], 24000)
    np.testing.assert_allclose(H, R.response(s, PRESET_FREQS[preset], 24000), rtol=1e-12)
    T0 = R.l1(s)
    for f, h in zip(PRESET_FREQS[preset], H):
        ph = 2.0 * np.pi * f * n / 24000.0
        ys = R.eq((A * np.sin(ph)).astype(np.float32), s, W, S)[0].astype(np.float64)
        yc = R.eq((A * np.cos(ph)).astype(np.float32), s, W, S)[0].astype(np.float64)
        amp = np.sqrt(ys * ys + yc * yc)[W:]
        margin = math.sqrt(2.0) * U * A * (1.0 + T0 + h) + 1e-12 * A
        assert np.abs(amp - A * h).max() <= margin, (preset, f, float(np.abs(amp - A * h).max()), margin)
    # what the presets are for, in round numbers
    if preset == "rumble":
        assert H[0] < 0.07 and abs(H[1] - math.sqrt(0.5)) < 1e-3 and abs(H[3] - 1.0) < 1e-3
    if preset == "telephone":
        assert H[0] < 0.02 and abs(H[1] - math.sqrt(0.5)) < 2e-3 and abs(H[2] - 1.0) < 0.01 and abs(H[3] - math.sqrt(0.5)) < 2e-3 and H[4] < 0.11
    if preset == "presence":
        assert abs(20 * math.log10(H[2]) - 4.0) < 0.3 and abs(20 * math.log10(H[4]) - 3.0) < 0.3 and abs(H[0] - 1.0) < 0.01


def test_eq_objects():
    a, b = Eq.peak(1000.0, -3.0, 2.0), Eq.low_shelf(120.0, 2.0)
    assert isinstance(a + b, Eq) and tuple(a + b) == (("peak", 1000.0, 2.0, -3.0), ("low_shelf", 120.0, 0.7071, 2.0))
    assert len(Eq.telephone()) == 4 and len(Eq.presence()) == 2 and len(Eq.telephone() + Eq.presence() + a + b) == 8
    assert tuple(Eq.telephone()) == (("highpass", 300.0, 0.5412, 0.0), ("highpass", 300.0, 1.3066, 0.0), ("lowpass", 3400.0, 0.5412, 0.0),
                                     ("lowpass", 3400.0, 1.3066, 0.0))
    assert tuple(Eq.rumble()) == (("highpass", 80.0, 0.7071, 0.0),) and hash(Eq.rumble()) == hash(Eq.highpass(80.0, 0.7071))
    with pytest.raises((AttributeError, TypeError)):
        a.extra = 1
    with pytest.raises(ValueError, match="kind"):
        Eq([("allpass", 100.0, 1.0, 0.0)])
    with pytest.raises(ValueError, match="gain_db"):
        Eq.peak(100.0, 30.0)
    np.testing.assert_array_equal(Eq.rumble().sections(16000)[0], Engine.eq_design("highpass", 80.0, 0.7071, 0.0, 16000))
    np.testing.assert_array_equal(Engine._eq_sections(Eq.rumble(), 8000), Eq.rumble().sections(8000))
    with pytest.raises(ValueError, match="shape"):
        Engine._eq_sections(np.zeros((2, 4)))


# ---- the generation layer on stub engines ----------------------------------------------------------------------------------------------

class _StageEngine(Engine):
    """an Engine without a context: the vocoder entries of the library answer 0 and write nothing, every stage records its name"""

    def __init__(self):
        self.calls = []
        self.ctx = None
        self.lib = types.SimpleNamespace(vx_vocos_decode=lambda *a: 0, vx_encodec_decode=lambda *a: 0)

    def denoise(self, rows, **kw):
        self.calls.append("denoise")
        return rows, []

    def _paused(self, rows, pauses, rate=24000):
        if pauses is not None:
            self.calls.append("pauses")
        return rows

    def stretch(self, rows, speed):
        self.calls.append("stretch")
        return rows

    def eq(self, rows, sections, sample_rate=24000, return_info=False):
        self.calls.append(("eq", sample_rate, len(self._eq_sections(sections, sample_rate))))
        return rows

    def resample(self, rows, a, b):
        self.calls.append(("resample", a, b))
        return rows


def test_engine_order_of_the_stages_and_eq_none_calls_nothing():
    codes = [np.zeros((12, 8), np.int64)]
    for decode in ("vocos_decode", "encodec_decode"):
        kw = dict(bandwidth_id=2) if decode == "vocos_decode" else {}
        e = _StageEngine()
        getattr(e, decode)(codes, sample_rate=8000, **kw)
        assert e.calls == [("resample", 24000, 8000)]
        e = _StageEngine()
        getattr(e, decode)(codes, sample_rate=8000, eq=None, **kw)
        assert e.calls == [("resample", 24000, 8000)]
        e = _StageEngine()
        getattr(e, decode)(codes, sample_rate=8000, denoise=True, pauses=G.Pauses(max_ms=300.0), speed=1.25, eq=Eq.telephone(), **kw)
        assert e.calls == ["denoise", "pauses", "stretch", ("eq", 24000, 4), ("resample", 24000, 8000)]
        e = _StageEngine()
        out = getattr(e, decode)(codes, eq=Eq.rumble(), **kw)
        assert e.calls == [("eq", 24000, 1)] and len(out) == 1 and len(out[0]) == 12 * 320
        e = _StageEngine()
        with pytest.raises(ValueError, match="too long"):                  # before the vocoder runs
            getattr(e, decode)(codes, eq=Eq.notch(50.0, 100.0), **kw)
        assert e.calls == []


class _GenEngine:
    """stands in for model.engine under utils.generation / utils.prompt_making: records the stages, refuses like the real one"""

    def __init__(self):
        self.calls = []

    def eq_plan(self, eq, rate=24000):
        self.calls.append(("eq_plan", rate))
        return Engine.eq_plan(eq, rate)

    def _equalised(self, rows, eq, rate=24000):
        self.calls.append(("eq", rate))
        return rows

    def _denoised(self, rows, denoise):
        self.calls.append("denoise")
        return rows

    def _denoise_opts(self, **kw):
        return None

    def _denoise_parts(self, denoise):
        return {}

    def _paused(self, rows, pauses, rate=24000):
        self.calls.append("pauses")
        return rows

    def stretch(self, rows, speed):
        self.calls.append("stretch")
        return rows

    def resample(self, rows, a, b):
        self.calls.append(("resample", a, b))
        return rows

    def vocos_decode(self, codes, bw, **kw):
        self.calls.append(("vocos_decode", kw.get("eq")))
        return [np.zeros(320 * len(c), np.float32) for c in codes]


class _GenModel:
    def __init__(self):
        self.engine, self.calls = _GenEngine(), 0

    def inference(self, x, x_lens, y, enroll_x_lens=0, **kw):
        self.calls += 1
        return np.zeros((1, 3, 8), np.int64)

    def inference_batch(self, rows, **kw):
        self.calls += 1
        return [np.zeros((3, 8), np.int64) for _ in rows]


class _GenVocos:
    def codes_to_features(self, frames):
        return np.asarray(frames)

    def decode(self, features, bandwidth_id=None):
        return np.zeros((1, 320 * features.shape[-1]), np.float32)


@pytest.fixture
def gen(monkeypatch):
    m = _GenModel()
    monkeypatch.setattr(G, "model", m)
    monkeypatch.setattr(G, "vocos", _GenVocos())
    monkeypatch.setattr(G, "rng", None)
    monkeypatch.setattr(G, "language_detector", lambda t: "en")
    monkeypatch.setattr(G, "sentence_splitter", lambda t: t.split("|"))
    monkeypatch.setattr(G, "text_tokenizer", lambda t: ([7] * 4, ["en"] * 4))
    return m


def test_generation_layer_order_and_none(gen):
    e = gen.engine
    assert G.generate_audio("hello", language="en").shape == (960,) and e.calls == []                       # eq=None calls nothing
    assert G.generate_audio("hello", language="en", eq=None, sample_rate=8000).shape == (960,) and e.calls == [("resample", 24000, 8000)]
    e.calls.clear()
    G.generate_audio("hello", language="en", eq=Eq.telephone(), sample_rate=8000, denoise=True, pauses=G.Pauses(max_ms=300.0), speed=1.25)
    assert e.calls == [("eq_plan", 24000), "denoise", "pauses", "stretch", ("eq", 24000), ("resample", 24000, 8000)]
    e.calls.clear()
    G.generate_audio("hello", language="en", eq=Eq.rumble())
    assert e.calls == [("eq_plan", 24000), ("eq", 24000)]
    e.calls.clear()
    G.generate_audio_from_long_text("one|two", language="en", eq=Eq.presence(), sample_rate=16000)
    assert e.calls == [("eq_plan", 24000), ("eq", 24000), ("resample", 24000, 16000)]
    e.calls.clear()
    tele = Eq.telephone()
    G.generate_audio_batch(["a", "b"], language="en", eq=tele, sample_rate=8000)
    assert e.calls == [("eq_plan", 24000), ("vocos_decode", tele)]
    e.calls.clear()
    G.generate_audio_batch(["a", "b"], language="en")
    assert e.calls == [("vocos_decode", None)]


def test_check_eq_raises_before_any_model_work(gen):
    for bad, why in ((Eq.highpass(13000.0), "f0"), (Eq.notch(50.0, 100.0), "too long"), (Eq(), "no section")):
        for call in (lambda: G.generate_audio("hello", language="en", eq=bad), lambda: G.generate_audio_batch(["a"], language="en", eq=bad),
                     lambda: G.generate_audio_from_long_text("one|two", language="en", eq=bad), lambda: G.AudioServer(eq=bad)):
            with pytest.raises(ValueError, match=why):
                call()
    assert gen.calls == 0 and all(c[0] == "eq_plan" for c in gen.engine.calls)


def test_enrolment_runs_eq_first_of_all(gen):
    class Tok:
        sample_rate = 24000

        def encode(self, wav):
            return [(np.zeros((1, 8, 2), np.int64), None)]

    wav = R.noise_row(2400, dc=0.2)
    PM.tokenize_audio(Tok(), (wav, 24000))
    assert gen.engine.calls == []
    PM.tokenize_audio(Tok(), (wav, 24000), eq=Eq.rumble(), denoise=True, max_pause_ms=300.0)
    assert gen.engine.calls == [("eq", 24000), "denoise", "pauses"]
    Tok.sample_rate = 16000
    gen.engine.calls.clear()
    PM.tokenize_audio(Tok(), (wav, 16000), eq=Eq.rumble())
    assert gen.engine.calls == [("eq", 16000)]                              # at the tokenizer's rate
    assert "first of all" in PM.tokenize_audio.__doc__.split("eq (")[1].split("denoise (")[0]
    assert PM.equalise(wav[None], Eq.rumble(), 24000).shape == (1, 2400)
