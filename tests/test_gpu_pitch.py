"""GPU: the pitch control (Engine.shift and `pitch=` at the audio end) -- vx_stretch at speed q / p, then vx_resample p -> q.

The shift is compared bit for bit with its numpy composition (tests/_f0_refs.py: the WSOLA restatement of tests/_stretch_refs.py, then
the resampler's fma chain with the geometry and padding of tests/_resample_refs.py on the tap table the device reports -- its libm may
differ from torch's by an ulp, as tests/test_gpu_resample.py records).  That it shifts the pitch by p / q is shown through vx_f0.

Accuracy, measured on the CPU with the numpy composition and the restatement of vx_f0 alone (docs/log_r26.md): five-harmonic tones
of 4800 samples at 24 kHz (150 Hz up 3 semitones = 44/37, 220 Hz down 4 = 177/223, 180 Hz by 3/2, 300 Hz by 2/3), hop 240, window
600, lags 48 .. 400, threshold 0.15: the ratio of the median F0 after and before is off p / q by at most 0.3924 cents (220 Hz);
the test allows twice that."""
from fractions import Fraction

import numpy as np
import pytest

from tests import _f0_refs as R
from vallex_amd._capi import Engine, VallexHipError  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = ((150.0, 3.0, Fraction(44, 37)), (220.0, -4.0, Fraction(177, 223)), (180.0, (3, 2), Fraction(3, 2)), (300.0, Fraction(2, 3), Fraction(2, 3)))
WORST_CENTS = 0.3924                     # of the numpy composition on CASES (measured on the CPU)
F0_OPTS = (24000, 240, 600, 48, 400, 0.15)


@pytest.fixture(scope="module")
def eng():
    e = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)      # created, never finalized
    yield e
    e.close()


@pytest.fixture(scope="module")
def taps(eng):
    """the device's tap table of every ratio the tests use"""
    return {r: eng.dev_resample_taps(r.numerator, r.denominator)[1] for r in [c[2] for c in CASES]}


@pytest.fixture(scope="module")
def ref(taps):
    """per case: the tone, its shift by the numpy composition, and the restatement of vx_f0 on both"""
    out = []
    for fr, pitch, r in CASES:
        x = R.tone(fr, 24000, 4800)
        y = R.shift(x, r.numerator, r.denominator, taps=taps[r])
        out.append((x, y, R.f0(x, F0_OPTS), R.f0(y, F0_OPTS)))
    return out


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    view = {4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize]
    np.testing.assert_array_equal(a.view(view), b.view(view), err_msg=str(what))


def test_shift_equals_the_composition_bit_for_bit(eng, ref, taps):
    for (fr, pitch, r), (x, want, _, _) in zip(CASES, ref):
        assert Engine.pitch_ratio(pitch) == r
        got = eng.shift([x], pitch)
        assert len(got) == 1 and len(got[0]) == len(x) == len(want)      # the duration is kept to the sample
        _same(got[0], want, (fr, r))
        assert not np.array_equal(got[0], x)
    # a ragged list: every row as alone, an empty and a one-sample row included
    r = Fraction(44, 37)
    rows = [ref[0][0], np.zeros(0, np.float32), (R.tone(210.0, 24000, 2477) + 0.2 * R.noise(2477, 3)).astype(np.float32), np.ones(1, np.float32),
            ref[1][0][:999]]
    got = eng.shift(rows, 3.0)
    assert [len(g) for g in got] == [len(x) for x in rows]
    for g, x in zip(got, rows):
        _same(g, R.shift(x, 44, 37, taps=taps[r]), len(x))
    _same(got[0], ref[0][1])
    assert eng.shift([], 3.0) == []


def test_ratio_one_returns_the_input_bits(eng, ref):
    x = ref[0][0]
    hot = x.copy()
    hot[5], hot[77] = np.nan, np.float32(-0.0)
    for pitch in (0.0, (1, 1), Fraction(7, 7), (512, 512)):
        got = eng.shift([x, hot, x[:1]], pitch)
        _same(got[0], x, pitch)
        _same(got[1], hot, pitch)                                      # the bits, a NaN included: nothing ran
        _same(got[2], x[:1], pitch)


def test_the_pitch_moves_by_the_ratio(eng, ref):
    worst = 0.0
    for (fr, pitch, r), (x, y, fx, fy) in zip(CASES, ref):
        got = eng.shift([x], pitch)[0]
        gx, gy = eng.f0([x])[3][0], eng.f0([got])[3][0]
        assert gx == fx[3] and gy == fy[3]                              # the device is the restatement, on both sides
        assert gx["voiced_frames"] >= 17 and gy["voiced_frames"] >= 17
        err = 1200.0 * np.log2(gy["f0_median"] / gx["f0_median"] / float(r))
        print(f"shift accuracy: {fr} Hz by {r}: median {gx['f0_median']:.3f} -> {gy['f0_median']:.3f} Hz, {err:+.4f} cents off the ratio")
        assert abs(err) <= 2.0 * WORST_CENTS, (fr, r, err)
        assert abs(float(R.cents(gx["f0_median"], fr))) <= 1.0
        worst = max(worst, abs(err))
    assert worst >= 0.5 * WORST_CENTS                                  # the constant is the measurement, not a loose guess


def test_speed_and_pitch_are_one_stretch_and_one_resample(eng, ref, taps):
    x = ref[0][0]
    r = Fraction(44, 37)
    for speed, sp in ((1.25, Fraction(5, 4)), ((4, 5), Fraction(4, 5)), (Fraction(3, 2), Fraction(3, 2))):
        comb = sp / r
        st = eng.stretch([x], comb)
        want = eng.resample(st, 44, 37)[0][: -(-len(x) * sp.denominator // sp.numerator)]
        got = eng.shift([x], 3.0, speed)[0]
        _same(got, want, speed)
        assert len(got) == -(-len(x) * sp.denominator // sp.numerator)
        _same(got, R.shift(x, 44, 37, (sp.numerator, sp.denominator), taps=taps[r]), speed)
    _same(eng.shift([x], (1, 1), (4, 5))[0], eng.stretch([x], (4, 5))[0])      # ratio 1 with a speed: the stretch alone


def test_value_errors_come_before_any_launch():
    class NoLaunch(Engine):
        def __init__(self):                                            # no context: any launch would fail on the missing attributes
            pass

        def __del__(self):
            pass
    e = NoLaunch()
    x = np.zeros(100, np.float32)
    for pitch, speed in ((12.5, None), (float("nan"), None), ((3, 1), None), ((1, 3), None), ((513, 512), None), ((3, 0), None),
                         (12.0, 0.9), (-12.0, 1.1), (3.0, 2.5), (3.0, (1, 0)), (1.0, Fraction(997, 1000))):
        with pytest.raises(ValueError):
            e.shift([x], pitch, speed)
        with pytest.raises(ValueError):
            e.vocos_decode([np.zeros((4, 8), np.int64)], 2, pitch=pitch, speed=speed)
        with pytest.raises(ValueError):
            e.encodec_decode([np.zeros((4, 8), np.int64)], pitch=pitch, speed=speed)


def _golden_codes12():
    from tests._util import golden
    codes = golden("nl2_bestof3")["codes"][0].astype(np.int64)
    assert codes.shape == (12, 8)
    return codes


def test_vocos_decode_with_a_pitch_is_the_stages_one_by_one():
    from tests._util import get_model
    from vallex_amd.utils.generation import Finish
    m = get_model(2, 0, 2.5, vocos=True)
    e = m.engine
    codes = [_golden_codes12(), _golden_codes12()[:5]]
    w24 = [w.copy() for w in e.vocos_decode(codes, 2)]
    for a, b in zip(e.vocos_decode(codes, 2, pitch=None), w24):            # the default: the bits of a call without the argument
        _same(a, b)
    fin = Finish(trim=3, keep=40, level_mode=2, level_db=-20.0, fade_in=16, fade_out=16, pcm16=True)
    kw = {k: getattr(fin, k) for k in ("silence_db", "trim", "keep", "level_mode", "level_db", "max_gain_db", "fade_in", "fade_out", "pcm16")}
    sh = e.shift(w24, -2.0)
    assert [len(a) for a in sh] == [3840, 1600]
    r = Engine.pitch_ratio(-2.0)
    tp = e.dev_resample_taps(r.numerator, r.denominator)[1]
    for x, a in zip(w24, sh):
        _same(a, R.shift(x, r.numerator, r.denominator, taps=tp))
    for a, b in zip(e.vocos_decode(codes, 2, pitch=-2.0), sh):             # 24 kHz, no output stage
        _same(a, b)
    want = e.finish(e.resample(sh, 24000, 16000), 160, **kw)[0]            # the rate is a separate resample call behind the shift
    got = e.vocos_decode(codes, 2, pitch=-2.0, sample_rate=16000, finish=fin)
    for a, b in zip(got, want):
        _same(a, b)
        assert a.dtype == np.int16
    sp = Fraction(5, 4)
    want = e.finish(e.resample(e.shift(w24, -2.0, sp), 24000, 16000), 160, **kw)[0]
    for a, b in zip(e.vocos_decode(codes, 2, pitch=-2.0, speed=sp, sample_rate=16000, finish=fin), want):
        _same(a, b)
    for a, b in zip(e.vocos_decode(codes, 2, pitch=(1, 1)), w24):
        _same(a, b)


def test_generate_audio_family_with_a_pitch():
    from oracle import synth
    from vallex_amd.utils import generation as G
    G.preload_models(state_dict=synth.vallex_state_dict(2, 11), vocos_state_dict=synth.vocos_state_dict(2), num_layers=2, max_new=64,
                     max_prompt=128, max_text=64, max_batch=2)
    e = G.model.engine
    ids = synth.synth_text(6, 1)
    us = synth.uniforms(32, 1, 5)[:, 0]
    fin = G.Finish(trim=3, keep=80, level_mode=2, level_db=-20.0, fade_in=32, fade_out=32, pcm16=True)
    kw = {k: getattr(fin, k) for k in ("silence_db", "trim", "keep", "level_mode", "level_db", "max_gain_db", "fade_in", "fade_out", "pcm16")}
    pt = 2.0
    w24 = G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12)
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, pitch=None), w24)
    want24 = e.shift([w24], pt)[0]
    assert len(want24) == len(w24)
    want16 = e.finish(e.resample([want24], 24000, 16000), 160, **kw)[0][0]
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, pitch=pt), want24)
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, pitch=pt, sample_rate=16000, finish=fin), want16)
    _same(G.generate_audio_batch([ids], language="en", uniforms=us[:, None], force_eos_at=12, pitch=pt, sample_rate=16000, finish=fin)[0], want16)
    _same(G.generate_audio_from_long_text([ids], language="en", uniforms=us, force_eos_at=12, pitch=pt, sample_rate=16000, finish=fin), want16)
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, pitch=pt, speed=(5, 4)), e.shift([w24], pt, (5, 4))[0])
    with G.AudioServer(sample_rate=16000, finish=fin, pitch=pt, force_eos_at=12) as srv:
        s16 = srv.submit(ids, language="en", seed=9).result()
    with G.AudioServer(force_eos_at=12) as srv:
        s24 = srv.submit(ids, language="en", seed=9).result()
    _same(s16, e.finish(e.resample(e.shift([s24], pt), 24000, 16000), 160, **kw)[0][0])
    for call in (lambda: G.generate_audio(ids, language="en", pitch=13.0), lambda: G.generate_audio_batch([ids], language="en", pitch=(3, 1)),
                 lambda: G.generate_audio_from_long_text([ids], language="en", pitch=12.0, speed=0.9), lambda: G.AudioServer(pitch=-13)):
        with pytest.raises(ValueError):
            call()
