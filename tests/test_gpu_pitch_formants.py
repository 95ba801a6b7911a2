"""GPU: the formant-preserving pitch control -- vx_f0's lags into vx_psola, Engine.shift(..., formants=True), utils.generation.Pitch
and the contour of utils.alignment.range_contour -- against the numpy restatements (tests/_f0_refs.py, tests/_psola_refs.py), bit for
bit, and against what it is for: the pitch moves by the ratio, the formant stays, a glide comes out flat.

Figures of the restatements alone, measured on the CPU (docs/log_r27.md); the tests allow twice each, because the yardstick is itself
a YIN reading with a parabola fit:
- Pitch.  The six vowels of the issue's table (4 000 samples at 8 kHz: f0, F1, ratio below), lags from vx_f0 at hop 80, window 320
  (two periods of lag_max), lags 16 .. 160, threshold 0.15; PSOLA at hop 80, periods 16 .. 160, U 40.  The ratio of the median F0
  after and before is off the ratio by at most 1.3223 cents (100 Hz by 177/223).  With a window of 200 the 120 Hz vowel at ratio 2
  reads an octave low: the synthesis marks are whole samples (33, 34, 33, ...), and only a window of two long periods averages
  that jitter out.
- Contour.  A glide from 100 to 140 Hz (24 000 samples at 24 kHz, F1 700 Hz) through shift(formants=True, range=0): the input's
  segment medians read 107.17, 119.55 and 132.03 Hz, the output's 120.58, 120.47 and 120.41 Hz against the input median of 120.11 Hz:
  at most 6.7538 cents off."""
from fractions import Fraction

import numpy as np
import pytest

from tests import _f0_refs as F
from tests import _psola_refs as R
from vallex_amd import _capi
from vallex_amd._capi import Engine
from vallex_amd.utils.alignment import range_contour
from vallex_amd.utils.generation import Pitch

pytestmark = pytest.mark.gpu

TABLE = ((110.0, 700.0, Fraction(3, 2)), (150.0, 900.0, Fraction(2, 3)), (130.0, 700.0, Fraction(44, 37)), (120.0, 800.0, Fraction(2, 1)),
         (100.0, 700.0, Fraction(177, 223)), (160.0, 1000.0, Fraction(5, 4)))
F8 = (8000, 80, 320, 16, 160, 0.15)
WORST_CENTS = 1.3223                     # of the restatements on TABLE (measured on the CPU)
F24 = (24000, 240, 600, 48, 400, 0.15)   # the defaults of Engine.f0 at 24 kHz, which Engine.shift uses
P24 = (240, 48, 400, 120)                # and those of Engine.psola
GLIDE_CENTS = 6.7538                     # of the restatements on the glide (measured on the CPU)
SEGMENTS = ((5, 33), (36, 64), (67, 95))


@pytest.fixture(scope="module")
def eng():
    e = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)      # created, never finalized
    yield e
    e.close()


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    view = {4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize]
    np.testing.assert_array_equal(a.view(view), b.view(view), err_msg=str(what))


def _f0_opts(o):
    import ctypes as C
    return _capi.vx_f0_opts(C.sizeof(_capi.vx_f0_opts), int(o[0]), int(o[1]), int(o[2]), int(o[3]), int(o[4]), float(o[5]))


def _q16(r):
    return int(round(r * 65536))


def _shift_ref(x, r, scale=None):
    """Engine.shift(formants=True) of one 24 kHz row by the restatements: (out, f0 of the input)"""
    fx = F.f0(x, F24)
    con = None if scale is None else range_contour(fx[0], fx[1], r, scale)
    return R.psola(x, fx[1], P24 + (_q16(r),), con)["out"], fx


def test_the_pitch_moves_by_the_ratio(eng):
    worst = 0.0
    o = _f0_opts(F8)
    for f0, F1, r in TABLE:
        x = R.vowel(f0, F1, 8000, 4000)
        fx = F.f0(x, F8)
        want = R.psola(x, fx[1], R.SMALL + (_q16(r),))
        fy = F.f0(want["out"], F8)
        gf, glag, _, ginfo = eng.f0_lags([x], o)
        _same(glag[0], fx[1], (f0, "lags"))
        rows, infos = eng.psola([x], glag, 80, r, period_min=16, period_max=160, unvoiced_period=40)
        _same(rows[0], want["out"], (f0, r))
        assert infos[0] == want["info"]
        gy = eng.f0_lags(rows, o)[3][0]
        assert ginfo[0] == fx[3] and gy == fy[3]                              # the device is the restatement, on both sides
        assert ginfo[0]["voiced_frames"] >= 45 and gy["voiced_frames"] >= 43
        err = 1200.0 * np.log2(gy["f0_median"] / ginfo[0]["f0_median"] / float(r))
        print(f"psola accuracy: {f0} Hz by {r}: median {ginfo[0]['f0_median']:.3f} -> {gy['f0_median']:.3f} Hz, {err:+.4f} cents off the ratio")
        assert abs(err) <= 2.0 * WORST_CENTS, (f0, r, err)
        worst = max(worst, abs(err))
    assert worst >= 0.5 * WORST_CENTS                                         # the constant is the measurement, not a loose guess


def test_the_formant_stays_where_the_plain_shift_moves_it(eng):
    for f0, F1, r in (TABLE[0], TABLE[1], TABLE[3]):
        x = R.vowel(f0, F1, 24000, 12000)
        want, _ = _shift_ref(x, r)
        got = eng.shift([x], r, formants=True)[0]
        _same(got, want, (f0, r))
        assert len(got) == len(x)
        spacing = f0 * float(r)
        peak = R.strongest_harmonic(got, 24000, spacing)
        print(f"formants: {f0} Hz by {r}, F1 {F1}: strongest harmonic {R.strongest_harmonic(x, 24000, f0):.0f} -> {peak:.0f} Hz")
        assert abs(peak - F1) <= spacing, (f0, r, peak)
        assert abs(F1 * float(r) - F1) > spacing                              # which excludes the formant the plain shift gives
    # a ragged list with an empty and a one-sample row, through the Pitch object too; ratio 1 copies the bits, a NaN included
    x = R.vowel(110.0, 700.0, 24000, 12000)
    rows = [x, np.zeros(0, np.float32), np.ones(1, np.float32), x[:2477]]
    got = eng.shift(rows, Pitch((3, 2)))
    assert [len(g) for g in got] == [len(v) for v in rows]
    for g, v in zip(got, rows):
        _same(g, _shift_ref(v, Fraction(3, 2))[0], len(v))
    hot = x.copy()
    hot[5] = np.nan
    _same(eng.shift([hot], Pitch(0.0))[0], hot)
    _same(eng.shift([hot], (1, 1), formants=True)[0], hot)
    assert eng.shift([], 3.0, formants=True) == []


def test_a_glide_comes_out_flat(eng):
    x = R.glide(100.0, 140.0, 700.0, 24000, 24000)
    want, fx = _shift_ref(x, Fraction(1), 0.0)
    got = eng.shift([x], Pitch(0.0, range=0.0))[0]
    _same(got, want)
    _same(eng.shift([x], 0.0, formants=True, range=0.0)[0], want)
    f, lag, _, info = eng.f0_lags([got], _f0_opts(F24))
    med = fx[3]["f0_median"]
    worst, spread_in = 0.0, []
    for a, b in SEGMENTS:
        v = np.sort(f[0][a:b][lag[0][a:b] > 0])
        vi = np.sort(fx[0][a:b][fx[1][a:b] > 0])
        assert len(v) >= 20 and len(vi) >= 20
        c = float(R.cents(v[(len(v) - 1) // 2], med))
        spread_in.append(float(R.cents(vi[(len(vi) - 1) // 2], med)))
        print(f"contour: frames {a} .. {b}: {vi[(len(vi) - 1) // 2]:.2f} -> {v[(len(v) - 1) // 2]:.2f} Hz, {c:+.4f} cents off the median {med:.2f}")
        assert abs(c) <= 2.0 * GLIDE_CENTS, (a, b, c)
        worst = max(worst, abs(c))
    assert worst >= 0.5 * GLIDE_CENTS and spread_in[0] < -150.0 and spread_in[2] > 150.0      # the input did glide
    wide = eng.shift([x], Pitch(0.0, range=1.5))[0]                             # a wider range: the restatement again
    _same(wide, _shift_ref(x, Fraction(1), 1.5)[0])


def _golden_codes12():
    from tests._util import golden
    codes = golden("nl2_bestof3")["codes"][0].astype(np.int64)
    assert codes.shape == (12, 8)
    return codes


def test_vocos_decode_with_a_pitch_object_is_the_stages_one_by_one():
    from tests._util import get_model
    from vallex_amd.utils.generation import Finish
    m = get_model(2, 0, 2.5, vocos=True)
    e = m.engine
    codes = [_golden_codes12(), _golden_codes12()[:5]]
    w24 = [w.copy() for w in e.vocos_decode(codes, 2)]
    fin = Finish(trim=3, keep=40, level_mode=2, level_db=-20.0, fade_in=16, fade_out=16, pcm16=True)
    kw = {k: getattr(fin, k) for k in ("silence_db", "trim", "keep", "level_mode", "level_db", "max_gain_db", "fade_in", "fade_out", "pcm16")}
    # the steps one by one: the pitch tracker, the PSOLA shift, the rate, the output stage
    o = e._f0_opts(24000, None, None, 60.0, 500.0, 0.15)
    lag = e.f0_lags(w24, o)[1]
    r = Engine.pitch_ratio(-2.0)
    sh = e.psola(w24, lag, 240, r)[0]
    assert [len(a) for a in sh] == [3840, 1600]
    for a, b in zip(e.vocos_decode(codes, 2, pitch=Pitch(-2.0)), sh):
        _same(a, b)
    want = e.finish(e.resample(sh, 24000, 16000), 160, **kw)[0]
    got = e.vocos_decode(codes, 2, pitch=Pitch(-2.0, formants=True), sample_rate=16000, finish=fin)
    for a, b in zip(got, want):
        _same(a, b)
        assert a.dtype == np.int16
    # with a speed: the stretch at the speed alone first
    sp = Fraction(5, 4)
    st = e.stretch(w24, sp)
    want = e.finish(e.resample(e.psola(st, e.f0_lags(st, o)[1], 240, r)[0], 24000, 16000), 160, **kw)[0]
    for a, b in zip(e.vocos_decode(codes, 2, pitch=Pitch(-2.0), speed=sp, sample_rate=16000, finish=fin), want):
        _same(a, b)
    # the defaults: formants=False, a plain number and None are the calls of before -- one stretch and one resample, or nothing
    p3 = Engine.pitch_ratio(3.0)
    old = [y[: len(x)] for x, y in zip(w24, e.resample(e.stretch(w24, 1 / p3), p3.numerator, p3.denominator))]
    for call in (lambda: e.vocos_decode(codes, 2, pitch=3.0), lambda: e.vocos_decode(codes, 2, pitch=Pitch(3.0, formants=False)),
                 lambda: e.shift(w24, 3.0), lambda: e.shift(w24, 3.0, formants=False), lambda: e.shift(w24, p3)):
        for a, b in zip(call(), old):
            _same(a, b)
    for a, b in zip(e.vocos_decode(codes, 2, pitch=None), w24):
        _same(a, b)
    for a, b in zip(e.vocos_decode(codes, 2, pitch=Pitch((1, 1))), w24):
        _same(a, b)
    with pytest.raises(ValueError):
        e.vocos_decode(codes, 2, pitch=Pitch((3, 2), formants=False), speed=(1, 2))      # the stretch would run at 1/3: refused before the vocoder


def test_generate_audio_family_with_a_pitch_object():
    from oracle import synth
    from vallex_amd.utils import generation as G
    G.preload_models(state_dict=synth.vallex_state_dict(2, 11), vocos_state_dict=synth.vocos_state_dict(2), num_layers=2, max_new=64,
                     max_prompt=128, max_text=64, max_batch=2)
    e = G.model.engine
    ids = synth.synth_text(6, 1)
    us = synth.uniforms(32, 1, 5)[:, 0]
    fin = G.Finish(trim=3, keep=80, level_mode=2, level_db=-20.0, fade_in=32, fade_out=32, pcm16=True)
    kw = {k: getattr(fin, k) for k in ("silence_db", "trim", "keep", "level_mode", "level_db", "max_gain_db", "fade_in", "fade_out", "pcm16")}
    pt = G.Pitch(2.0, range=0.5)
    w24 = G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12)
    want24 = e.shift([w24], 2.0, formants=True, range=0.5)[0]
    assert len(want24) == len(w24)
    want16 = e.finish(e.resample([want24], 24000, 16000), 160, **kw)[0][0]
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, pitch=pt), want24)
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, pitch=pt, sample_rate=16000, finish=fin), want16)
    _same(G.generate_audio_batch([ids], language="en", uniforms=us[:, None], force_eos_at=12, pitch=pt, sample_rate=16000, finish=fin)[0], want16)
    _same(G.generate_audio_from_long_text([ids], language="en", uniforms=us, force_eos_at=12, pitch=pt, sample_rate=16000, finish=fin), want16)
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, pitch=G.Pitch(2.0), speed=(5, 4)),
          e.shift([w24], 2.0, (5, 4), formants=True)[0])
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, pitch=G.Pitch(2.0, formants=False)), e.shift([w24], 2.0)[0])
    with G.AudioServer(sample_rate=16000, finish=fin, pitch=pt, force_eos_at=12) as srv:
        s16 = srv.submit(ids, language="en", seed=9).result()
    with G.AudioServer(force_eos_at=12) as srv:
        s24 = srv.submit(ids, language="en", seed=9).result()
    _same(s16, e.finish(e.resample(e.shift([s24], pt), 24000, 16000), 160, **kw)[0][0])
    for call in (lambda: G.generate_audio(ids, language="en", pitch=3.0, speed=(1, 0)), lambda: G.Pitch((1, 2)),
                 lambda: G.AudioServer(pitch=G.Pitch(3.0), speed=3.0)):
        with pytest.raises(ValueError):
            call()
