"""GPU: the spectral noise suppression (vx_denoise, csrc/denoise.hip) against tests/_denoise_refs.py, the numpy restatement of the
header's contract, on the tables the library reports.

Everything is compared word for word: the network on chosen frames (vx_dev_denoise_fft), the powers, the energies, the chosen frames and
the gains (vx_dev_denoise_table), the profiles, the output samples and the infos.  The contract fixes the order of every addition, so
there is no tolerance anywhere.  The division the gain rests on is probed on operands where a reciprocal-multiply would differ from the
correctly rounded quotient.  One un-finalized context serves the kernel tests: the entry needs no weights.  The restatement of every
row is computed once and shared."""
import ctypes as C

import numpy as np
import pytest

from tests import _denoise_refs as R
from vallex_amd import _capi
from vallex_amd._capi import VX_EINVAL, Engine, _ptr

pytestmark = pytest.mark.gpu

SENT_F = np.float32(-1.0e30)
SENT_D = -1.0e300
SENT_I = -123456789
INFO = ("frames", "full_frames", "k", "nonfinite")
STRONG = (7.5, 0.01, 0.5, 0)


@pytest.fixture(scope="module")
def eng():
    e = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)      # created, never finalized
    yield e
    e.close()


@pytest.fixture(scope="module")
def tab():
    return Engine.denoise_tables()


@pytest.fixture(scope="module")
def rows():
    return R.length_rows()


@pytest.fixture(scope="module")
def ref(tab, rows):
    """the restatement of every row of the ragged batch at the defaults"""
    return [R.denoise(x, R.DEFAULTS, tab) for x in rows]


def _opts(o):
    return _capi.vx_denoise_opts(C.sizeof(_capi.vx_denoise_opts), float(o[0]), float(o[1]), float(o[2]), int(o[3]))


def _raw(eng, rows, o, psd=None, pad=5, **kw):
    """vx_denoise on sentinel-filled outputs: (rc, message, out (n, stride + pad), profiles (n, 257), info structs)"""
    n = len(rows)
    ln = np.array([len(r) for r in rows], np.int32)
    ws = max(1, int(ln.max()))
    buf = np.zeros((n, ws), np.float32)
    for i, r in enumerate(rows):
        buf[i, : len(r)] = r
    out = np.full((n, ws + pad), SENT_F, np.float32)
    prof = np.full((n, R.B), SENT_D, np.float64)
    info = (_capi.vx_denoise_info * n)()
    for w in info:
        w.frames = SENT_I
    p = None if psd is None else np.ascontiguousarray(psd, np.float64)
    a = dict(wav=_ptr(buf, C.c_float), wav_stride=ws, lens=_ptr(kw.pop("lens_arr", ln), C.c_int32), batch=n, opts=C.byref(o),
             psd=None if p is None else _ptr(p, C.c_double), out=_ptr(out, C.c_float), out_stride=ws + pad, prof=_ptr(prof, C.c_double), info=info)
    a.update(kw)
    rc = eng.lib.vx_denoise(eng.ctx, a["wav"], a["wav_stride"], a["lens"], a["batch"], a["opts"], a["psd"], a["out"], a["out_stride"], a["prof"],
                            a["info"])
    return rc, eng.lib.vx_last_error(eng.ctx).decode(), out, prof, info


def _check(res, wants, what):
    rc, msg, out, prof, info = res
    assert rc == 0, msg
    for i, want in enumerate(wants):
        L = len(want["out"])
        R.same(out[i, :L], want["out"], (what, "out", i))
        assert (out[i, L:] == SENT_F).all(), (what, "behind the row", i)
        R.same(prof[i], want["psd"], (what, "profile", i))
        assert {k: getattr(info[i], k) for k in INFO} == want["info"], (what, i)


def test_the_network_on_chosen_frames_word_for_word(eng, tab):
    rng = np.random.default_rng(1)
    re, im = np.zeros((9, R.N)), np.zeros((9, R.N))
    for f, n in enumerate((0, R.N - 1, 255, 256)):                    # unit impulses: first, last and the two middle positions
        re[f, n] = 1.0
    im[3, 256] = -1.0
    re[4, :] = 1.0                                                    # a constant frame
    re[5, :], im[5, :] = -0.25, 0.5
    re[6:], im[6:] = rng.normal(size=(3, R.N)), rng.normal(size=(3, R.N))
    re[8] *= 1e-200                                                   # far apart in magnitude: every rounding shows
    for inverse in (False, True):
        gr, gi = eng.dev_denoise_fft(re, im, inverse)
        wr, wi = R.fft(re, im, tab, inverse)
        if inverse:
            wr, wi = wr * (1.0 / R.N), wi * (1.0 / R.N)
        R.same(gr, wr, ("re", inverse))
        R.same(gi, wi, ("im", inverse))
    gr, gi = eng.dev_denoise_fft(re[:1], im[:1])                      # and the network is a transform: an impulse at 0 is all ones
    assert (gr == 1).all() and (gi == 0).all()
    gr, gi = eng.dev_denoise_fft(re[4:5], im[4:5])
    assert gr[0, 0] == R.N and (gr[0, 1:] == 0).all() and (gi == 0).all()
    for bad in (dict(nframes=0), dict(nframes=1025), dict(inverse=2)):
        a = dict(nframes=1, inverse=0)
        a.update(bad)
        o = np.zeros(R.N)
        assert eng.lib.vx_dev_denoise_fft(eng.ctx, _ptr(o, C.c_double), _ptr(o, C.c_double), a["nframes"], a["inverse"], _ptr(o, C.c_double),
                                          _ptr(o, C.c_double)) == VX_EINVAL
        assert next(iter(bad)) in eng.lib.vx_last_error(eng.ctx).decode()


def test_double_division_on_the_device_is_correctly_rounded(eng):
    """operands where a * (1 / b) differs from a / b, the quotients of the gain (x / 5.0, small over large), subnormal results"""
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.random(8192) + 0.5, rng.normal(size=2048) * 10.0 ** rng.integers(-150, 150, 2048), rng.random(1024), [1.0, 2.0, 0.0, 1e-310, 3e-308]])
    b = np.concatenate([rng.random(8192) + 0.5, rng.normal(size=2048) * 10.0 ** rng.integers(-150, 150, 2048), np.full(1024, 5.0), [3.0, 3.0, 7.0, 3.0, 1e10]])
    with np.errstate(under="ignore", over="ignore"):
        want, lazy = a / b, a * (1.0 / b)
    differ = int((want.view(np.uint64) != lazy.view(np.uint64)).sum())
    assert differ > 1000, differ                                     # the operands do tell the two apart
    R.same(eng.dev_denoise_div(a, b), want)


def test_ragged_batch_word_for_word(eng, rows, ref):
    _check(_raw(eng, rows, _opts(R.DEFAULTS)), ref, "batch")
    assert [w["info"]["k"] for w in ref] == [0, 0, 0, 0, 0, 0, 1, 1, 7, 8]           # no full frame, all of them, the kmin quietest
    for i, (x, want) in enumerate(zip(rows, ref)):
        P, E, sel, g = eng.dev_denoise_table(x, _opts(R.DEFAULTS))
        R.same(P, want["P"], ("P", i))
        R.same(E, want["E"], ("E", i))
        assert list(sel) == list(want["sel"]), i
        R.same(g, want["gain"], ("gain", i))


def test_rows_alone_and_in_another_order_give_the_same_bits(eng, rows, ref):
    for i, (x, want) in enumerate(zip(rows, ref)):
        _check(_raw(eng, [x], _opts(R.DEFAULTS)), [want], ("alone", i))
    _check(_raw(eng, rows[::-1], _opts(R.DEFAULTS)), ref[::-1], "reversed")
    order = [9, 0, 5, 8, 1, 7, 2, 6, 3, 4]
    _check(_raw(eng, [rows[i] for i in order], _opts(R.DEFAULTS)), [ref[i] for i in order], "shuffled")


def test_the_smallest_window_gives_the_same_bits(eng, rows, ref):
    eng.dev_denoise_window(_capi.DEV_DENOISE_WINDOW_MIN)
    try:
        _check(_raw(eng, rows + rows, _opts(R.DEFAULTS)), ref + ref, "window")          # 3072 samples a launch: at least five launches
        rc, msg, *_ = _raw(eng, [np.zeros(_capi.DEV_DENOISE_WINDOW_MIN + 1, np.float32)], _opts(R.DEFAULTS))
        assert rc == VX_EINVAL and "lens[0]" in msg and "window" in msg
    finally:
        eng.dev_denoise_window(0)
    for bad in (_capi.DEV_DENOISE_WINDOW_MIN - 1, _capi.DENOISE_WINDOW + 1, -1):
        assert eng.lib.vx_dev_denoise_window(eng.ctx, bad) == VX_EINVAL


def test_other_options_and_a_given_profile(eng, tab, rows, ref):
    x = rows[-1]
    for o in (STRONG, (2.0, 0.5, 0.0, 0), (0.0, 1.0, 1.0, 3)):
        want = R.denoise(x, o, tab)
        _check(_raw(eng, [x], _opts(o)), [want], o)
        P, E, sel, g = eng.dev_denoise_table(x, _opts(o))
        assert list(sel) == list(want["sel"]), o
        R.same(g, want["gain"], ("gain", o))
    psd = ref[-1]["psd"]
    first = _raw(eng, [x], _opts(R.DEFAULTS))
    again = _raw(eng, [x, rows[-2]], _opts(R.DEFAULTS), psd=first[3][0])
    R.same(again[2][0, : len(x)], first[2][0, : len(x)], "a returned profile reproduces the call")
    _check(again, [R.denoise(x, R.DEFAULTS, tab, psd), R.denoise(rows[-2], R.DEFAULTS, tab, psd)], "given")
    P, E, sel, g = eng.dev_denoise_table(rows[-2], _opts(R.DEFAULTS), psd)
    assert len(sel) == 0
    R.same(g, R.denoise(rows[-2], R.DEFAULTS, tab, psd)["gain"], "gain under a given profile")


def test_odd_inputs(eng, tab):
    x = R.odd_row()
    want = R.denoise(x, R.DEFAULTS, tab)
    res = _raw(eng, [x, np.zeros(700, np.float32)], _opts(R.DEFAULTS))
    _check(res, [want, R.denoise(np.zeros(700, np.float32), R.DEFAULTS, tab)], "odd")
    assert res[4][0].nonfinite == 6 and np.isfinite(res[2][0, : len(x)]).all()
    assert (res[2][1, :700] == 0).all() and (res[3][1] == 0).all()


def test_argument_errors(eng, rows):
    x = [rows[-1]]
    good = R.DEFAULTS

    def refused(o=None, field="", **kw):
        oo = _opts(good if o is None else o)
        if "struct_size" in kw:
            oo.struct_size = kw.pop("struct_size")
        rc, msg, out, prof, info = _raw(eng, x, oo, **kw)
        assert rc == VX_EINVAL and field in msg and msg, (o, kw, msg)
        assert (out == SENT_F).all() and (prof == SENT_D).all() and info[0].frames == SENT_I                 # nothing written

    refused(struct_size=C.sizeof(_capi.vx_denoise_opts) - 4, field="struct_size")
    refused(lens_arr=np.array([-1], np.int32), field="lens[0]")
    refused(lens_arr=np.array([len(x[0]) + 1], np.int32), field="lens[0]")
    refused(o=(2.0, 0.0, 0.1, 8), field="floor")
    refused(o=(2.0, 1.5, 0.1, 8), field="floor")
    refused(o=(2.0, float("nan"), 0.1, 8), field="floor")
    refused(o=(-1.0, 0.126, 0.1, 8), field="alpha")
    refused(o=(float("inf"), 0.126, 0.1, 8), field="alpha")
    refused(o=(2.0, 0.126, -0.5, 8), field="frac")
    refused(o=(2.0, 0.126, 1.5, 8), field="frac")
    refused(o=(2.0, 0.126, 0.1, -1), field="kmin")
    refused(batch=0, field="batch")
    refused(out_stride=len(x[0]) - 1, field="out_stride")
    refused(psd=np.full(R.B, -1.0), field="noise_psd")
    refused(psd=np.full(R.B, np.nan), field="noise_psd")
    for name in ("wav", "lens", "opts", "out", "info"):
        refused(field="NULL", **{name: None})
    big = np.zeros(1, np.int32)
    big[0] = _capi.DENOISE_WINDOW + 1                                                      # above the window: refused by the length alone
    rc, msg, *_ = _raw(eng, x, _opts(good), lens_arr=big, wav_stride=_capi.DENOISE_WINDOW + 1, out_stride=_capi.DENOISE_WINDOW + 1)
    assert rc == VX_EINVAL and "window" in msg and "lens[0]" in msg
    with pytest.raises(ValueError, match="denoise"):
        eng.denoise(x, floor_db=3.0)


def test_engine_denoise_and_noise_profile(eng, rows, ref):
    got, infos, profs = eng.denoise(rows, return_profiles=True)
    for i, want in enumerate(ref):
        R.same(got[i], want["out"], i)
        R.same(profs[i], want["psd"], i)
        assert infos[i] == want["info"] and eng.last_denoise_info[i] == want["info"]
    R.same(eng.noise_profile(rows[-1]), ref[-1]["psd"])
    R.same(eng.denoise([rows[-1]], profile=eng.noise_profile(rows[-1]))[0][0], ref[-1]["out"])
    assert eng.denoise([]) == ([], [])


def test_denoise_at_both_audio_ends():
    """tokenize_audio(..., denoise=True) is Engine.denoise followed by the existing path, denoise=None the bits of before; behind the
    vocoder it is Engine.denoise on the decoded waveform, before speed, pitch, resample and finish"""
    from oracle import synth
    from vallex_amd.utils import generation as G
    from vallex_amd.utils import prompt_making as PM
    G.preload_models(state_dict=synth.vallex_state_dict(2, 11), vocos_state_dict=synth.vocos_state_dict(2), num_layers=2, max_new=64,
                     max_prompt=128, max_text=64, max_batch=2)
    e = G.model.engine
    seen = []

    class Tok:
        sample_rate = 24000

        def encode(self, w):
            seen.append(np.array(w))
            return [(np.zeros((1, 8, 1), np.int64), None)]

    rng = np.random.default_rng(12)
    x = np.zeros(9000, np.float32)
    x[3000:6000] = R.vowel(150.0, 600.0, 24000, 3000)
    x = (x + rng.normal(0.0, 0.01, 9000)).astype(np.float32)
    den = e.denoise([x])[0][0]
    custom = G.Denoise(strength_db=6.0, floor_db=-30.0, frac=0.2, kmin=4)
    stored = G.Denoise(profile=e.noise_profile(x))
    PM.tokenize_audio(Tok(), (x[None], 24000))
    PM.tokenize_audio(Tok(), (x[None], 24000), denoise=None)
    PM.tokenize_audio(Tok(), (x[None], 24000), denoise=True)
    PM.tokenize_audio(Tok(), (x[None], 24000), denoise=custom)
    PM.tokenize_audio(Tok(), (x[None], 24000), denoise=stored)
    PM.tokenize_audio(Tok(), (x[None], 24000), denoise=True, trim_db=-40, lufs=-23.0, pitch=2.0)
    R.same(seen[0][0, 0], x)
    R.same(seen[1][0, 0], x)
    R.same(seen[2][0, 0], den)
    R.same(seen[3][0, 0], e.denoise([x], strength_db=6.0, floor_db=-30.0, frac=0.2, kmin=4)[0][0])
    R.same(seen[4][0, 0], den)
    R.same(seen[5][0, 0], PM.level_loudness(PM.trim_silence(PM.shift_pitch(den[None], 2.0), -40), -23.0, 24000)[0])
    assert np.abs(den[:2000].astype(np.float64)).mean() < 0.5 * np.abs(x[:2000].astype(np.float64)).mean()      # the pause got quieter

    ids = synth.synth_text(6, 1)
    us = synth.uniforms(32, 1, 5)[:, 0]
    fin = G.Finish(level_mode=2, level_db=-20.0, fade_in=32, fade_out=32, pcm16=True)
    kw = {k: getattr(fin, k) for k in ("silence_db", "trim", "keep", "level_mode", "level_db", "max_gain_db", "fade_in", "fade_out", "pcm16")}
    w24 = G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12)
    R.same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, denoise=None), w24)
    d24 = e.denoise([w24])[0][0]
    R.same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, denoise=True), d24)
    want16 = e.finish(e.resample(e.shift([d24], 2.0, (5, 4)), 24000, 16000), 160, **kw)[0][0]
    assert want16.dtype == np.int16 and len(want16) > len(w24) // 2 and np.abs(want16).max() > 0
    a = dict(language="en", force_eos_at=12, denoise=True, pitch=2.0, speed=(5, 4), sample_rate=16000, finish=fin)
    R.same(G.generate_audio(ids, uniforms=us, **a), want16)
    R.same(G.generate_audio_batch([ids], uniforms=us[:, None], **a)[0], want16)
    R.same(G.generate_audio_from_long_text([ids], uniforms=us, **a), want16)
    with G.AudioServer(denoise=custom, force_eos_at=12) as srv:
        sd = srv.submit(ids, language="en", seed=9).result()
    with G.AudioServer(force_eos_at=12) as srv:
        s24 = srv.submit(ids, language="en", seed=9).result()
    R.same(sd, e.denoise([s24], strength_db=6.0, floor_db=-30.0, frac=0.2, kmin=4)[0][0])
    for call in (lambda: G.generate_audio(ids, language="en", denoise=1.5), lambda: G.generate_audio_batch([ids], language="en", denoise="on"),
                 lambda: G.AudioServer(denoise=False)):
        with pytest.raises(ValueError):
            call()
