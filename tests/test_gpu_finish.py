"""GPU: the output stage (vx_finish, csrc/finish.hip) against tests/_finish_refs.py, the numpy restatement of the header's contract.

Everything is compared word for word: frame tables (the doubles included), spans, counts, peaks, mean squares, fp32 and int16 outputs.
The one exception is the gain, which goes through pow on the host: it is held to 1 fp32 ulp, and the outputs are compared with the
restatement applied at the gain the call REPORTED.  Every frame of every input of a decision-dependent test is at least a quarter of
an octave away from the silence threshold (asserted on the reference), so a last bit of pow cannot flip a frame.  One un-finalized
context serves the kernel tests: the entry needs no weights."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from tests import _finish_refs as R
from vallex_amd import _capi
from vallex_amd._capi import VX_EINVAL, Engine, VallexHipError, _ptr

pytestmark = pytest.mark.gpu

DB = -40.0
LONG = 20000                # a fade longer than every row


@pytest.fixture(scope="module")
def eng():
    e = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)      # created, never finalized
    yield e
    e.close()


@pytest.fixture(scope="module")
def data():
    """per frame size: the eight rows, one more with a NaN, +Inf, -Inf and -0.0 in it, and the frame table of each -- computed once"""
    d = {}
    for F in R.FRAMES:
        rows = R.rows(F)
        odd = rows[6].copy()
        odd[5], odd[F + 1], odd[F + 2], odd[2 * F], odd[4800] = np.nan, np.inf, -np.inf, np.float32(-0.0), np.nan
        rows.append(odd)
        worst = min(R.margin(x, F, DB) for x in rows)
        print(f"frame {F}: worst |log2(e / (thr2 n))| over the inputs = {worst:.2f}")
        assert worst >= 0.25
        d[F] = (rows, [R.frames(x, F) for x in rows])
    return d


def _opts(F, **kw):
    o = dict(R.DEFAULTS, **kw)
    return _capi.vx_finish_opts(C.sizeof(_capi.vx_finish_opts), F, o["silence_db"], o["trim"], o["keep"], o["level_mode"], o["level_db"],
                                o["max_gain_db"], o["fade_in"], o["fade_out"], _capi.PCM_S16 if o["pcm16"] else _capi.PCM_F32)


def _raw(eng, rows, F, out=True, pad=5, **kw):
    """vx_finish on a sentinel-filled out: (rc, message, out (n, stride + pad), out_lens, infos)"""
    n = len(rows)
    ln = np.array([len(r) for r in rows], np.int32)
    ws = max(1, int(ln.max()))
    buf = np.zeros((n, ws), np.float32)
    for i, r in enumerate(rows):
        buf[i, : len(r)] = r
    pcm16 = kw.get("pcm16", False)
    outa = np.full((n, ws + pad), R.SENT_H if pcm16 else R.SENT_F, np.int16 if pcm16 else np.float32)
    ol = np.full(n, -7, np.int32)
    info = (_capi.vx_wave_info * n)()
    o = _opts(F, **kw)
    rc = eng.lib.vx_finish(eng.ctx, _ptr(buf, C.c_float), ws, _ptr(ln, C.c_int32), n, C.byref(o),
                           outa.ctypes.data_as(C.c_void_p) if out else None, ws + pad, _ptr(ol, C.c_int32), info)
    infos = [{f[0]: getattr(w, f[0]) for f in _capi.vx_wave_info._fields_} for w in info]
    return rc, eng.lib.vx_last_error(eng.ctx).decode(), outa, ol, infos


def _same_info(got, want, what):
    for k in ("begin", "end", "active_frames", "nonfinite", "clipped"):
        assert got[k] == want[k], (what, k, got, want)
    assert np.float32(got["peak"]).view(np.uint32) == np.float32(want["peak"]).view(np.uint32), (what, got, want)
    assert np.float64(got["mean_square"]).view(np.uint64) == np.float64(want["mean_square"]).view(np.uint64), (what, got, want)
    assert R.ulp_diff([got["gain"]], [want["gain"]])[0] <= 1, (what, got, want)


def _bits(a):
    return a.view(np.uint16 if a.dtype == np.int16 else np.uint32)


@pytest.mark.parametrize("F", R.FRAMES)
def test_frames_word_for_word(eng, data, F):
    rows, tables = data[F]
    for x, (e, p, z) in zip(rows, tables):
        ge, gp, gz = eng.dev_finish_frames(x, F)
        assert ge.shape == e.shape and gp.shape == p.shape
        np.testing.assert_array_equal(ge.view(np.uint64), e.view(np.uint64), err_msg=f"row of {len(x)}")       # the doubles
        np.testing.assert_array_equal(gp.view(np.uint32), p.view(np.uint32))
        np.testing.assert_array_equal(gz, z)
    assert tables[-1][2].sum() == 4 and tables[-1][2][-1] == 1          # the non-finite samples were counted, the cut last frame too


@pytest.mark.parametrize("F", R.FRAMES)
def test_measure_alone_and_as_one_ragged_batch(eng, data, F):
    """a frame's bits do not depend on its launch: the infos of the rows as one batch and of every row alone are the restatement's,
    with and without an output"""
    rows, tables = data[F]
    kw = dict(silence_db=DB, trim=3, keep=5, level_mode=R.RMS, level_db=-20.0)
    want = [R.measure(x, F, table=t, **kw) for x, t in zip(rows, tables)]
    rc, msg, _, ol, infos = _raw(eng, rows, F, out=False, **kw)
    assert rc == 0, msg
    assert ol.tolist() == [w["end"] - w["begin"] for w in want]          # out_lens is written when given, with or without out
    for i, (g, w) in enumerate(zip(infos, want)):
        _same_info(g, w, f"batch row {i}")
        rc, msg, _, _, one = _raw(eng, [rows[i]], F, out=False, **kw)
        assert rc == 0, msg
        _same_info(one[0], w, f"row {i} alone")
        assert one[0]["gain"] == g["gain"]
    assert want[0]["active_frames"] == 0 and want[-1]["nonfinite"] == 4 and want[-2]["gain"] != 1
    # Engine.measure: the active span, nothing applied
    for g, x, t in zip(eng.measure(rows, F, DB), rows, tables):
        _same_info(g, R.measure(x, F, silence_db=DB, trim=3, table=t), "Engine.measure")


COMBOS = [dict(trim=t, level_mode=m, fade_in=a, fade_out=b)
          for t, m, (a, b) in itertools.product((0, 1, 2, 3), (0, 1, 2), ((0, 0), (7, 7), (LONG, LONG), (7, LONG)))]


@pytest.mark.parametrize("pcm16", [False, True])
@pytest.mark.parametrize("F", R.FRAMES)
def test_apply_word_for_word(eng, data, F, pcm16):
    """every trim x level x fade combination on the ragged batch: out equals the restatement at the reported gain, `clipped` and the
    rest of the info are exact, nothing is written behind out_lens[b]"""
    rows, tables = data[F]
    sent = R.SENT_H if pcm16 else R.SENT_F
    nclip = 0
    for c in COMBOS:
        kw = dict(c, silence_db=DB, keep=3, level_db=-3.0 if c["level_mode"] == R.PEAK else -1.0, max_gain_db=20.0, pcm16=pcm16)
        rc, msg, out, ol, infos = _raw(eng, rows, F, **kw)
        assert rc == 0, msg
        for b, (x, t, g) in enumerate(zip(rows, tables, infos)):
            w = R.measure(x, F, table=t, **kw)
            assert R.ulp_diff([g["gain"]], [w["gain"]])[0] <= 1, (c, b)
            want, w["clipped"] = R.apply(x, w["begin"], w["end"], g["gain"], c["fade_in"], c["fade_out"], pcm16)
            _same_info(g, w, (c, b))
            assert ol[b] == len(want) == w["end"] - w["begin"]
            np.testing.assert_array_equal(_bits(out[b, : ol[b]]), _bits(want), err_msg=f"{c}, row {b}")
            assert (out[b, ol[b]:] == sent).all(), (c, b)
            nclip += w["clipped"]
    assert (out[0] == sent).all()                                        # the zero-length row wrote nothing
    print(f"frame {F}, {'s16' if pcm16 else 'f32'}: {len(COMBOS)} combinations x {len(rows)} rows, {nclip} clipped samples in all")


@pytest.mark.parametrize("F", R.FRAMES)
def test_clipped_is_exact_on_a_hot_row(eng, data, F):
    """a row driven 6 dB over full scale, and a quiet one pushed over it by the RMS level"""
    rows, _ = data[F]
    hot = (rows[7] * np.float32(8.0)).astype(np.float32)                 # the 0.25 tone at 2.0: 6 dB over
    assert R.margin(hot, F, DB) >= 0.25
    for pcm16 in (False, True):
        for x, kw in ((hot, dict(fade_in=7)), (rows[7], dict(level_mode=R.RMS, level_db=-1.0, trim=3))):
            rc, msg, out, ol, infos = _raw(eng, [x], F, silence_db=DB, pcm16=pcm16, **kw)
            assert rc == 0, msg
            want, w = R.finish(x, F, gain_used=infos[0]["gain"], silence_db=DB, pcm16=pcm16, **kw)
            assert w["clipped"] > 100 and infos[0]["clipped"] == w["clipped"]
            np.testing.assert_array_equal(_bits(out[0, : ol[0]]), _bits(want))
            if pcm16:
                assert out[0, : ol[0]].max() == 32767 and out[0, : ol[0]].min() == -32768


def test_s16_rule_on_the_device(eng):
    """the half-way cases and the clamp of tests/test_finish_refs.py, through the kernel"""
    v = np.float32([0.5 / 32768, -0.5 / 32768, 1.5 / 32768, 2.5 / 32768, 1.0, 0.99999, -1.0, -1.00002, 0.5, np.nan, np.inf, -np.inf] + [0.25] * 20)
    rc, msg, out, ol, infos = _raw(eng, [v], 16, pcm16=True)
    assert rc == 0 and ol[0] == 32, msg
    assert out[0, :12].tolist() == [0, 0, 2, 2, 32767, 32767, -32768, -32768, 16384, 0, 0, 0]
    assert infos[0]["clipped"] == 3 and infos[0]["nonfinite"] == 3
    rc, msg, out, ol, infos = _raw(eng, [v], 16)
    assert rc == 0 and infos[0]["clipped"] == 1 and np.isfinite(out[0, :32]).all() and out[0, 9:12].tolist() == [0, 0, 0]


def test_sentinels_silence_and_repeat(eng, data):
    F = 240
    rows, tables = data[F]
    silent = (1e-4 * np.random.default_rng(5).standard_normal(1000)).astype(np.float32)
    assert R.margin(silent, F, DB) >= 0.25
    batch = [rows[7], np.zeros(0, np.float32), silent, rows[5]]
    for pcm16 in (False, True):
        sent = R.SENT_H if pcm16 else R.SENT_F
        kw = dict(silence_db=DB, trim=3, keep=10, level_mode=R.PEAK, fade_in=7, fade_out=LONG, pcm16=pcm16)
        rc, msg, out, ol, infos = _raw(eng, batch, F, **kw)
        assert rc == 0, msg
        assert ol[1] == 0 and ol[2] == 0 and (out[1] == sent).all() and (out[2] == sent).all()     # nothing kept, nothing written
        assert infos[2]["active_frames"] == 0 and infos[2]["gain"] == 1 and (infos[2]["begin"], infos[2]["end"]) == (0, 0)
        for b in (0, 3):
            assert 0 < ol[b] < len(batch[b]) and (out[b, ol[b]:] == sent).all()
        rc2, _, out2, ol2, infos2 = _raw(eng, batch, F, **kw)
        assert rc2 == 0 and infos2 == infos and ol2.tolist() == ol.tolist()
        np.testing.assert_array_equal(_bits(out), _bits(out2))                                     # two calls, the same bits
        got, ginfo = eng.finish(batch, F, **kw)
        assert ginfo == infos and [len(g) for g in got] == ol.tolist() and got[0].dtype == out.dtype
        for b, g in enumerate(got):
            np.testing.assert_array_equal(g, out[b, : ol[b]])
        # an untrimmed call keeps an all-silent row as it is, at gain 1
        rc, msg, out, ol, infos = _raw(eng, [silent], F, silence_db=DB, level_mode=R.RMS, pcm16=pcm16)
        assert rc == 0 and ol[0] == 1000 and infos[0]["gain"] == 1 and infos[0]["mean_square"] == 0
        np.testing.assert_array_equal(_bits(out[0, :1000]), _bits(R.apply(silent, 0, 1000, 1.0, pcm16=pcm16)[0]))
    assert eng.finish([], F) == ([], [])


def test_windows_are_bit_identical(eng, data):
    """512 and 777 input samples per launch: the 4801 and 13 001 rows go through many windows of both passes and give the words of
    the default single pass; 0 restores the default; values out of range are refused"""
    assert _capi.DEV_FINISH_WINDOW_MIN == 512 and _capi.FINISH_WINDOW == 1 << 23
    kws = [dict(silence_db=DB, trim=3, keep=33, level_mode=R.RMS, level_db=-12.0, fade_in=7, fade_out=LONG, pcm16=p) for p in (False, True)]
    kws.append(dict(silence_db=DB, level_mode=R.PEAK, fade_in=LONG))
    eng.dev_finish_window(0)
    ref = {}
    for F in R.FRAMES:
        rows = [data[F][0][i] for i in (6, 7, 8)]
        ref[F] = [_raw(eng, rows, F, **kw)[2:] for kw in kws], [eng.dev_finish_frames(x, F) for x in rows]
    try:
        for win in (_capi.DEV_FINISH_WINDOW_MIN, 777):
            eng.dev_finish_window(win)
            for F in R.FRAMES:
                rows = [data[F][0][i] for i in (6, 7, 8)]
                for kw, (out, ol, infos) in zip(kws, ref[F][0]):
                    rc, msg, out2, ol2, infos2 = _raw(eng, rows, F, **kw)
                    assert rc == 0, msg
                    assert infos2 == infos and ol2.tolist() == ol.tolist(), (win, F)
                    np.testing.assert_array_equal(_bits(out2), _bits(out), err_msg=f"window {win}, frame {F}")
                for x, (e, p, z) in zip(rows, ref[F][1]):
                    e2, p2, z2 = eng.dev_finish_frames(x, F)
                    np.testing.assert_array_equal(e2.view(np.uint64), e.view(np.uint64))
                    np.testing.assert_array_equal(p2.view(np.uint32), p.view(np.uint32))
                    np.testing.assert_array_equal(z2, z)
        # a frame above the window: the launch holds one frame
        eng.dev_finish_window(512)
        x = data[441][0][7]
        e, p, z = R.frames(x, 4096)
        e2, p2, z2 = eng.dev_finish_frames(x, 4096)
        np.testing.assert_array_equal(e2.view(np.uint64), e.view(np.uint64))
        for bad in (1, _capi.DEV_FINISH_WINDOW_MIN - 1, -5, _capi.FINISH_WINDOW + 1):
            with pytest.raises(VallexHipError) as ei:
                eng.dev_finish_window(bad)
            assert ei.value.code == VX_EINVAL and "input_samples" in str(ei.value)
    finally:
        eng.dev_finish_window(0)
    F = 240
    out, ol, infos = ref[F][0][0]
    rc, _, out2, ol2, infos2 = _raw(eng, [data[F][0][i] for i in (6, 7, 8)], F, **kws[0])
    assert rc == 0 and infos2 == infos
    np.testing.assert_array_equal(_bits(out2), _bits(out))


def _golden_codes12():
    from tests._util import golden
    codes = golden("nl2_bestof3")["codes"][0].astype(np.int64)
    assert codes.shape == (12, 8)
    return codes


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    np.testing.assert_array_equal(_bits(np.ascontiguousarray(a)), _bits(np.ascontiguousarray(b)))


def test_vocos_decode_with_an_output_stage():
    from tests._util import get_model
    from vallex_amd.utils.generation import Finish
    m = get_model(2, 0, 2.5, vocos=True)
    e = m.engine
    codes = [_golden_codes12(), _golden_codes12()[:5]]
    w24 = [w.copy() for w in e.vocos_decode(codes, 2)]
    buf = np.zeros((2, 12, 8), np.int64)
    buf[0], buf[1, :5] = codes[0], codes[1]
    lens = np.array([12, 5], np.int32)
    audio = np.zeros((2, 12 * 320), np.float32)
    assert e.lib.vx_vocos_decode(e.ctx, _ptr(buf, C.c_int64), 12, _ptr(lens, C.c_int32), 2, 2, _ptr(audio, C.c_float), 12 * 320) == 0
    for a, b in zip(e.vocos_decode(codes, 2, finish=None), (audio[0], audio[1, : 5 * 320])):      # without the argument: a plain call
        _same(a, b)
    w16 = e.resample(w24, 24000, 16000)
    for fin in (Finish(trim=3, keep=40, level_mode=2, level_db=-20.0, fade_in=16, fade_out=16, pcm16=True),
                Finish(silence_db=-60.0, level_mode=1, fade_out=5000), Finish(frame=64, trim=1)):
        frame = fin.frame or 160
        want, winfo = e.finish(w16, frame, fin.silence_db, fin.trim, fin.keep, fin.level_mode, fin.level_db, fin.max_gain_db, fin.fade_in,
                               fin.fade_out, fin.pcm16)
        got = e.vocos_decode(codes, 2, sample_rate=16000, finish=fin)
        assert e.last_finish_info == winfo
        for a, b in zip(got, want):
            _same(a, b)
            assert a.dtype == (np.int16 if fin.pcm16 else np.float32)
        # ... and the device's words are the restatement's (where no frame of the vocoder's output is near the threshold)
        for x, a, i in zip(w16, got, winfo):
            if R.margin(x, frame, fin.silence_db) >= 0.25:
                _same(a, R.finish(x, frame, gain_used=i["gain"], **{k: getattr(fin, k) for k in R.DEFAULTS})[0])
    fin = Finish(level_mode=1, pcm16=True)
    for a, b in zip(e.vocos_decode(codes, 2, finish=fin), e.finish(w24, 240, level_mode=1, pcm16=True)[0]):       # at 24 kHz: frame 240
        _same(a, b)


def test_encodec_decode_with_an_output_stage():
    from oracle.encodec_oracle import encodec_encoder_state_dict, encodec_state_dict
    from tests._util import get_model
    from vallex_amd.utils.generation import Finish
    m = get_model(2, 0, 2.5, max_new=64, max_batch=4)
    sd = dict(encodec_state_dict(3))
    sd.update(encodec_encoder_state_dict(4))
    m.load_encodec_state_dict(sd)
    e = m.engine
    codes = [_golden_codes12()]
    fin = Finish(level_mode=2, level_db=-18.0, fade_in=100, fade_out=100, pcm16=True)
    kw = {k: getattr(fin, k) for k in R.DEFAULTS}
    w24 = e.encodec_decode(codes)
    _same(e.encodec_decode(codes, finish=None)[0], w24[0])
    _same(e.encodec_decode(codes, finish=fin)[0], e.finish(w24, 240, **kw)[0][0])
    _same(e.encodec_decode(codes, sample_rate=48000, finish=fin)[0], e.finish(e.resample(w24, 24000, 48000), 480, **kw)[0][0])


def test_generate_audio_and_the_enrolment_trim():
    from oracle import synth
    from vallex_amd.utils import generation as G
    from vallex_amd.utils import prompt_making as PM
    G.preload_models(state_dict=synth.vallex_state_dict(2, 11), vocos_state_dict=synth.vocos_state_dict(2), num_layers=2, max_new=64,
                     max_prompt=128, max_text=64, max_batch=2)
    e = G.model.engine
    ids = synth.synth_text(6, 1)
    us = synth.uniforms(32, 1, 5)[:, 0]
    fin = G.Finish(trim=3, keep=80, level_mode=2, level_db=-20.0, fade_in=32, fade_out=32, pcm16=True)
    kw = {k: getattr(fin, k) for k in R.DEFAULTS}
    w24 = G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12)
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, finish=None), w24)
    w16 = e.resample([w24], 24000, 16000)[0]
    want16 = e.finish([w16], 160, **kw)[0][0]
    want24 = e.finish([w24], 240, **kw)[0][0]
    assert want16.dtype == np.int16 and want24.dtype == np.int16
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, sample_rate=16000, finish=fin), want16)
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, finish=fin), want24)
    f32 = G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, finish=G.Finish(level_mode=1))
    i = e.last_finish_info[0]
    assert f32.dtype == np.float32 and len(f32) == len(w24) and np.abs(f32).max() == np.float32(i["peak"]) * np.float32(i["gain"])
    _same(G.generate_audio_batch([ids], language="en", uniforms=us[:, None], force_eos_at=12, sample_rate=16000, finish=fin)[0], want16)
    _same(G.generate_audio_from_long_text([ids], language="en", uniforms=us, force_eos_at=12, sample_rate=16000, finish=fin), want16)
    with G.AudioServer(sample_rate=16000, finish=fin, force_eos_at=12) as srv:
        s16 = srv.submit(ids, language="en", seed=9).result()
    with G.AudioServer(force_eos_at=12) as srv:
        s24 = srv.submit(ids, language="en", seed=9).result()
    assert s24.dtype == np.float32
    _same(s16, e.finish(e.resample([s24], 24000, 16000), 160, **kw)[0][0])

    # tokenize_audio(..., trim_db=-40) hands the tokenizer the clip without its leading and trailing silence
    seen = []

    class Tok:
        sample_rate = 24000

        def encode(self, w):
            seen.append(np.array(w))
            return [(np.zeros((1, 8, 1), np.int64), None)]

    x = R.row(9000, 240, 3000, 2700, np.random.default_rng(7))
    assert R.margin(x, 240, -40.0) >= 0.25
    i = R.measure(x, 240, silence_db=-40.0, trim=3, keep=2400)
    assert (i["begin"], i["end"]) == (480, 8880)
    PM.tokenize_audio(Tok(), (x[None], 24000), trim_db=-40)
    PM.tokenize_audio(Tok(), (x[None], 24000))
    assert seen[0].shape == (1, 1, 8400) and seen[1].shape == (1, 1, 9000)
    _same(seen[0][0, 0], x[480:8880])                                  # level and format untouched
    _same(seen[1][0, 0], x)
    with pytest.raises(ValueError, match="silent"):
        PM.tokenize_audio(Tok(), ((1e-4 * x[None, :2400] / np.abs(x[:2400]).max()).astype(np.float32), 24000), trim_db=-40)


def test_nothing_else_moves():
    """greedy ids of nl2_greedy_eos before and after interleaved finish calls; a finish call while a serving session is open succeeds
    and the session's result is what it is without the call; no fallback is counted"""
    from tests._util import case_row, get_model, golden
    c, row, _ = case_row("nl2_greedy_eos")
    m = get_model(c["num_layers"], c["seed"], c["eos_gain"], vocos=True)
    e = m.engine
    x = R.rows(240)[7]
    kw = dict(silence_db=DB, trim=3, level_mode=2, fade_in=7, fade_out=7, pcm16=True)
    before = m.inference_batch([row], top_k=1, force_eos_at=c["force_eos_at"])[0]
    r1 = e.finish([x], 240, **kw)[0][0].copy()
    after = m.inference_batch([row], top_k=1, force_eos_at=c["force_eos_at"])[0]
    np.testing.assert_array_equal(before, golden("nl2_greedy_eos")["codes"][0])
    np.testing.assert_array_equal(after, before)
    fb = e.last_fallbacks()
    e.finish([x], 240, level_mode=1)
    e.measure([x], 240)
    assert e.last_fallbacks() == fb
    _same(r1, R.finish(x, 240, gain_used=e.finish([x], 240, **kw)[1][0]["gain"], **kw)[0])

    def session(interleave):
        got = {}
        with e.serve(top_k=10, force_eos_at=30) as sess:
            ids = sess.submit(m.make_batch([row, row]), [dict(seed=5), dict(seed=6, best_of=2)])
            sess.run(3, lambda rid, cd: got.__setitem__(rid, cd))
            if interleave:
                _same(e.finish([x], 240, **kw)[0][0], r1)
            sess.run(0, lambda rid, cd: got.__setitem__(rid, cd))
        return [got[i] for i in ids]

    for a, b in zip(session(False), session(True)):
        np.testing.assert_array_equal(a, b)


def test_refusals(eng):
    F = 16
    x = R.rows(F)[5]
    L = len(x)
    kw = dict(silence_db=DB, trim=3, level_mode=2, fade_in=7, pcm16=True)
    ok = eng.finish([x], F, **kw)
    lib, ctx = eng.lib, eng.ctx
    buf = x[None].copy()
    ln = np.array([L], np.int32)
    out = np.full((1, L), R.SENT_H, np.int16)
    ol = np.full(1, -7, np.int32)
    info = (_capi.vx_wave_info * 1)()
    info[0].begin = -9
    fp, ip, vp = lambda a: _ptr(a, C.c_float), lambda a: _ptr(a, C.c_int32), lambda a: a.ctypes.data_as(C.c_void_p)
    good = _opts(F, **kw)

    def refused(field, *args):
        rc = lib.vx_finish(ctx, *args)
        msg = lib.vx_last_error(ctx).decode()
        assert rc == VX_EINVAL and field in msg and "vx_finish" in msg, (field, rc, msg)
        assert (out == R.SENT_H).all() and ol[0] == -7 and info[0].begin == -9, field      # nothing launched, nothing written

    o = C.byref(good)
    refused("wav", None, L, ip(ln), 1, o, vp(out), L, ip(ol), info)
    refused("lens", fp(buf), L, None, 1, o, vp(out), L, ip(ol), info)
    refused("o is NULL", fp(buf), L, ip(ln), 1, None, vp(out), L, ip(ol), info)
    refused("info", fp(buf), L, ip(ln), 1, o, vp(out), L, ip(ol), None)
    refused("out_lens", fp(buf), L, ip(ln), 1, o, vp(out), L, None, info)
    assert lib.vx_finish(None, fp(buf), L, ip(ln), 1, o, vp(out), L, ip(ol), info) == VX_EINVAL
    refused("batch", fp(buf), L, ip(ln), 0, o, vp(out), L, ip(ol), info)
    refused("batch", fp(buf), L, ip(ln), -1, o, vp(out), L, ip(ol), info)
    refused("lens[0]", fp(buf), L, ip(np.array([-1], np.int32)), 1, o, vp(out), L, ip(ol), info)
    refused("wav_stride", fp(buf), L, ip(np.array([L + 1], np.int32)), 1, o, vp(out), L, ip(ol), info)
    refused("out_stride", fp(buf), L, ip(ln), 1, o, vp(out), L - 1, ip(ol), info)      # the UNTRIMMED length, though the kept span is shorter
    assert ok[1][0]["end"] - ok[1][0]["begin"] < L - 1
    short = _opts(F, **kw)
    short.struct_size -= 4
    refused("struct_size", fp(buf), L, ip(ln), 1, C.byref(short), vp(out), L, ip(ol), info)
    nan, inf = float("nan"), float("inf")
    for field, bad in (("frame", 15), ("frame", 4097), ("silence_db", 0.5), ("silence_db", nan), ("silence_db", -inf), ("trim", 4),
                       ("trim", -1), ("keep", -1), ("level_mode", 3), ("level_mode", -1), ("level_db", 0.5), ("level_db", inf),
                       ("max_gain_db", -0.5), ("max_gain_db", nan), ("fade_in", -1), ("fade_in", (1 << 20) + 1), ("fade_out", -1),
                       ("fade_out", (1 << 20) + 1), ("format", 2), ("format", -1)):
        b = _opts(F, **kw)
        setattr(b, field, bad)
        refused(field, fp(buf), L, ip(ln), 1, C.byref(b), vp(out), L, ip(ol), info)
        refused(field, fp(buf), L, ip(ln), 1, C.byref(b), None, L, None, info)         # the options are checked in a measure-only call too
    with pytest.raises(VallexHipError) as ei:
        eng.dev_finish_frames(x, 15)
    assert ei.value.code == VX_EINVAL and "frame" in str(ei.value)
    with pytest.raises(VallexHipError) as ei:
        eng.finish([x], F, silence_db=1.0)
    assert ei.value.code == VX_EINVAL and "silence_db" in str(ei.value)
    # the context still finishes, to the same bits
    assert lib.vx_finish(ctx, fp(buf), L, ip(ln), 1, o, vp(out), L, ip(ol), info) == 0
    assert ol[0] == len(ok[0][0]) and (out[0, ol[0]:] == R.SENT_H).all() and info[0].begin == ok[1][0]["begin"]
    np.testing.assert_array_equal(out[0, : ol[0]], ok[0][0])
    assert math.isfinite(info[0].gain) and info[0].clipped == ok[1][0]["clipped"]
