"""GPU: the true-peak look-ahead limiter on the device (vx_limit / vx_finish_limited, csrc/limit.hip) against tests/_limit_refs.py, the
numpy restatement of the header's contract, on the taps and the ceiling the library reports.

Detector readings, gains, outputs and infos are compared bit for bit: the hold and the smoothing are integers, everything else is a
function of a few samples.  The gain of vx_finish_limited goes through log10 and pow on the host: it is held to 1 fp32 ulp, and the
outputs are compared with the restatement applied at the gain the call REPORTED.  One un-finalized context serves the kernel tests:
the entries need no weights."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from tests import _finish_refs as FR
from tests import _limit_refs as R
from tests import _loudness_refs as LR
from tests import _resample_refs as RS
from vallex_amd import _capi
from vallex_amd._capi import VX_EINVAL, Engine, VallexHipError, _ptr

pytestmark = pytest.mark.gpu

TILE = 2048                      # LM_T of csrc/limit.hip
DB = -40.0


@pytest.fixture(scope="module")
def eng():
    e = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)      # created, never finalized
    yield e
    e.close()


@pytest.fixture(scope="module")
def taps(eng):
    """n -> the reported taps; they are the resampler's"""
    t = {n: eng.limit_taps(n) for n in (1, 2, 4, 8)}
    for n in (2, 4, 8):
        assert np.array_equal(R.bits(t[n]), R.bits(RS.taps(1, n))) and t[n].shape == (n, 15)
    assert t[1].shape == (0, 15)
    return t


def _bits(a):
    return a.view(np.uint16 if a.dtype == np.int16 else np.uint32)


def _same(a, b, msg=""):
    assert a.dtype == b.dtype and a.shape == b.shape, (msg, a.dtype, b.dtype, a.shape, b.shape)
    np.testing.assert_array_equal(_bits(np.ascontiguousarray(a)), _bits(np.ascontiguousarray(b)), err_msg=str(msg))


def _same_info(got, want, what):
    for k in ("peak", "min_gain", "ceiling"):
        assert R.bits(np.float32(got[k])) == R.bits(np.float32(want[k])), (what, k, got, want)
    assert (got["reduced"], got["nonfinite"]) == (want["reduced"], want["nonfinite"]), (what, got, want)


def _rows(Wn):
    """the rows of the CPU suite at this look-ahead, plus rows around the kernel's tile"""
    rows = dict(R.cpu_rows(Wn))
    for L in (TILE - 1, TILE, TILE + 1, 2 * TILE + 5):
        rows["len%d" % L] = R.noise(L, L, 0.7)
    return rows


OPTS = [(1.0, -1.0), (2.5, -1.0), (1.0, 0.0), (2.5, 0.0)]


@pytest.mark.parametrize("Wn", [1, 16, 1024])
@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_word_for_word(eng, taps, Wn, n):
    """P and g as the kernel wrote them, the outputs and the infos of the ragged batch, every row alone: the restatement's words"""
    rows = _rows(Wn)
    names = list(rows)
    for k, (gs, db) in enumerate(OPTS if (Wn, n) in ((16, 4), (1024, 2)) else [OPTS[(Wn + n) % 4]]):
        outs, infos = eng.limit([rows[m] for m in names], db, gs, Wn, n)
        c = np.float32(infos[0]["ceiling"])
        assert R.ulp_diff([c], [R.ceiling(db)])[0] <= 1
        for i, name in enumerate(names):
            x = rows[name]
            want = R.limit(x, gs, c, Wn, n, taps[n])
            what = (Wn, n, gs, db, name)
            _same(outs[i], want["out"], what)
            _same_info(infos[i], want, what)
            assert np.all(np.abs(outs[i].astype(np.float64)) <= float(c) * (1.0 + 2.0 ** -22)), what
            if k == 0:
                P, g = eng.dev_limit_gain(x, gs, db, Wn, n)
                _same(P, want["P"], what)
                _same(g, want["g"], what)
                one, info1 = eng.limit([x], db, gs, Wn, n)                 # alone: the bits of the batch
                _same(one[0], outs[i], what)
                _same_info(info1[0], infos[i], what)
    assert eng.limit([], -1.0) == ([], [])


def test_properties_on_the_device(eng):
    """under the ceiling the input bits come back; the all-zero row; two calls give the same bits"""
    x = R.cpu_rows(16)["under"]
    out, info = eng.limit([x, np.zeros(100, np.float32), np.zeros(0, np.float32)])
    _same(out[0], x)
    assert info[0]["reduced"] == 0 and info[0]["min_gain"] == 1.0
    assert not out[1].any() and info[1]["peak"] == 0 and info[1]["min_gain"] == 1.0
    assert len(out[2]) == 0 and (info[2]["peak"], info[2]["min_gain"], info[2]["reduced"], info[2]["nonfinite"]) == (0.0, 1.0, 0, 0)
    y = R.voice(24000, 24000, 3, 0.9)
    a, ia = eng.limit([y], -1.0, 2.0)
    b, ib = eng.limit([y], -1.0, 2.0)
    _same(a[0], b[0])
    assert ia == ib and ia[0]["reduced"] > 0


def test_true_peak_measures_only(eng, taps):
    rows = [R.voice(8000, 8000, 4, 0.8), R.noise(TILE + 77, 9, 0.4), R.nonfinite_row(), np.zeros(0, np.float32)]
    got = eng.true_peak(rows, 4)
    for x, g in zip(rows, got):
        want = R.limit(x, 1.0, np.float32(1), 1, 4, taps[4])
        assert R.bits(np.float32(g["peak"])) == R.bits(want["peak"]) and g["nonfinite"] == want["nonfinite"]
        assert g["min_gain"] == 1.0 and g["reduced"] == 0 and g["ceiling"] == 1.0
    # against the resampler itself: max(|x|, |resample(x, 8000, 32000)|) within the derived bound of its K fp32 fmas
    x = rows[0]
    up = eng.resample([x], 8000, 32000)[0]
    y64, a = RS.resample_ref64(x, taps[4], 1, 4, 7)
    bound = float(RS.bound(a, 15).max())
    ref = max(float(np.abs(x).max()), float(np.abs(up).max()))
    assert abs(got[0]["peak"] - ref) <= bound + float(np.spacing(np.float32(ref))), (got[0]["peak"], ref, bound)
    assert abs(got[0]["peak"] - max(float(np.abs(x).max()), float(np.abs(y64).max()))) <= float(np.spacing(np.float32(ref)))


def _raw(eng, rows, rate, lufs, ceiling_db=-1.0, lookahead=None, oversample=4, out=True, pad=5, **kw):
    """vx_finish_limited on a sentinel-filled out: (rc, message, out (n, stride + pad), out_lens, infos, loudness infos, limiter infos)"""
    n = len(rows)
    ln = np.array([len(r) for r in rows], np.int32)
    ws = max(1, int(ln.max()))
    buf = np.zeros((n, ws), np.float32)
    for i, r in enumerate(rows):
        buf[i, : len(r)] = r
    o = dict(FR.DEFAULTS, **kw)
    pcm16 = o["pcm16"]
    outa = np.full((n, ws + pad), FR.SENT_H if pcm16 else FR.SENT_F, np.int16 if pcm16 else np.float32)
    ol = np.full(n, -7, np.int32)
    info, linfo, minfo = (_capi.vx_wave_info * n)(), (_capi.vx_loudness_info * n)(), (_capi.vx_limit_info * n)()
    fo = _capi.vx_finish_opts(C.sizeof(_capi.vx_finish_opts), rate // 100, o["silence_db"], o["trim"], o["keep"], o["level_mode"], o["level_db"],
                              o["max_gain_db"], o["fade_in"], o["fade_out"], _capi.PCM_S16 if pcm16 else _capi.PCM_F32)
    lo = _capi.vx_loudness_opts(C.sizeof(_capi.vx_loudness_opts), rate, lufs, ceiling_db)
    lim = _capi.vx_limit_opts(C.sizeof(_capi.vx_limit_opts), rate // 200 if lookahead is None else lookahead, oversample)
    rc = eng.lib.vx_finish_limited(eng.ctx, _ptr(buf, C.c_float), ws, _ptr(ln, C.c_int32), n, C.byref(fo), C.byref(lo), C.byref(lim),
                                   outa.ctypes.data_as(C.c_void_p) if out else None, ws + pad, _ptr(ol, C.c_int32), info, linfo, minfo)
    dicts = [[{f[0]: getattr(w, f[0]) for f in t._fields_} for w in a]
             for t, a in ((_capi.vx_wave_info, info), (_capi.vx_loudness_info, linfo), (_capi.vx_limit_info, minfo))]
    return (rc, eng.lib.vx_last_error(eng.ctx).decode(), outa, ol) + tuple(dicts)


@pytest.fixture(scope="module")
def level_rows():
    """the ragged 8 kHz batch of the loudness tests (quiet leads and tails, a row with non-finite samples, an empty row)"""
    rows = LR.rows(8000)
    odd = rows[9].copy()
    odd[5], odd[9000], odd[9001], odd[16004] = np.nan, np.inf, -np.inf, np.nan
    return rows + [odd]


LEVEL_CASES = [dict(trim=t, fade_in=f, fade_out=f, pcm16=p) for t, f, p in itertools.product((0, 3), (0, 7), (False, True))]
LUFS = -3.0                      # loud enough that the limiter works on every row with a tone


@pytest.mark.parametrize("case", LEVEL_CASES, ids=lambda c: f"trim{c['trim']}-fade{c['fade_in']}-{'s16' if c['pcm16'] else 'f32'}")
def test_level_word_for_word(eng, taps, level_rows, case):
    """every output word is finish(limit(x[begin:end], g, ceiling)) -- from the restatements and from the two device calls -- at the
    reported gain; the gain is the restatement's within an ulp; the loudness is vx_loudness of the kept span bit for bit; nothing
    clips at -1 dB; nothing is written behind out_lens[b]; the measure-only call gives the same infos"""
    rows = level_rows
    coef = eng.loudness_coeffs(8000)
    kw = dict(case, silence_db=DB, keep=3)
    rc, msg, out, ol, infos, linfos, minfos = _raw(eng, rows, 8000, LUFS, **kw)
    assert rc == 0, msg
    sent = FR.SENT_H if case["pcm16"] else FR.SENT_F
    spans, worked = [], 0
    for b, x in enumerate(rows):
        w = FR.measure(x, 80, silence_db=DB, trim=case["trim"], keep=3)
        gi = infos[b]
        assert (gi["begin"], gi["end"], gi["active_frames"], gi["nonfinite"]) == (w["begin"], w["end"], w["active_frames"], w["nonfinite"]), b
        xs = x[w["begin"]:w["end"]]
        li = LR.measure(xs, 8000, coef)
        assert R.ulp_diff([gi["gain"]], [R.gain(li["loudness"], LUFS, 20.0)])[0] <= 1, (b, gi["gain"])
        lim = R.limit(xs, gi["gain"], np.float32(minfos[b]["ceiling"]), 40, 4, taps[4])
        _same_info(minfos[b], lim, (case, b))
        want, clipped = FR.apply(lim["out"], 0, len(xs), np.float32(1), case["fade_in"], case["fade_out"], case["pcm16"])
        assert clipped == 0 and gi["clipped"] == 0 and ol[b] == len(want) == w["end"] - w["begin"]
        _same(out[b, : ol[b]], want, (case, b))
        assert (out[b, ol[b]:] == sent).all()
        worked += lim["reduced"] > 0
        spans.append(xs)
    assert worked >= 8
    for b, li in enumerate(eng.loudness(spans, 8000)):                # the reported loudness is vx_loudness of the slice
        assert all(np.float64(li[k]).view(np.uint64) == np.float64(linfos[b][k]).view(np.uint64) if isinstance(li[k], float) else li[k] == linfos[b][k]
                   for k in li), (b, li, linfos[b])
    # the two device calls composed
    for b in (4, 9, 10):
        mid, _ = eng.limit([spans[b]], -1.0, infos[b]["gain"], 40, 4)
        fin, _ = eng.finish(mid, 80, fade_in=case["fade_in"], fade_out=case["fade_out"], pcm16=case["pcm16"])
        _same(out[b, : ol[b]], fin[0], (case, b))
    # measure only: the same infos, nothing written; the limiter then reports the span's true peak alone
    rc, msg, out2, ol2, infos2, linfos2, minfos2 = _raw(eng, rows, 8000, LUFS, out=False, **kw)
    assert rc == 0 and (out2 == sent).all() and ol2.tolist() == ol.tolist() and infos2 == infos
    for a, b in zip(minfos2, minfos):
        assert (a["peak"], a["nonfinite"], a["ceiling"], a["min_gain"], a["reduced"]) == (b["peak"], b["nonfinite"], b["ceiling"], 1.0, 0)


def test_the_point_of_the_feature(eng):
    """the row on which finish_loud's gain is set by the ceiling: the limited row is strictly closer to the target"""
    x = LR.rows(8000)[7]
    target = -3.0
    loud, li = eng.finish_loud([x], 8000, target)
    peak = li[0]["peak"]
    assert R.ulp_diff([li[0]["gain"]], [np.float32(10 ** (-1.0 / 20) / peak)])[0] <= 1          # the ceiling term won
    lim, mi = eng.finish_limited([x], 8000, target)
    a = eng.loudness(loud, 8000)[0]["loudness"]
    b = eng.loudness(lim, 8000)[0]["loudness"]
    tp = [20 * math.log10(v["peak"]) for v in eng.true_peak([loud[0], lim[0]], 4)]
    print(f"[limit] target {target} LUFS: finish_loud reaches {a:.3f} (gain {li[0]['gain']:.4f}, {tp[0]:+.3f} dBTP), finish_limited {b:.3f} "
          f"(gain {mi[0]['gain']:.4f}, {tp[1]:+.3f} dBTP, min gain {eng.last_limit_info[0]['min_gain']:.4f}); shortfall {target - b:.3f} LU")
    assert abs(b - target) < abs(a - target) and b <= target + 1e-3
    c = float(np.float32(eng.last_limit_info[0]["ceiling"]))
    assert float(np.abs(lim[0]).max()) <= c * (1.0 + 2.0 ** -22) and mi[0]["clipped"] == 0


def test_windows_are_bit_identical(eng, level_rows):
    """8192 and 9000 samples per launch: long rows go through several parts and launches and give the words of the default single
    pass; 0 restores the default; values out of range are refused"""
    assert _capi.DEV_LIMIT_WINDOW_MIN == 8192 and _capi.LIMIT_WINDOW == 1 << 23
    rows = [R.voice(30011, 8000, 5, 0.9), level_rows[9], R.noise(8192, 6, 0.6), level_rows[10]]
    kws = [dict(silence_db=DB, trim=3, keep=33, fade_in=7, fade_out=7, pcm16=p) for p in (False, True)] + [dict()]
    eng.dev_limit_window(0)
    ref_gain = [eng.dev_limit_gain(x, 2.0, -1.0, 120, 4) for x in rows] + [eng.dev_limit_gain(rows[0], 2.0, -1.0, 1024, 2)]
    ref_lim = eng.limit(rows, -1.0, 2.0, 120, 4)
    ref_tp = eng.true_peak(rows, 4)
    ref_out = [_raw(eng, rows, 8000, LUFS, **kw)[2:] for kw in kws]
    try:
        for win in (8192, 9000):
            eng.dev_limit_window(win)
            for x, (P, g) in zip(rows + [None], ref_gain):
                P2, g2 = eng.dev_limit_gain(x, 2.0, -1.0, 120, 4) if x is not None else eng.dev_limit_gain(rows[0], 2.0, -1.0, 1024, 2)
                _same(P2, P, win)
                _same(g2, g, win)
            outs, infos = eng.limit(rows, -1.0, 2.0, 120, 4)
            assert infos == ref_lim[1] and eng.true_peak(rows, 4) == ref_tp
            for a, b in zip(outs, ref_lim[0]):
                _same(a, b, win)
            for kw, (out, ol, infos, linfos, minfos) in zip(kws, ref_out):
                rc, msg, out2, ol2, infos2, linfos2, minfos2 = _raw(eng, rows, 8000, LUFS, **kw)
                assert rc == 0, msg
                assert infos2 == infos and ol2.tolist() == ol.tolist() and minfos2 == minfos, win
                np.testing.assert_array_equal(_bits(out2), _bits(out), err_msg=f"window {win}")
        for bad in (1, 8191, -5, (1 << 23) + 1):
            with pytest.raises(VallexHipError) as ei:
                eng.dev_limit_window(bad)
            assert ei.value.code == VX_EINVAL and "samples" in str(ei.value)
    finally:
        eng.dev_limit_window(0)
    out, ol, infos, _, minfos = ref_out[0]
    rc, _, out2, ol2, infos2, _, minfos2 = _raw(eng, rows, 8000, LUFS, **kws[0])
    assert rc == 0 and infos2 == infos and minfos2 == minfos
    np.testing.assert_array_equal(_bits(out2), _bits(out))


def _golden_codes12():
    from tests._util import golden
    codes = golden("nl2_bestof3")["codes"][0].astype(np.int64)
    assert codes.shape == (12, 8)
    return codes


def test_vocos_decode_to_a_limited_loudness():
    from tests._util import get_model
    from vallex_amd.utils.generation import Finish, LimitedFinish
    m = get_model(2, 0, 2.5, vocos=True)
    e = m.engine
    codes = [_golden_codes12(), _golden_codes12()[:5]]
    w24 = [w.copy() for w in e.vocos_decode(codes, 2)]
    w16 = e.resample(w24, 24000, 16000)
    fin = LimitedFinish(lufs=-16.0, pcm16=True)
    want, winfo = e.finish_limited(w16, 16000, -16.0, pcm16=True)
    wl, wm = e.last_loudness_info, e.last_limit_info
    got = e.vocos_decode(codes, 2, sample_rate=16000, finish=fin)
    assert e.last_finish_info == winfo and e.last_limit_info == wm and len(e.last_loudness_info) == len(wl)
    for a, b in zip(got, want):
        _same(a, b)
        assert a.dtype == np.int16
    fin = LimitedFinish(lufs=-10.0, ceiling_db=-3.0, lookahead=64, oversample=2, trim=3, keep=40, fade_in=16, fade_out=16)
    want = e.finish_limited(w24, 24000, -10.0, -3.0, 64, 2, None, fin.silence_db, 3, 40, fin.max_gain_db, 16, 16, False)[0]
    for a, b in zip(e.vocos_decode(codes, 2, finish=fin), want):       # at 24 kHz: frame 240
        _same(a, b)
    # a plain Finish with lufs: the bits of vx_finish_loud; without: the bits of vx_finish
    for a, b in zip(e.vocos_decode(codes, 2, finish=Finish(lufs=-16.0)), e.finish_loud(w24, 24000, -16.0)[0]):
        _same(a, b)
    for a, b in zip(e._finished(w24, Finish(), 24000), e.finish(w24, 240)[0]):
        _same(a, b)


def test_generate_audio_family():
    from oracle import synth
    from vallex_amd.utils import generation as G
    G.preload_models(state_dict=synth.vallex_state_dict(2, 11), vocos_state_dict=synth.vocos_state_dict(2), num_layers=2, max_new=64,
                     max_prompt=128, max_text=64, max_batch=2)
    e = G.model.engine
    ids = synth.synth_text(6, 1)
    us = synth.uniforms(32, 1, 5)[:, 0]
    fin = G.LimitedFinish(lufs=-12.0, trim=3, keep=80, fade_in=32, fade_out=32, pcm16=True)
    kw = dict(silence_db=fin.silence_db, trim=3, keep=80, max_gain_db=fin.max_gain_db, fade_in=32, fade_out=32, pcm16=True)
    w24 = G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12)
    w16 = e.resample([w24], 24000, 16000)[0]
    want16 = e.finish_limited([w16], 16000, -12.0, -1.0, **kw)[0][0]
    want24 = e.finish_limited([w24], 24000, -12.0, -1.0, **kw)[0][0]
    assert want16.dtype == np.int16
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, sample_rate=16000, finish=fin), want16)
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, finish=fin), want24)
    _same(G.generate_audio_batch([ids], language="en", uniforms=us[:, None], force_eos_at=12, sample_rate=16000, finish=fin)[0], want16)
    _same(G.generate_audio_from_long_text([ids], language="en", uniforms=us, force_eos_at=12, sample_rate=16000, finish=fin), want16)
    with G.AudioServer(sample_rate=16000, finish=fin, force_eos_at=12) as srv:
        s16 = srv.submit(ids, language="en", seed=9).result()
    with G.AudioServer(force_eos_at=12) as srv:
        s24 = srv.submit(ids, language="en", seed=9).result()
    _same(s16, e.finish_limited(e.resample([s24], 24000, 16000), 16000, -12.0, -1.0, **kw)[0][0])


def test_nothing_else_moves():
    """greedy ids of nl2_greedy_eos before and after interleaved limiter calls; a call while a serving session is open succeeds and
    the session's result is what it is without the call; no fallback is counted; Finish(lufs=) is still vx_finish_loud"""
    from tests._util import case_row, get_model, golden
    from vallex_amd.utils.generation import Finish
    c, row, _ = case_row("nl2_greedy_eos")
    m = get_model(c["num_layers"], c["seed"], c["eos_gain"], vocos=True)
    e = m.engine
    x = LR.rows(8000)[9]
    kw = dict(trim=3, fade_in=7, fade_out=7, pcm16=True)
    before = m.inference_batch([row], top_k=1, force_eos_at=c["force_eos_at"])[0]
    r1 = e.finish_limited([x], 8000, LUFS, **kw)[0][0].copy()
    l1, i1 = e.limit([x], -1.0, 3.0)
    l1 = l1[0].copy()
    after = m.inference_batch([row], top_k=1, force_eos_at=c["force_eos_at"])[0]
    np.testing.assert_array_equal(before, golden("nl2_greedy_eos")["codes"][0])
    np.testing.assert_array_equal(after, before)
    fb = e.last_fallbacks()
    e.finish_limited([x], 8000, -23.0)
    e.true_peak([x])
    assert e.last_fallbacks() == fb
    _same(l1, R.limit(x, 3.0, np.float32(i1[0]["ceiling"]), 120, 4, e.limit_taps(4))["out"])
    _same(e._finished([x], Finish(lufs=-16.0), 8000)[0], e.finish_loud([x], 8000, -16.0)[0][0])

    def session(interleave):
        got = {}
        with e.serve(top_k=10, force_eos_at=30) as sess:
            ids = sess.submit(m.make_batch([row, row]), [dict(seed=5), dict(seed=6, best_of=2)])
            sess.run(3, lambda rid, cd: got.__setitem__(rid, cd))
            if interleave:
                _same(e.finish_limited([x], 8000, LUFS, **kw)[0][0], r1)
                _same(e.limit([x], -1.0, 3.0)[0][0], l1)
            sess.run(0, lambda rid, cd: got.__setitem__(rid, cd))
        return [got[i] for i in ids]

    for a, b in zip(session(False), session(True)):
        np.testing.assert_array_equal(a, b)


def test_refusals(eng, level_rows):
    x = level_rows[8]
    L = len(x)
    lib, ctx = eng.lib, eng.ctx
    buf = x[None].copy()
    ln = np.array([L], np.int32)
    fp, ip, vp = lambda a: _ptr(a, C.c_float), lambda a: _ptr(a, C.c_int32), lambda a: a.ctypes.data_as(C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def mopts(**f):
        s = _capi.vx_limit_opts(C.sizeof(_capi.vx_limit_opts), 40, 4)
        for k, v in f.items():
            setattr(s, k, v)
        return s

    # vx_limit
    ok = eng.limit([x], -1.0, 3.0, 40, 4)
    out = np.full((1, L), FR.SENT_F, np.float32)
    info = (_capi.vx_limit_info * 1)()
    info[0].reduced = -9

    def refused(field, *args):
        rc = lib.vx_limit(ctx, *args)
        msg = lib.vx_last_error(ctx).decode()
        assert rc == VX_EINVAL and field in msg and "vx_limit" in msg, (field, rc, msg)
        assert (out == FR.SENT_F).all() and info[0].reduced == -9, field      # nothing written

    o = C.byref(mopts())
    refused("wav", None, L, ip(ln), 1, 3.0, -1.0, o, fp(out), L, info)
    refused("lens", fp(buf), L, None, 1, 3.0, -1.0, o, fp(out), L, info)
    refused("o is NULL", fp(buf), L, ip(ln), 1, 3.0, -1.0, None, fp(out), L, info)
    refused("info", fp(buf), L, ip(ln), 1, 3.0, -1.0, o, fp(out), L, None)
    refused("batch", fp(buf), L, ip(ln), 0, 3.0, -1.0, o, fp(out), L, info)
    refused("lens[0]", fp(buf), L, ip(np.array([-1], np.int32)), 1, 3.0, -1.0, o, fp(out), L, info)
    refused("wav_stride", fp(buf), L, ip(np.array([L + 1], np.int32)), 1, 3.0, -1.0, o, fp(out), L, info)
    refused("out_stride", fp(buf), L, ip(ln), 1, 3.0, -1.0, o, fp(out), L - 1, info)
    refused("vx_limit_opts.struct_size", fp(buf), L, ip(ln), 1, 3.0, -1.0, C.byref(mopts(struct_size=8)), fp(out), L, info)
    assert lib.vx_limit(None, fp(buf), L, ip(ln), 1, 3.0, -1.0, o, fp(out), L, info) == VX_EINVAL
    for bad in (0.0, -1.0, nan, inf):
        refused("pre_gain", fp(buf), L, ip(ln), 1, bad, -1.0, o, fp(out), L, info)
    for bad in (0.5, nan, inf, -inf):
        refused("ceiling_db", fp(buf), L, ip(ln), 1, 3.0, bad, o, fp(out), L, info)
    for field, bad in (("lookahead", 0), ("lookahead", 1025), ("lookahead", -1), ("oversample", 0), ("oversample", 3), ("oversample", 16)):
        refused(field, fp(buf), L, ip(ln), 1, 3.0, -1.0, C.byref(mopts(**{field: bad})), fp(out), L, info)
        refused(field, fp(buf), L, ip(ln), 1, 3.0, -1.0, C.byref(mopts(**{field: bad})), None, 0, info)      # in a measure-only call too
    for edge in (dict(lookahead=1), dict(lookahead=1024), dict(oversample=1), dict(oversample=8)):
        assert lib.vx_limit(ctx, fp(buf), L, ip(ln), 1, 3.0, 0.0, C.byref(mopts(**edge)), None, 0, (_capi.vx_limit_info * 1)()) == 0, edge
    t = np.full((8, 15), -7.0, np.float32)
    assert lib.vx_limit_taps(3, fp(t)) == VX_EINVAL and lib.vx_limit_taps(0, fp(t)) == VX_EINVAL and lib.vx_limit_taps(4, None) == VX_EINVAL
    assert (t == -7.0).all()
    with pytest.raises(ValueError):
        eng.limit_taps(16)
    with pytest.raises(VallexHipError) as ei:
        eng.dev_limit_gain(x, 1.0, -1.0, 2000, 4)
    assert ei.value.code == VX_EINVAL and "lookahead" in str(ei.value)
    assert lib.vx_limit(ctx, fp(buf), L, ip(ln), 1, 3.0, -1.0, o, fp(out), L, info) == 0
    _same(out[0], ok[0][0])
    assert {f[0]: getattr(info[0], f[0]) for f in _capi.vx_limit_info._fields_} == ok[1][0]

    # vx_finish_limited
    kw = dict(silence_db=DB, trim=3, fade_in=7, pcm16=True)
    ok = eng.finish_limited([x], 8000, LUFS, **kw)
    ok_m = eng.last_limit_info[0]
    out = np.full((1, L), FR.SENT_H, np.int16)
    ol = np.full(1, -7, np.int32)
    winfo, linfo, minfo = (_capi.vx_wave_info * 1)(), (_capi.vx_loudness_info * 1)(), (_capi.vx_limit_info * 1)()
    winfo[0].begin = -9
    linfo[0].blocks = -9
    minfo[0].reduced = -9

    def fopts(**f):
        d = dict(FR.DEFAULTS, **kw)
        s = _capi.vx_finish_opts(C.sizeof(_capi.vx_finish_opts), 80, d["silence_db"], d["trim"], d["keep"], 0, d["level_db"], d["max_gain_db"],
                                 d["fade_in"], d["fade_out"], _capi.PCM_S16)
        for k, v in f.items():
            setattr(s, k, v)
        return s

    def lopts(**f):
        s = _capi.vx_loudness_opts(C.sizeof(_capi.vx_loudness_opts), 8000, LUFS, -1.0)
        for k, v in f.items():
            setattr(s, k, v)
        return s

    def refused2(field, *args):
        rc = lib.vx_finish_limited(ctx, *args)
        msg = lib.vx_last_error(ctx).decode()
        assert rc == VX_EINVAL and field in msg and "vx_finish_limited" in msg, (field, rc, msg)
        assert (out == FR.SENT_H).all() and ol[0] == -7 and winfo[0].begin == -9 and linfo[0].blocks == -9 and minfo[0].reduced == -9, field

    fo, lo, mo = C.byref(fopts()), C.byref(lopts()), C.byref(mopts())
    tail = (vp(out), L, ip(ol), winfo, linfo, minfo)
    refused2("wav", None, L, ip(ln), 1, fo, lo, mo, *tail)
    refused2("lens", fp(buf), L, None, 1, fo, lo, mo, *tail)
    refused2("o is NULL", fp(buf), L, ip(ln), 1, None, lo, mo, *tail)
    refused2("lo is NULL", fp(buf), L, ip(ln), 1, fo, None, mo, *tail)
    refused2("lim is NULL", fp(buf), L, ip(ln), 1, fo, lo, None, *tail)
    refused2("info", fp(buf), L, ip(ln), 1, fo, lo, mo, vp(out), L, ip(ol), None, linfo, minfo)
    refused2("linfo", fp(buf), L, ip(ln), 1, fo, lo, mo, vp(out), L, ip(ol), winfo, None, minfo)
    refused2("liminfo", fp(buf), L, ip(ln), 1, fo, lo, mo, vp(out), L, ip(ol), winfo, linfo, None)
    refused2("out_lens", fp(buf), L, ip(ln), 1, fo, lo, mo, vp(out), L, None, winfo, linfo, minfo)
    assert lib.vx_finish_limited(None, fp(buf), L, ip(ln), 1, fo, lo, mo, *tail) == VX_EINVAL
    refused2("batch", fp(buf), L, ip(ln), 0, fo, lo, mo, *tail)
    refused2("lens[0]", fp(buf), L, ip(np.array([-1], np.int32)), 1, fo, lo, mo, *tail)
    refused2("wav_stride", fp(buf), L, ip(np.array([L + 1], np.int32)), 1, fo, lo, mo, *tail)
    refused2("out_stride", fp(buf), L, ip(ln), 1, fo, lo, mo, vp(out), L - 1, ip(ol), winfo, linfo, minfo)
    refused2("vx_finish_opts.struct_size", fp(buf), L, ip(ln), 1, C.byref(fopts(struct_size=40)), lo, mo, *tail)
    refused2("vx_loudness_opts.struct_size", fp(buf), L, ip(ln), 1, fo, C.byref(lopts(struct_size=12)), mo, *tail)
    refused2("vx_limit_opts.struct_size", fp(buf), L, ip(ln), 1, fo, lo, C.byref(mopts(struct_size=16)), *tail)
    for field, bad in (("level_mode", 1), ("level_mode", 2), ("frame", 15), ("silence_db", 0.5), ("trim", 4), ("keep", -1), ("max_gain_db", nan),
                       ("fade_in", -1), ("fade_out", (1 << 20) + 1), ("format", 2)):
        refused2(field, fp(buf), L, ip(ln), 1, C.byref(fopts(**{field: bad})), lo, mo, *tail)
    for field, bad in (("sample_rate", 7999), ("sample_rate", 192001), ("target_lufs", 0.5), ("target_lufs", nan), ("ceiling_db", 0.5),
                       ("ceiling_db", nan), ("ceiling_db", -inf)):
        refused2(field, fp(buf), L, ip(ln), 1, fo, C.byref(lopts(**{field: bad})), mo, *tail)
    for field, bad in (("lookahead", 0), ("lookahead", 1025), ("oversample", 5), ("oversample", -2)):
        refused2(field, fp(buf), L, ip(ln), 1, fo, lo, C.byref(mopts(**{field: bad})), *tail)
    with pytest.raises(VallexHipError) as ei:
        eng.finish_limited([x], 8000, LUFS, oversample=3)
    assert ei.value.code == VX_EINVAL and "oversample" in str(ei.value)
    # the context still levels, to the same bits
    assert lib.vx_finish_limited(ctx, fp(buf), L, ip(ln), 1, fo, lo, mo, *tail) == 0
    assert ol[0] == len(ok[0][0]) and (out[0, ol[0]:] == FR.SENT_H).all() and winfo[0].begin == ok[1][0]["begin"]
    np.testing.assert_array_equal(out[0, : ol[0]], ok[0][0])
    assert {f[0]: getattr(minfo[0], f[0]) for f in _capi.vx_limit_info._fields_} == ok_m
