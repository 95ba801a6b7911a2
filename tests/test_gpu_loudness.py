"""GPU: BS.1770 loudness on the device (vx_loudness / vx_finish_loud, csrc/loudness.hip) against tests/_loudness_refs.py, the numpy
restatement of the header's contract, on the coefficients the library reports.

Step tables, counts, mean squares and every output word are compared bit for bit.  loudness and max_momentary go through log10 on
the host: they are held to 1e-12.  The gain goes through pow: it is held to 1 fp32 ulp, and the outputs are compared with the
restatement applied at the gain the call REPORTED.  Every block of every input is at least 0.1 dB away from both gates and every
frame a quarter of an octave from the silence threshold (asserted on the reference), so a last bit of log10 or pow cannot flip one.
One un-finalized context serves the kernel tests: the entries need no weights."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from tests import _finish_refs as FR
from tests import _loudness_refs as R
from vallex_amd import _capi
from vallex_amd._capi import VX_EINVAL, Engine, VallexHipError, _ptr

pytestmark = pytest.mark.gpu

RATES = (8000, 24000, 11025)
DB = -40.0


@pytest.fixture(scope="module")
def eng():
    e = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)      # created, never finalized
    yield e
    e.close()


@pytest.fixture(scope="module")
def data(eng):
    """rate -> (reported coefficients, rows, step tables of the restatement on those coefficients) -- computed once.  The 8 kHz set
    ends with a row holding a NaN and both infinities (each also lies in the warm-up of later steps)."""
    d = {}
    for rate in RATES:
        c = eng.loudness_coeffs(rate)
        assert float(np.max(np.abs(c - R.coeffs(rate)))) <= 1e-14
        rows = R.rows(rate)
        if rate == 8000:
            odd = rows[9].copy()
            odd[5], odd[9000], odd[9001], odd[16004] = np.nan, np.inf, -np.inf, np.nan
            rows.append(odd)
        zs = [R.steps(x, rate, c) for x in rows]
        for x, z in zip(rows, zs):
            assert R.gate_margin_db(z, len(x), rate // 10) >= 0.1
        d[rate] = (c, rows, zs)
    return d


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _bits(a):
    return a.view(np.uint16 if a.dtype == np.int16 else np.uint32)


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    np.testing.assert_array_equal(_bits(np.ascontiguousarray(a)), _bits(np.ascontiguousarray(b)))


def _same_linfo(got, want, what):
    for k in ("blocks", "above_abs", "gated", "nonfinite"):
        assert got[k] == want[k], (what, k, got, want)
    assert _u64([got["mean_square"]])[0] == _u64([want["mean_square"]])[0], (what, got, want)
    for k in ("loudness", "max_momentary"):
        assert got[k] == want[k] if math.isinf(want[k]) else abs(got[k] - want[k]) <= 1e-12, (what, k, got, want)


def _equal_bits(a, b):
    return all(_u64([a[k]])[0] == _u64([b[k]])[0] if isinstance(a[k], float) else a[k] == b[k] for k in a)


@pytest.mark.parametrize("rate", RATES)
def test_steps_word_for_word(eng, data, rate):
    """every z_j is the restatement's double: one lane, from rest at j S - W, every operation rounded on its own (a contracted
    multiply-add in the recursion changes these words)"""
    c, rows, zs = data[rate]
    for x, z in zip(rows, zs):
        got = eng.dev_loudness_steps(x, rate)
        assert got.shape == z.shape
        np.testing.assert_array_equal(_u64(got), _u64(z), err_msg=f"rate {rate}, row of {len(x)}")


def test_measure_alone_and_as_one_ragged_batch(eng, data):
    c, rows, zs = data[8000]
    want = [R.measure(x, 8000, c, z) for x, z in zip(rows, zs)]
    batch = eng.loudness(rows, 8000)
    for i, (g, w) in enumerate(zip(batch, want)):
        _same_linfo(g, w, f"batch row {i}")
        one = eng.loudness([rows[i]], 8000)[0]
        assert _equal_bits(one, g), (i, one, g)
    assert want[0]["blocks"] == 0 and want[-1]["nonfinite"] == 4 and want[9]["gated"] < want[9]["above_abs"] < want[9]["blocks"]
    q = R.quiet_row(4801, 8000)
    assert R.gate_margin_db(R.steps(q, 8000, c), len(q), 800) >= 0.1
    g = eng.loudness([q], 8000)[0]
    _same_linfo(g, R.measure(q, 8000, c), "noise floor")
    assert g["above_abs"] == 0 and g["loudness"] == -math.inf and g["blocks"] == 3
    for rate in (24000, 11025):
        c2, rows2, zs2 = data[rate]
        for g, x, z in zip(eng.loudness(rows2, rate), rows2, zs2):
            _same_linfo(g, R.measure(x, rate, c2, z), f"rate {rate}")
    assert eng.loudness([], 8000) == []


def _raw(eng, rows, rate, lufs, ceiling_db=-1.0, out=True, pad=5, **kw):
    """vx_finish_loud on a sentinel-filled out: (rc, message, out (n, stride + pad), out_lens, infos, loudness infos)"""
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
    info, linfo = (_capi.vx_wave_info * n)(), (_capi.vx_loudness_info * n)()
    fo = _capi.vx_finish_opts(C.sizeof(_capi.vx_finish_opts), rate // 100, o["silence_db"], o["trim"], o["keep"], o["level_mode"], o["level_db"],
                              o["max_gain_db"], o["fade_in"], o["fade_out"], _capi.PCM_S16 if pcm16 else _capi.PCM_F32)
    lo = _capi.vx_loudness_opts(C.sizeof(_capi.vx_loudness_opts), rate, lufs, ceiling_db)
    rc = eng.lib.vx_finish_loud(eng.ctx, _ptr(buf, C.c_float), ws, _ptr(ln, C.c_int32), n, C.byref(fo), C.byref(lo),
                                outa.ctypes.data_as(C.c_void_p) if out else None, ws + pad, _ptr(ol, C.c_int32), info, linfo)
    infos = [{f[0]: getattr(w, f[0]) for f in _capi.vx_wave_info._fields_} for w in info]
    linfos = [{f[0]: getattr(w, f[0]) for f in _capi.vx_loudness_info._fields_} for w in linfo]
    return rc, eng.lib.vx_last_error(eng.ctx).decode(), outa, ol, infos, linfos


def _want(x, rate, c, lufs, ceiling_db, **kw):
    """the restatement of vx_finish_loud on one row: (vx_wave_info without gain and clipped, vx_loudness_info, gain)"""
    o = dict(FR.DEFAULTS, **kw)
    w = FR.measure(x, rate // 100, silence_db=o["silence_db"], trim=o["trim"], keep=o["keep"])
    xs = x[w["begin"]:w["end"]]
    z = R.steps(xs, rate, c)
    assert R.gate_margin_db(z, len(xs), rate // 10) >= 0.1
    li = R.measure(xs, rate, c, z)
    return w, li, R.gain(li["loudness"], lufs, ceiling_db, o["max_gain_db"], w["peak"])


LEVEL_CASES = [dict(trim=t, fade_in=f, fade_out=f, pcm16=p) for t, f, p in itertools.product((0, 3), (0, 7), (False, True))]


@pytest.mark.parametrize("case", LEVEL_CASES, ids=lambda c: f"trim{c['trim']}-fade{c['fade_in']}-{'s16' if c['pcm16'] else 'f32'}")
def test_level_word_for_word(eng, data, case):
    """the ragged 8 kHz batch to -16 LUFS: every output word is the restatement's at the reported gain, the gain is the restatement's
    within an ulp, the loudness is vx_loudness of the kept span bit for bit, nothing is written behind out_lens[b]"""
    c, rows, _ = data[8000]
    for x in rows:
        assert FR.margin(x, 80, DB) >= 0.25
    kw = dict(case, silence_db=DB, keep=3)
    rc, msg, out, ol, infos, linfos = _raw(eng, rows, 8000, -16.0, **kw)
    assert rc == 0, msg
    sent = FR.SENT_H if case["pcm16"] else FR.SENT_F
    spans = []
    for b, x in enumerate(rows):
        w, li, g = _want(x, 8000, c, -16.0, -1.0, **kw)
        gi = infos[b]
        assert (gi["begin"], gi["end"], gi["active_frames"], gi["nonfinite"]) == (w["begin"], w["end"], w["active_frames"], w["nonfinite"]), b
        assert np.float32(gi["peak"]).view(np.uint32) == np.float32(w["peak"]).view(np.uint32)
        assert R.ulp_diff([gi["gain"]], [g])[0] <= 1, (b, gi["gain"], g)
        _same_linfo(linfos[b], li, (case, b))
        want, clipped = FR.apply(x, w["begin"], w["end"], gi["gain"], case["fade_in"], case["fade_out"], case["pcm16"])
        assert gi["clipped"] == clipped and ol[b] == len(want) == w["end"] - w["begin"]
        np.testing.assert_array_equal(_bits(out[b, : ol[b]]), _bits(want), err_msg=f"{case}, row {b}")
        assert (out[b, ol[b]:] == sent).all()
        spans.append(x[w["begin"]:w["end"]])
    for b, li in enumerate(eng.loudness(spans, 8000)):                # the reported loudness is vx_loudness of the slice
        assert _equal_bits(li, linfos[b]), (b, li, linfos[b])
    if case["trim"] == 3:
        assert infos[9]["begin"] > 7000 and linfos[9]["blocks"] < 17     # the quiet lead is cut: the loud part alone is measured
        assert linfos[0]["blocks"] == 0 and infos[0]["gain"] == 1
    # measure only: the same infos, nothing written
    rc, msg, out2, ol2, infos2, linfos2 = _raw(eng, rows, 8000, -16.0, out=False, **kw)
    assert rc == 0 and (out2 == sent).all() and ol2.tolist() == ol.tolist()
    assert all(_equal_bits(a, b) for a, b in zip(linfos2, linfos))
    assert [dict(i, clipped=0) for i in infos] == infos2


def test_gain_by_target_cap_and_ceiling(eng, data):
    c, rows, _ = data[8000]
    x = rows[7]                                                         # 4 S + 1 of tone, peak about 0.25
    w, li, _ = _want(x, 8000, c, -16.0, -1.0)
    L, peak = li["loudness"], float(np.float32(w["peak"]))
    ceil = 10 ** (-1.0 / 20)
    for lufs, cap, ceiling_db, term in ((-16.0, 20.0, -1.0, 10 ** ((-16.0 - L) / 20)), (-6.0, 3.0, -1.0, 10 ** (3.0 / 20)),
                                        (-3.0, 20.0, -1.0, ceil / peak), (-30.0, 20.0, -1.0, 10 ** ((-30.0 - L) / 20))):
        others = [10 ** ((lufs - L) / 20), 10 ** (cap / 20), 10 ** (ceiling_db / 20) / peak]
        assert term == min(others) and sorted(others)[1] / term > 1.01      # the case is decided by the term it names
        out, infos = eng.finish_loud([x], 8000, lufs, ceiling_db, max_gain_db=cap)
        g = infos[0]["gain"]
        assert R.ulp_diff([g], [np.float32(term)])[0] <= 1 and R.ulp_diff([g], [R.gain(L, lufs, ceiling_db, cap, w["peak"])])[0] <= 1
        _same(out[0], FR.apply(x, 0, len(x), g)[0])
        assert _equal_bits(eng.last_loudness_info[0], eng.loudness([x], 8000)[0])
        if term == ceil / peak:
            assert abs(float(np.float32(g)) * peak - ceil) <= float(np.spacing(np.float32(ceil)))
            assert np.abs(out[0]).max() <= np.float32(ceil) + np.spacing(np.float32(ceil)) and infos[0]["clipped"] == 0
    # nothing passes the gates: the gain is 1
    q = R.quiet_row(4801, 8000)
    out, infos = eng.finish_loud([q], 8000, -16.0)
    assert infos[0]["gain"] == 1 and eng.last_loudness_info[0]["loudness"] == -math.inf
    _same(out[0], q)
    assert eng.finish_loud([], 8000, -16.0) == ([], []) and eng.last_loudness_info == []


def test_round_trip_reaches_the_target(eng, data):
    """the levelled row measures -16 LUFS: the fp32 rounding of the gain and of the samples are each about 5e-7 dB"""
    c, rows, zs = data[8000]
    x, z = rows[7], zs[7]
    assert all(10 * math.log10(v / R.ABS_GATE) >= 25 for v in R.blocks(z, len(x), 800))
    out, infos = eng.finish_loud([x], 8000, -16.0)
    assert infos[0]["clipped"] == 0 and out[0].dtype == np.float32 and len(out[0]) == len(x)
    got = eng.loudness(out, 8000)[0]["loudness"]
    print(f"after finish_loud(lufs=-16): {got:.7f} LUFS (gain {infos[0]['gain']:.6f})")
    assert abs(got - (-16.0)) <= 1e-5


def test_windows_are_bit_identical(eng, data):
    """4096 and 5000 samples per launch: the 20 S + 5 and 7 S + 13 rows go through several jobs and launches and give the words of
    the default single pass; 0 restores the default; values out of range, and a window below 3 S of the call's rate, are refused"""
    assert _capi.DEV_LOUDNESS_WINDOW_MIN == 4096 and _capi.LOUDNESS_WINDOW == 1 << 23
    c, rows, zs = data[8000]
    rows = [rows[9], rows[8], rows[10]]
    kws = [dict(silence_db=DB, trim=3, keep=33, fade_in=7, fade_out=7, pcm16=p) for p in (False, True)] + [dict()]
    eng.dev_loudness_window(0)
    ref_steps = [eng.dev_loudness_steps(x, 8000) for x in rows]
    ref_info = eng.loudness(rows, 8000)
    ref_out = [_raw(eng, rows, 8000, -16.0, **kw)[2:] for kw in kws]
    try:
        for win in (4096, 5000):
            eng.dev_loudness_window(win)
            for x, z in zip(rows, ref_steps):
                np.testing.assert_array_equal(_u64(eng.dev_loudness_steps(x, 8000)), _u64(z), err_msg=f"window {win}")
            assert all(_equal_bits(a, b) for a, b in zip(eng.loudness(rows, 8000), ref_info)), win
            for kw, (out, ol, infos, linfos) in zip(kws, ref_out):
                rc, msg, out2, ol2, infos2, linfos2 = _raw(eng, rows, 8000, -16.0, **kw)
                assert rc == 0, msg
                assert infos2 == infos and ol2.tolist() == ol.tolist() and all(_equal_bits(a, b) for a, b in zip(linfos2, linfos)), win
                np.testing.assert_array_equal(_bits(out2), _bits(out), err_msg=f"window {win}")
        # a window below 3 S of the rate is refused by the call, not enlarged
        eng.dev_loudness_window(4096)
        x24 = data[24000][1][0]
        for call in (lambda: eng.loudness([x24], 24000), lambda: eng.dev_loudness_steps(x24, 24000), lambda: eng.finish_loud([x24], 24000, -16.0)):
            with pytest.raises(VallexHipError) as ei:
                call()
            assert ei.value.code == VX_EINVAL and "3 S" in str(ei.value)
        for bad in (1, 4095, -5, (1 << 23) + 1):
            with pytest.raises(VallexHipError) as ei:
                eng.dev_loudness_window(bad)
            assert ei.value.code == VX_EINVAL and "samples" in str(ei.value)
    finally:
        eng.dev_loudness_window(0)
    np.testing.assert_array_equal(_u64(eng.dev_loudness_steps(x24, 24000)), _u64(data[24000][2][0]))
    out, ol, infos, linfos = ref_out[0]
    rc, _, out2, ol2, infos2, _ = _raw(eng, rows, 8000, -16.0, **kws[0])
    assert rc == 0 and infos2 == infos
    np.testing.assert_array_equal(_bits(out2), _bits(out))


def _golden_codes12():
    from tests._util import golden
    codes = golden("nl2_bestof3")["codes"][0].astype(np.int64)
    assert codes.shape == (12, 8)
    return codes


def test_vocos_decode_to_a_loudness():
    from tests._util import get_model
    from vallex_amd.utils.generation import Finish
    m = get_model(2, 0, 2.5, vocos=True)
    e = m.engine
    codes = [_golden_codes12(), _golden_codes12()[:5]]
    w24 = [w.copy() for w in e.vocos_decode(codes, 2)]
    w16 = e.resample(w24, 24000, 16000)
    fin = Finish(lufs=-16.0, pcm16=True)
    want, winfo = e.finish_loud(w16, 16000, -16.0, pcm16=True)
    wl = e.last_loudness_info
    got = e.vocos_decode(codes, 2, sample_rate=16000, finish=fin)
    assert e.last_finish_info == winfo and all(_equal_bits(a, b) for a, b in zip(e.last_loudness_info, wl))
    for a, b in zip(got, want):
        _same(a, b)
        assert a.dtype == np.int16
    fin = Finish(lufs=-23.0, ceiling_db=-3.0, trim=3, keep=40, fade_in=16, fade_out=16)
    want = e.finish_loud(w24, 24000, -23.0, -3.0, None, fin.silence_db, 3, 40, fin.max_gain_db, 16, 16, False)[0]
    for a, b in zip(e.vocos_decode(codes, 2, finish=fin), want):       # at 24 kHz: frame 240
        _same(a, b)
    # Finish() without lufs: the bits of vx_finish
    old = Finish(level_mode=2, level_db=-20.0, pcm16=True)
    for a, b in zip(e.vocos_decode(codes, 2, finish=old), e.finish(w24, 240, level_mode=2, level_db=-20.0, pcm16=True)[0]):
        _same(a, b)
    for a, b in zip(e._finished(w24, Finish(), 24000), e.finish(w24, 240)[0]):
        _same(a, b)


def test_generate_audio_family_and_the_enrolment_level():
    from oracle import synth
    from vallex_amd.utils import generation as G
    from vallex_amd.utils import prompt_making as PM
    G.preload_models(state_dict=synth.vallex_state_dict(2, 11), vocos_state_dict=synth.vocos_state_dict(2), num_layers=2, max_new=64,
                     max_prompt=128, max_text=64, max_batch=2)
    e = G.model.engine
    ids = synth.synth_text(6, 1)
    us = synth.uniforms(32, 1, 5)[:, 0]
    fin = G.Finish(lufs=-16.0, trim=3, keep=80, fade_in=32, fade_out=32, pcm16=True)
    kw = dict(silence_db=fin.silence_db, trim=3, keep=80, max_gain_db=fin.max_gain_db, fade_in=32, fade_out=32, pcm16=True)
    w24 = G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12)
    w16 = e.resample([w24], 24000, 16000)[0]
    want16 = e.finish_loud([w16], 16000, -16.0, -1.0, **kw)[0][0]
    want24 = e.finish_loud([w24], 24000, -16.0, -1.0, **kw)[0][0]
    assert want16.dtype == np.int16
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, sample_rate=16000, finish=fin), want16)
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, finish=fin), want24)
    _same(G.generate_audio_batch([ids], language="en", uniforms=us[:, None], force_eos_at=12, sample_rate=16000, finish=fin)[0], want16)
    _same(G.generate_audio_from_long_text([ids], language="en", uniforms=us, force_eos_at=12, sample_rate=16000, finish=fin), want16)
    with G.AudioServer(sample_rate=16000, finish=fin, force_eos_at=12) as srv:
        s16 = srv.submit(ids, language="en", seed=9).result()
    with G.AudioServer(force_eos_at=12) as srv:
        s24 = srv.submit(ids, language="en", seed=9).result()
    _same(s16, e.finish_loud(e.resample([s24], 24000, 16000), 16000, -16.0, -1.0, **kw)[0][0])

    # tokenize_audio(..., lufs=-20) hands the tokenizer the levelled clip, after the trim
    seen = []

    class Tok:
        sample_rate = 24000

        def encode(self, w):
            seen.append(np.array(w))
            return [(np.zeros((1, 8, 1), np.int64), None)]

    x = FR.row(9000, 240, 3000, 2700, np.random.default_rng(7))
    PM.tokenize_audio(Tok(), (x[None], 24000), lufs=-20)
    PM.tokenize_audio(Tok(), (x[None], 24000), trim_db=-40, lufs=-20)
    PM.tokenize_audio(Tok(), (x[None], 24000))
    assert seen[0].shape == (1, 1, 9000) and seen[1].shape == (1, 1, 8400) and seen[0].dtype == np.float32
    _same(seen[0][0, 0], e.finish_loud([x], 24000, -20.0, PM.PROMPT_CEILING_DB)[0][0])
    _same(seen[1][0, 0], e.finish_loud([x[480:8880]], 24000, -20.0, PM.PROMPT_CEILING_DB)[0][0])
    _same(seen[2][0, 0], x)
    assert abs(e.loudness([seen[1][0, 0]], 24000)[0]["loudness"] - (-20.0)) <= 1e-4


def test_nothing_else_moves():
    """greedy ids of nl2_greedy_eos before and after interleaved loudness calls; a call while a serving session is open succeeds and
    the session's result is what it is without the call; no fallback is counted"""
    from tests._util import case_row, get_model, golden
    c, row, _ = case_row("nl2_greedy_eos")
    m = get_model(c["num_layers"], c["seed"], c["eos_gain"], vocos=True)
    e = m.engine
    x = R.rows(8000)[9]
    kw = dict(trim=3, fade_in=7, fade_out=7, pcm16=True)
    before = m.inference_batch([row], top_k=1, force_eos_at=c["force_eos_at"])[0]
    r1 = e.finish_loud([x], 8000, -16.0, **kw)[0][0].copy()
    l1 = e.loudness([x], 8000)[0]
    after = m.inference_batch([row], top_k=1, force_eos_at=c["force_eos_at"])[0]
    np.testing.assert_array_equal(before, golden("nl2_greedy_eos")["codes"][0])
    np.testing.assert_array_equal(after, before)
    fb = e.last_fallbacks()
    e.finish_loud([x], 8000, -23.0)
    e.loudness([x], 8000)
    assert e.last_fallbacks() == fb
    _same_linfo(l1, R.measure(x, 8000, e.loudness_coeffs(8000)), "finalized context")

    def session(interleave):
        got = {}
        with e.serve(top_k=10, force_eos_at=30) as sess:
            ids = sess.submit(m.make_batch([row, row]), [dict(seed=5), dict(seed=6, best_of=2)])
            sess.run(3, lambda rid, cd: got.__setitem__(rid, cd))
            if interleave:
                _same(e.finish_loud([x], 8000, -16.0, **kw)[0][0], r1)
                assert _equal_bits(e.loudness([x], 8000)[0], l1)
            sess.run(0, lambda rid, cd: got.__setitem__(rid, cd))
        return [got[i] for i in ids]

    for a, b in zip(session(False), session(True)):
        np.testing.assert_array_equal(a, b)


def test_refusals(eng, data):
    c, rows, _ = data[8000]
    x = rows[8]
    L = len(x)
    kw = dict(silence_db=DB, trim=3, fade_in=7, pcm16=True)
    ok = eng.finish_loud([x], 8000, -16.0, **kw)
    ok_l = eng.last_loudness_info[0]
    lib, ctx = eng.lib, eng.ctx
    buf = x[None].copy()
    ln = np.array([L], np.int32)
    out = np.full((1, L), FR.SENT_H, np.int16)
    ol = np.full(1, -7, np.int32)
    info, linfo = (_capi.vx_wave_info * 1)(), (_capi.vx_loudness_info * 1)()
    info[0].begin = -9
    linfo[0].blocks = -9
    fp, ip, vp = lambda a: _ptr(a, C.c_float), lambda a: _ptr(a, C.c_int32), lambda a: a.ctypes.data_as(C.c_void_p)

    def fopts(**f):
        o = dict(FR.DEFAULTS, **kw)
        s = _capi.vx_finish_opts(C.sizeof(_capi.vx_finish_opts), 80, o["silence_db"], o["trim"], o["keep"], 0, o["level_db"], o["max_gain_db"],
                                 o["fade_in"], o["fade_out"], _capi.PCM_S16)
        for k, v in f.items():
            setattr(s, k, v)
        return s

    def lopts(**f):
        s = _capi.vx_loudness_opts(C.sizeof(_capi.vx_loudness_opts), 8000, -16.0, -1.0)
        for k, v in f.items():
            setattr(s, k, v)
        return s

    def refused(field, *args):
        rc = lib.vx_finish_loud(ctx, *args)
        msg = lib.vx_last_error(ctx).decode()
        assert rc == VX_EINVAL and field in msg and "vx_finish_loud" in msg, (field, rc, msg)
        assert (out == FR.SENT_H).all() and ol[0] == -7 and info[0].begin == -9 and linfo[0].blocks == -9, field      # nothing written

    o, lo = C.byref(fopts()), C.byref(lopts())
    refused("wav", None, L, ip(ln), 1, o, lo, vp(out), L, ip(ol), info, linfo)
    refused("lens", fp(buf), L, None, 1, o, lo, vp(out), L, ip(ol), info, linfo)
    refused("o is NULL", fp(buf), L, ip(ln), 1, None, lo, vp(out), L, ip(ol), info, linfo)
    refused("lo is NULL", fp(buf), L, ip(ln), 1, o, None, vp(out), L, ip(ol), info, linfo)
    refused("info", fp(buf), L, ip(ln), 1, o, lo, vp(out), L, ip(ol), None, linfo)
    refused("linfo", fp(buf), L, ip(ln), 1, o, lo, vp(out), L, ip(ol), info, None)
    refused("out_lens", fp(buf), L, ip(ln), 1, o, lo, vp(out), L, None, info, linfo)
    assert lib.vx_finish_loud(None, fp(buf), L, ip(ln), 1, o, lo, vp(out), L, ip(ol), info, linfo) == VX_EINVAL
    refused("batch", fp(buf), L, ip(ln), 0, o, lo, vp(out), L, ip(ol), info, linfo)
    refused("lens[0]", fp(buf), L, ip(np.array([-1], np.int32)), 1, o, lo, vp(out), L, ip(ol), info, linfo)
    refused("wav_stride", fp(buf), L, ip(np.array([L + 1], np.int32)), 1, o, lo, vp(out), L, ip(ol), info, linfo)
    refused("out_stride", fp(buf), L, ip(ln), 1, o, lo, vp(out), L - 1, ip(ol), info, linfo)
    refused("vx_finish_opts.struct_size", fp(buf), L, ip(ln), 1, C.byref(fopts(struct_size=40)), lo, vp(out), L, ip(ol), info, linfo)
    refused("vx_loudness_opts.struct_size", fp(buf), L, ip(ln), 1, o, C.byref(lopts(struct_size=12)), vp(out), L, ip(ol), info, linfo)
    nan, inf = float("nan"), float("inf")
    for field, bad in (("level_mode", 1), ("level_mode", 2), ("level_mode", 3), ("frame", 15), ("silence_db", 0.5), ("trim", 4), ("keep", -1),
                       ("max_gain_db", -0.5), ("max_gain_db", nan), ("fade_in", -1), ("fade_out", (1 << 20) + 1), ("format", 2)):
        b = C.byref(fopts(**{field: bad}))
        refused(field, fp(buf), L, ip(ln), 1, b, lo, vp(out), L, ip(ol), info, linfo)
        refused(field, fp(buf), L, ip(ln), 1, b, lo, None, L, None, info, linfo)        # checked in a measure-only call too
    for field, bad in (("sample_rate", 7999), ("sample_rate", 192001), ("sample_rate", 0), ("target_lufs", 0.5), ("target_lufs", -70.5),
                       ("target_lufs", nan), ("target_lufs", -inf), ("ceiling_db", 0.5), ("ceiling_db", nan), ("ceiling_db", -inf)):
        refused(field, fp(buf), L, ip(ln), 1, o, C.byref(lopts(**{field: bad})), vp(out), L, ip(ol), info, linfo)
    for edge in (dict(sample_rate=192000), dict(target_lufs=0.0), dict(target_lufs=-70.0), dict(ceiling_db=0.0)):
        assert lib.vx_finish_loud(ctx, fp(buf), L, ip(ln), 1, o, C.byref(lopts(**edge)), None, L, None, (_capi.vx_wave_info * 1)(),
                                  (_capi.vx_loudness_info * 1)()) == 0, edge

    # vx_loudness
    def refused_l(field, *args):
        rc = lib.vx_loudness(ctx, *args)
        msg = lib.vx_last_error(ctx).decode()
        assert rc == VX_EINVAL and field in msg and "vx_loudness" in msg, (field, rc, msg)
        assert linfo[0].blocks == -9, field

    refused_l("wav", None, L, ip(ln), 1, 8000, linfo)
    refused_l("lens", fp(buf), L, None, 1, 8000, linfo)
    refused_l("info", fp(buf), L, ip(ln), 1, 8000, None)
    refused_l("batch", fp(buf), L, ip(ln), 0, 8000, linfo)
    refused_l("lens[0]", fp(buf), L, ip(np.array([-1], np.int32)), 1, 8000, linfo)
    refused_l("wav_stride", fp(buf), L, ip(np.array([L + 1], np.int32)), 1, 8000, linfo)
    for bad in (7999, 192001, 0, -8000):
        refused_l("sample_rate", fp(buf), L, ip(ln), 1, bad, linfo)
    assert lib.vx_loudness(None, fp(buf), L, ip(ln), 1, 8000, linfo) == VX_EINVAL
    cc = np.full(10, -7.0)
    assert lib.vx_loudness_coeffs(7999, _ptr(cc, C.c_double)) == VX_EINVAL and lib.vx_loudness_coeffs(192001, _ptr(cc, C.c_double)) == VX_EINVAL
    assert lib.vx_loudness_coeffs(8000, None) == VX_EINVAL and (cc == -7.0).all()
    with pytest.raises(VallexHipError) as ei:
        eng.dev_loudness_steps(x, 7999)
    assert ei.value.code == VX_EINVAL and "sample_rate" in str(ei.value)
    with pytest.raises(VallexHipError) as ei:
        eng.finish_loud([x], 8000, 1.0)
    assert ei.value.code == VX_EINVAL and "target_lufs" in str(ei.value)
    with pytest.raises(ValueError):
        eng.loudness_coeffs(100)
    # the context still levels, to the same bits
    assert lib.vx_finish_loud(ctx, fp(buf), L, ip(ln), 1, o, lo, vp(out), L, ip(ol), info, linfo) == 0
    assert ol[0] == len(ok[0][0]) and (out[0, ol[0]:] == FR.SENT_H).all() and info[0].begin == ok[1][0]["begin"]
    np.testing.assert_array_equal(out[0, : ol[0]], ok[0][0])
    assert _equal_bits({f[0]: getattr(linfo[0], f[0]) for f in _capi.vx_loudness_info._fields_}, ok_l)
