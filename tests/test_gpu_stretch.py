"""GPU: the speaking rate (vx_stretch, csrc/stretch.hip) against tests/_stretch_refs.py, the numpy restatement of the header's contract.

Everything is compared word for word: outputs, positions and the winning cost of every frame as doubles.  Nothing goes through a
transcendental or a library that could differ, so there is no tolerance anywhere.  One un-finalized context serves the kernel
tests: the entry needs no weights.  The restatement of every case is computed once and shared."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests import _stretch_refs as R
from vallex_amd import _capi
from vallex_amd._capi import VX_EINVAL, Engine, VallexHipError, _ptr

pytestmark = pytest.mark.gpu

SENT_F = np.float32(-1.0e30)
SENT_I = -123456789


@pytest.fixture(scope="module")
def eng():
    e = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)      # created, never finalized
    yield e
    e.close()


@pytest.fixture(scope="module")
def ref():
    """per hop: the nine rows (the eight lengths and the non-finite one) and, per case (search, speed), the restatement of each"""
    d = {}
    for H in R.HOPS:
        rows = R.rows(H) + [R.hot_row()]
        d[H] = (rows, {(D, sp): [R.stretch(x, sp[0], sp[1], H, D) for x in rows] for D, sp in R.cases(H)})
    return d


def _opts(num, den, H, D):
    return _capi.vx_stretch_opts(C.sizeof(_capi.vx_stretch_opts), num, den, H, D)


def _raw(eng, rows, num, den, H, D, pad=5):
    """vx_stretch on sentinel-filled outputs: (rc, message, out (n, stride + pad), out_lens, pos (n, pstride + pad))"""
    n = len(rows)
    ln = np.array([len(r) for r in rows], np.int32)
    ws = max(1, int(ln.max()))
    buf = np.zeros((n, ws), np.float32)
    for i, r in enumerate(rows):
        buf[i, : len(r)] = r
    os_ = max(1, R.out_len(ws, num, den))
    ps = max(1, -(-os_ // H))
    out = np.full((n, os_ + pad), SENT_F, np.float32)
    pos = np.full((n, ps + pad), SENT_I, np.int32)
    ol = np.full(n, -7, np.int32)
    o = _opts(num, den, H, D)
    rc = eng.lib.vx_stretch(eng.ctx, _ptr(buf, C.c_float), ws, _ptr(ln, C.c_int32), n, C.byref(o), _ptr(out, C.c_float), os_ + pad,
                            _ptr(ol, C.c_int32), _ptr(pos, C.c_int32), ps + pad)
    return rc, eng.lib.vx_last_error(eng.ctx).decode(), out, ol, pos


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    view = {4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize]
    np.testing.assert_array_equal(a.view(view), b.view(view), err_msg=str(what))


@pytest.mark.parametrize("H", R.HOPS)
def test_kernel_word_for_word_alone_and_as_one_ragged_batch(eng, ref, H):
    rows, cases = ref[H]
    assert {D for D, _ in cases} == set(R.SEARCHES) and {sp for _, sp in cases} == set(R.SPEEDS)
    assert [len(x) for x in rows] == [0, 1, H - 1, H, H + 1, 3 * H + 7, 4801, 13001, 4801] and not np.isfinite(rows[8]).all()
    moved = 0
    for (D, (num, den)), want in cases.items():
        what = f"H {H} D {D} speed {num}/{den}"
        for x, (out, pos, cost) in zip(rows, want):
            gout, gpos, gcost = eng.dev_stretch_costs(x, (num, den), H, D)
            _same(gpos, pos.astype(np.int32), (what, len(x), "pos"))
            _same(gcost, cost, (what, len(x), "cost"))                   # the winning D of every frame, as doubles
            _same(gout, out, (what, len(x), "out"))
            assert np.isfinite(gout).all()
            moved += int((pos != np.array([R.nominal(k, num, den, H) for k in range(len(pos))])).sum())
        rc, msg, bout, ol, bpos = _raw(eng, rows, num, den, H, D)          # all rows as one ragged batch
        assert rc == 0, msg
        rc, msg, bout2, ol2, bpos2 = _raw(eng, rows, num, den, H, D)       # two calls give the same bits
        assert rc == 0, msg
        _same(bout2, bout, what)
        _same(bpos2, bpos, what)
        assert ol.tolist() == ol2.tolist() == [len(w[0]) for w in want]
        for i, (out, pos, _) in enumerate(want):
            _same(bout[i, : len(out)], out, (what, "batch row", i))
            _same(bpos[i, : len(pos)], pos.astype(np.int32), (what, "batch row", i))
            assert (bout[i, len(out):] == SENT_F).all() and (bpos[i, len(pos):] == SENT_I).all(), (what, i)     # nothing behind the ends
        assert (bout[0] == SENT_F).all() and (bpos[0] == SENT_I).all() and ol[0] == 0                            # the zero-length row
        if D in (5, 300):
            for i in (5, 7, 8):                                            # Engine.stretch on a row alone
                w, p = eng.stretch([rows[i]], Fraction(num, den), H, D, return_positions=True)
                _same(w[0], want[i][0], (what, "alone", i))
                _same(p[0], want[i][1].astype(np.int32), (what, "alone", i))
    assert moved > 100                                                     # the search did move frames off their nominal positions


def test_windows(eng, ref):
    """a long row cut into windows, each started from the position the launch before found: the bits of one pass"""
    try:
        for H, D, sp in ((240, 150, (4, 5)), (441, 300, (5, 4)), (16, 5, (2, 3)), (441, 300, (1000, 999))):
            rows, cases = ref[H]
            want = cases[(D, sp)]
            for win in (_capi.DEV_STRETCH_WINDOW_MIN, 7777):
                eng.dev_stretch_window(win)
                for i in (6, 7, 8):
                    out, pos, cost = eng.dev_stretch_costs(rows[i], sp, H, D)
                    _same(out, want[i][0], (H, D, sp, win, i))
                    _same(pos, want[i][1].astype(np.int32), (H, D, sp, win, i))
                    _same(cost, want[i][2], (H, D, sp, win, i))
                rc, msg, bout, ol, bpos = _raw(eng, rows, sp[0], sp[1], H, D)
                assert rc == 0, msg
                for i, (out, pos, _) in enumerate(want):
                    _same(bout[i, : len(out)], out, (H, D, sp, win, "batch row", i))
                    _same(bpos[i, : len(pos)], pos.astype(np.int32), (H, D, sp, win, "batch row", i))
                    assert (bout[i, len(out):] == SENT_F).all() and (bpos[i, len(pos):] == SENT_I).all()
        # one frame's span above the window: refused, naming the entry that set it
        eng.dev_stretch_window(_capi.DEV_STRETCH_WINDOW_MIN)
        with pytest.raises(VallexHipError) as ei:
            eng.stretch([ref[240][0][7]], (4, 5), 2048, 1024)
        assert ei.value.code == VX_EINVAL and "vx_dev_stretch_window" in str(ei.value)
        for bad in (1, _capi.DEV_STRETCH_WINDOW_MIN - 1, -5, _capi.STRETCH_WINDOW + 1):
            with pytest.raises(VallexHipError) as ei:
                eng.dev_stretch_window(bad)
            assert ei.value.code == VX_EINVAL and "input_samples" in str(ei.value)
    finally:
        eng.dev_stretch_window(0)                                          # 0 restores the default
    rows, cases = ref[240]
    w = eng.stretch([rows[7], rows[8]], (4, 5), 240, 150)
    _same(w[0], cases[(150, (4, 5))][7][0])
    _same(w[1], cases[(150, (4, 5))][8][0])


def test_largest_options(eng):
    """hop 2048, search 1024: the 24-register prefetch, the largest LDS layout"""
    x = R.rows(240)[7]
    out, pos, cost = R.stretch(x, 3, 2, 2048, 1024)
    gout, gpos, gcost = eng.dev_stretch_costs(x, (3, 2), 2048, 1024)
    _same(gout, out)
    _same(gpos, pos.astype(np.int32))
    _same(gcost, cost)


def test_speed_one(eng, ref):
    rows, _ = ref[240]
    for num, den in ((1, 1), (7, 7), (32767, 32767)):
        rc, msg, out, ol, pos = _raw(eng, rows, num, den, 240, 150)
        assert rc == 0, msg
        for i, x in enumerate(rows):
            M = -(-len(x) // 240)
            assert ol[i] == len(x) and pos[i, :M].tolist() == [240 * k for k in range(M)]
            _same(out[i, : len(x)], x)                                     # the input bits, NaN and Inf included
            assert (out[i, len(x):] == SENT_F).all() and (pos[i, M:] == SENT_I).all()
    # ... and the general path agrees by its arithmetic: the self-match wins
    x = rows[7]
    out, pos, cost = eng.dev_stretch_costs(x, (1, 1), 240, 150)
    rout, rpos, rcost = R.stretch(x, 1, 1, 240, 150, shortcut=False)
    _same(out, rout)
    _same(pos, rpos.astype(np.int32))
    _same(cost, rcost)
    _same(out, x)
    assert pos.tolist() == [240 * k for k in range(len(pos))]


def _golden_codes12():
    from tests._util import golden
    codes = golden("nl2_bestof3")["codes"][0].astype(np.int64)
    assert codes.shape == (12, 8)
    return codes


def test_vocos_decode_at_a_speed():
    from tests._util import get_model
    from vallex_amd.utils.generation import Finish
    m = get_model(2, 0, 2.5, vocos=True)
    e = m.engine
    codes = [_golden_codes12(), _golden_codes12()[:5]]
    w24 = [w.copy() for w in e.vocos_decode(codes, 2)]
    for a, b in zip(e.vocos_decode(codes, 2, speed=None), w24):            # without the argument: a plain call
        _same(a, b)
    fin = Finish(trim=3, keep=40, level_mode=2, level_db=-20.0, fade_in=16, fade_out=16, pcm16=True)
    sp = Fraction(5, 4)
    st = e.stretch(w24, sp)
    for x, a in zip(w24, st):                                              # the stretch is the restatement's (hop 240, search 150)
        _same(a, R.stretch(x, 5, 4, 240, 150)[0])
    assert [len(a) for a in st] == [3072, 1280]
    want = e.finish(e.resample(st, 24000, 16000), 160, fin.silence_db, fin.trim, fin.keep, fin.level_mode, fin.level_db, fin.max_gain_db,
                    fin.fade_in, fin.fade_out, fin.pcm16)[0]
    got = e.vocos_decode(codes, 2, speed=sp, sample_rate=16000, finish=fin)
    for a, b in zip(got, want):
        _same(a, b)
        assert a.dtype == np.int16
    for a, b in zip(e.vocos_decode(codes, 2, speed=0.8), e.stretch(w24, (4, 5))):       # a float; 24 kHz, no output stage
        _same(a, b)
    for a, b in zip(e.vocos_decode(codes, 2, speed=(1, 1)), w24):
        _same(a, b)


def test_encodec_decode_at_a_speed():
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
    kw = {k: getattr(fin, k) for k in ("silence_db", "trim", "keep", "level_mode", "level_db", "max_gain_db", "fade_in", "fade_out", "pcm16")}
    w24 = e.encodec_decode(codes)
    _same(e.encodec_decode(codes, speed=None)[0], w24[0])
    st = e.stretch(w24, (4, 5))
    _same(st[0], R.stretch(w24[0], 4, 5, 240, 150)[0])
    _same(e.encodec_decode(codes, speed=Fraction(4, 5))[0], st[0])
    _same(e.encodec_decode(codes, speed=Fraction(4, 5), sample_rate=48000, finish=fin)[0],
          e.finish(e.resample(st, 24000, 48000), 480, **kw)[0][0])


def test_generate_audio_family_at_a_speed():
    from oracle import synth
    from vallex_amd.utils import generation as G
    G.preload_models(state_dict=synth.vallex_state_dict(2, 11), vocos_state_dict=synth.vocos_state_dict(2), num_layers=2, max_new=64,
                     max_prompt=128, max_text=64, max_batch=2)
    e = G.model.engine
    ids = synth.synth_text(6, 1)
    us = synth.uniforms(32, 1, 5)[:, 0]
    fin = G.Finish(trim=3, keep=80, level_mode=2, level_db=-20.0, fade_in=32, fade_out=32, pcm16=True)
    kw = {k: getattr(fin, k) for k in ("silence_db", "trim", "keep", "level_mode", "level_db", "max_gain_db", "fade_in", "fade_out", "pcm16")}
    sp = Fraction(5, 4)
    w24 = G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12)
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, speed=None), w24)
    st = e.stretch([w24], sp)[0]
    _same(st, R.stretch(w24, 5, 4, 240, 150)[0])
    want24 = st
    want16 = e.finish(e.resample([st], 24000, 16000), 160, **kw)[0][0]
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, speed=sp), want24)
    _same(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, speed=sp, sample_rate=16000, finish=fin), want16)
    _same(G.generate_audio_batch([ids], language="en", uniforms=us[:, None], force_eos_at=12, speed=sp, sample_rate=16000, finish=fin)[0], want16)
    _same(G.generate_audio_batch([ids], language="en", uniforms=us[:, None], force_eos_at=12, speed=sp)[0], want24)
    _same(G.generate_audio_from_long_text([ids], language="en", uniforms=us, force_eos_at=12, speed=sp, sample_rate=16000, finish=fin), want16)
    with G.AudioServer(sample_rate=16000, finish=fin, speed=sp, force_eos_at=12) as srv:
        s16 = srv.submit(ids, language="en", seed=9).result()
    with G.AudioServer(force_eos_at=12) as srv:
        s24 = srv.submit(ids, language="en", seed=9).result()
    assert s24.dtype == np.float32
    _same(s16, e.finish(e.resample(e.stretch([s24], sp), 24000, 16000), 160, **kw)[0][0])


def test_nothing_else_moves():
    """greedy ids of nl2_greedy_eos before and after interleaved stretch calls; a stretch call while a serving session is open succeeds
    and the session's result is what it is without the call; no fallback is counted"""
    from tests._util import case_row, get_model, golden
    c, row, _ = case_row("nl2_greedy_eos")
    m = get_model(c["num_layers"], c["seed"], c["eos_gain"], vocos=True)
    e = m.engine
    x = R.rows(240)[6]
    want = R.stretch(x, 4, 5, 240, 150)[0]
    before = m.inference_batch([row], top_k=1, force_eos_at=c["force_eos_at"])[0]
    fb = e.last_fallbacks()
    r1 = e.stretch([x], (4, 5))[0].copy()
    assert e.last_fallbacks() == fb
    after = m.inference_batch([row], top_k=1, force_eos_at=c["force_eos_at"])[0]
    np.testing.assert_array_equal(before, golden("nl2_greedy_eos")["codes"][0])
    np.testing.assert_array_equal(after, before)
    _same(r1, want)

    def session(interleave):
        got = {}
        with e.serve(top_k=10, force_eos_at=30) as sess:
            ids = sess.submit(m.make_batch([row, row]), [dict(seed=5), dict(seed=6, best_of=2)])
            sess.run(3, lambda rid, cd: got.__setitem__(rid, cd))
            if interleave:
                _same(e.stretch([x], (4, 5))[0], want)
            sess.run(0, lambda rid, cd: got.__setitem__(rid, cd))
        return [got[i] for i in ids]

    for a, b in zip(session(False), session(True)):
        np.testing.assert_array_equal(a, b)


def test_refusals(eng):
    H, D = 16, 5
    x = R.rows(H)[5]
    L = len(x)
    Lout, M = R.out_len(L, 4, 5), R.frames(L, 4, 5, H)
    ok = eng.stretch([x], (4, 5), H, D, return_positions=True)
    lib, ctx = eng.lib, eng.ctx
    buf = x[None].copy()
    ln = np.array([L], np.int32)
    out = np.full((1, Lout), SENT_F, np.float32)
    pos = np.full((1, M), SENT_I, np.int32)
    ol = np.full(1, -7, np.int32)
    fp, ip = lambda a: _ptr(a, C.c_float), lambda a: _ptr(a, C.c_int32)
    good = _opts(4, 5, H, D)

    def refused(field, *args):
        rc = lib.vx_stretch(ctx, *args)
        msg = lib.vx_last_error(ctx).decode()
        assert rc == VX_EINVAL and field in msg and "vx_stretch" in msg, (field, rc, msg)
        assert (out == SENT_F).all() and ol[0] == -7 and (pos == SENT_I).all(), field      # nothing launched, nothing written

    o = C.byref(good)
    refused("wav", None, L, ip(ln), 1, o, fp(out), Lout, ip(ol), ip(pos), M)
    refused("lens", fp(buf), L, None, 1, o, fp(out), Lout, ip(ol), ip(pos), M)
    refused("o is NULL", fp(buf), L, ip(ln), 1, None, fp(out), Lout, ip(ol), ip(pos), M)
    refused("out is NULL", fp(buf), L, ip(ln), 1, o, None, Lout, ip(ol), ip(pos), M)
    refused("out_lens", fp(buf), L, ip(ln), 1, o, fp(out), Lout, None, ip(pos), M)
    assert lib.vx_stretch(None, fp(buf), L, ip(ln), 1, o, fp(out), Lout, ip(ol), ip(pos), M) == VX_EINVAL
    refused("batch", fp(buf), L, ip(ln), 0, o, fp(out), Lout, ip(ol), ip(pos), M)
    refused("batch", fp(buf), L, ip(ln), -1, o, fp(out), Lout, ip(ol), ip(pos), M)
    refused("lens[0]", fp(buf), L, ip(np.array([-1], np.int32)), 1, o, fp(out), Lout, ip(ol), ip(pos), M)
    refused("wav_stride", fp(buf), L, ip(np.array([L + 1], np.int32)), 1, o, fp(out), Lout, ip(ol), ip(pos), M)
    refused("out_stride", fp(buf), L, ip(ln), 1, o, fp(out), Lout - 1, ip(ol), ip(pos), M)
    refused("pos_stride", fp(buf), L, ip(ln), 1, o, fp(out), Lout, ip(ol), ip(pos), M - 1)
    short = _opts(4, 5, H, D)
    short.struct_size -= 4
    refused("struct_size", fp(buf), L, ip(ln), 1, C.byref(short), fp(out), Lout, ip(ol), ip(pos), M)
    for field, bad in (("hop", 15), ("hop", 2049), ("search", -1), ("search", 1025), ("speed_num", 0), ("speed_num", 32768),
                       ("speed_den", 0), ("speed_den", 32768), ("speed_den", -3)):
        b = _opts(4, 5, H, D)
        setattr(b, field, bad)
        refused(field, fp(buf), L, ip(ln), 1, C.byref(b), fp(out), Lout, ip(ol), ip(pos), M)
    for num, den in ((1, 3), (3, 1), (999, 2000), (2001, 1000)):
        refused("speed_num / speed_den", fp(buf), L, ip(ln), 1, C.byref(_opts(num, den, H, D)), fp(out), Lout, ip(ol), ip(pos), M)
    for bad in (dict(speed=(1, 3)), dict(speed=2.5), dict(speed=(4, 5), hop=8), dict(speed=(4, 5), search=2000)):
        with pytest.raises(VallexHipError) as ei:
            eng.stretch([x], **bad)
        assert ei.value.code == VX_EINVAL
    with pytest.raises(VallexHipError) as ei:
        eng.dev_stretch_costs(x, (4, 5), 15, 5)
    assert ei.value.code == VX_EINVAL and "hop" in str(ei.value)
    # a pos of NULL is allowed; the context still stretches, to the same bits
    assert lib.vx_stretch(ctx, fp(buf), L, ip(ln), 1, o, fp(out), Lout, ip(ol), None, 0) == 0
    assert ol[0] == Lout and (pos == SENT_I).all()
    _same(out[0], ok[0][0])
    assert lib.vx_stretch(ctx, fp(buf), L, ip(ln), 1, o, fp(out), Lout, ip(ol), ip(pos), M) == 0
    _same(pos[0], ok[1][0])
    _same(out[0], R.stretch(x, 4, 5, H, D)[0])
