"""GPU: the three output-stage entries (vx_finish, vx_finish_loud, vx_finish_limited) side by side -- what they refuse, word for word,
and what they compute in every cell of (entry x one launch / several launches x output / measure-only).

The messages are the literal texts of the entries' checks, one fault per call.  The outputs and infos of a call that goes through
several launches of every pass (development windows of 512 / 4096 / 8192 samples) are the words of the one-launch call; those are the
numpy restatements' (tests/_finish_refs.py, _loudness_refs.py, _limit_refs.py) at the tolerance their own tests use: exact bits,
except a gain (pow on the host, 1 fp32 ulp; the outputs are compared at the gain the call reported) and a loudness (log10, 1e-12)."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import _finish_refs as FR
from tests import _limit_refs as MR
from tests import _loudness_refs as LR
from vallex_amd import _capi
from vallex_amd._capi import VX_EINVAL, Engine, _ptr

pytestmark = pytest.mark.gpu

ENTRIES = ("vx_finish", "vx_finish_loud", "vx_finish_limited")
RATE, F, DB, LUFS = 8000, 80, -40.0, -3.0
KW = dict(silence_db=DB, trim=3, keep=33, fade_in=7, fade_out=7)
WINDOWS = (("dev_finish_window", 512), ("dev_loudness_window", 4096), ("dev_limit_window", 8192))
INFO_TYPES = (_capi.vx_wave_info, _capi.vx_loudness_info, _capi.vx_limit_info)


def _engine():
    return Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)      # created, never finalized


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def rows():
    """0, 1, 79, 9000 and 20011 samples of the limiter tests' voice, the two long rows with a lead and a tail 60 dB down (trim = 3 cuts
    them); a NaN (in the lead) and an Inf in the 9000-sample row"""
    out = [MR.voice(L, RATE, 40 + i, 0.6) for i, L in enumerate((0, 1, 79, 9000, 20011))]
    out[3][5], out[3][4000] = np.nan, np.inf
    for x, a, b in ((out[3], 1003, 517), (out[4], 2005, 1501)):
        x[:a] *= np.float32(1e-3)
        x[len(x) - b:] *= np.float32(1e-3)
    for x in out:
        assert FR.margin(x, F, DB) >= 0.25
    return out


def _call(eng, entry, rows, rate=RATE, out=True, pad=5, **kw):
    """one entry on a sentinel-filled out: (rc, message, out (n, stride + pad), out_lens, (wave, loudness, limiter) info dicts).
    kw: finish options, or overrides of what the call passes: fo_size / lo_size / lim_size, lens, out_stride, no_out_lens, batch."""
    n = len(rows)
    ln = np.array(kw.pop("lens", [len(r) for r in rows]), np.int32)
    ws = max(1, max(len(r) for r in rows))
    buf = np.zeros((n, ws), np.float32)
    for i, r in enumerate(rows):
        buf[i, : len(r)] = r
    sizes = [kw.pop(k, C.sizeof(t)) for k, t in (("fo_size", _capi.vx_finish_opts), ("lo_size", _capi.vx_loudness_opts), ("lim_size", _capi.vx_limit_opts))]
    ostride, batch, no_out_lens = kw.pop("out_stride", ws + pad), kw.pop("batch", n), kw.pop("no_out_lens", False)
    o = dict(FR.DEFAULTS, **kw)
    pcm16 = o["pcm16"]
    outa = np.full((n, ws + pad), FR.SENT_H if pcm16 else FR.SENT_F, np.int16 if pcm16 else np.float32)
    ol = np.full(n, -7, np.int32)
    infos = [(t * n)() for t in INFO_TYPES]
    fo = _capi.vx_finish_opts(sizes[0], rate // 100, o["silence_db"], o["trim"], o["keep"], o["level_mode"], o["level_db"], o["max_gain_db"],
                              o["fade_in"], o["fade_out"], _capi.PCM_S16 if pcm16 else _capi.PCM_F32)
    lo = _capi.vx_loudness_opts(sizes[1], rate, LUFS, -1.0)
    lim = _capi.vx_limit_opts(sizes[2], rate // 200, 4)
    k = ENTRIES.index(entry)
    args = [eng.ctx, _ptr(buf, C.c_float), ws, _ptr(ln, C.c_int32), batch, C.byref(fo)] + [C.byref(lo), C.byref(lim)][:k]
    args += [outa.ctypes.data_as(C.c_void_p) if out else None, ostride, None if no_out_lens else _ptr(ol, C.c_int32)] + infos[: k + 1]
    rc = getattr(eng.lib, entry)(*args)
    dicts = tuple([{f[0]: getattr(w, f[0]) for f in t._fields_} for w in a] for t, a in zip(INFO_TYPES[: k + 1], infos))
    return rc, eng.lib.vx_last_error(eng.ctx).decode(), outa, ol, dicts


def _words(v):
    return np.float64(v).view(np.uint64) if isinstance(v, float) else v


def _same_dicts(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert {k: _words(v) for k, v in x.items()} == {k: _words(v) for k, v in y.items()}, (what, x, y)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.int16 else np.uint32)


# ---- messages ------------------------------------------------------------------------------------------------------------------------

def _refused(eng, entry, want, **kw):
    x = [MR.noise(100, 1), MR.noise(200, 2)]
    rc, msg, outa, _, _ = _call(eng, entry, x, **kw)
    assert rc == VX_EINVAL and msg == want, (entry, kw, rc, msg, want)
    assert (outa == FR.SENT_F).all()


@pytest.mark.parametrize("entry", ENTRIES)
def test_messages_word_for_word(eng, entry):
    who = entry + ": "
    size = "%s.struct_size is 7, this library expects %d (ABI version 6)"
    # vx_finish names the struct alone, the two others put their name in front
    _refused(eng, entry, ("" if entry == "vx_finish" else who) + size % ("vx_finish_opts", C.sizeof(_capi.vx_finish_opts)), fo_size=7)
    if entry != "vx_finish":
        _refused(eng, entry, who + size % ("vx_loudness_opts", C.sizeof(_capi.vx_loudness_opts)), lo_size=7)
        _refused(eng, entry, who + "level_mode 1 is not VX_LEVEL_NONE: the loudness target sets the level", level_mode=_capi.LEVEL_PEAK)
    if entry == "vx_finish_limited":
        _refused(eng, entry, who + size % ("vx_limit_opts", C.sizeof(_capi.vx_limit_opts)), lim_size=7)
    _refused(eng, entry, who + "lens[1] = 201 outside 0 .. wav_stride 200", lens=[100, 201])
    _refused(eng, entry, who + "out_stride 199 below the 200 samples of row 1 (its untrimmed length)", out_stride=199)
    _refused(eng, entry, who + "out is given without out_lens", no_out_lens=True)
    _refused(eng, entry, who + "batch 0 below 1", batch=0)
    rc, msg, _, _, _ = _call(eng, entry, [MR.noise(100, 1), MR.noise(200, 2)])
    assert rc == 0, msg


@pytest.mark.parametrize("entry", ENTRIES[1:])
def test_window_below_three_steps(eng, entry):
    """3 S = 4800 samples at 16 kHz do not fit a steps window of 4096"""
    try:
        eng.dev_loudness_window(4096)
        _refused(eng, entry, entry + ": the launch window of 4096 samples (vx_dev_loudness_window) is below 3 S = 4800 at sample_rate 16000",
                 rate=16000)
        rc, msg, _, _, _ = _call(eng, entry, [MR.noise(100, 1), MR.noise(200, 2)], rate=8000)
        assert rc == 0, msg
    finally:
        eng.dev_loudness_window(0)


# ---- every cell ----------------------------------------------------------------------------------------------------------------------

def _restated(entry, eng, rows, pcm16, outa, ol, dicts):
    """the one-launch call against the restatements"""
    infos = dicts[0]
    sent = FR.SENT_H if pcm16 else FR.SENT_F
    coef = eng.loudness_coeffs(RATE)
    tp = eng.limit_taps(4)
    for b, x in enumerate(rows):
        gi, what = infos[b], (entry, pcm16, b)
        if entry == "vx_finish":
            want, w = FR.finish(x, F, gain_used=gi["gain"], level_mode=FR.RMS, level_db=-20.0, pcm16=pcm16, **KW)
        else:
            w = FR.measure(x, F, **KW)
            xs = x[w["begin"]:w["end"]]
            z = LR.steps(xs, RATE, coef)
            assert LR.gate_margin_db(z, len(xs), RATE // 10) >= 0.1
            li = LR.measure(xs, RATE, coef, z)
            got = dicts[1][b]
            assert all(got[k] == li[k] for k in ("blocks", "above_abs", "gated", "nonfinite")), (what, got, li)
            assert _words(got["mean_square"]) == _words(li["mean_square"]), (what, got, li)
            for k in ("loudness", "max_momentary"):
                assert got[k] == li[k] if math.isinf(li[k]) else abs(got[k] - li[k]) <= 1e-12, (what, k, got, li)
            if entry == "vx_finish_loud":
                w["gain"] = LR.gain(li["loudness"], LUFS, -1.0, 20.0, w["peak"])
                assert LR.ulp_diff([gi["gain"]], [w["gain"]])[0] <= 1, (what, gi["gain"], w["gain"])
                want, w["clipped"] = FR.apply(x, w["begin"], w["end"], gi["gain"], 7, 7, pcm16)
            else:
                w["gain"] = MR.gain(li["loudness"], LUFS, 20.0)
                assert MR.ulp_diff([gi["gain"]], [w["gain"]])[0] <= 1, (what, gi["gain"], w["gain"])
                mi = dicts[2][b]
                lim = MR.limit(xs, gi["gain"], np.float32(mi["ceiling"]), RATE // 200, 4, tp)
                assert MR.ulp_diff([mi["ceiling"]], [MR.ceiling(-1.0)])[0] <= 1
                for k in ("peak", "min_gain"):
                    assert MR.bits(np.float32(mi[k])) == MR.bits(np.float32(lim[k])), (what, k, mi, lim)
                assert (mi["reduced"], mi["nonfinite"]) == (lim["reduced"], lim["nonfinite"]), (what, mi, lim)
                want, w["clipped"] = FR.apply(lim["out"], 0, len(xs), np.float32(1), 7, 7, pcm16)
        for k in ("begin", "end", "active_frames", "nonfinite", "clipped"):
            assert gi[k] == w[k], (what, k, gi, w)
        assert MR.bits(np.float32(gi["peak"])) == MR.bits(np.float32(w["peak"])) and _words(gi["mean_square"]) == _words(w["mean_square"]), (what, gi, w)
        assert ol[b] == len(want) == w["end"] - w["begin"], what
        np.testing.assert_array_equal(_bits(outa[b, : ol[b]]), _bits(want), err_msg=str(what))
        assert (outa[b, ol[b]:] == sent).all(), what
    assert infos[3]["nonfinite"] == 2 and infos[0]["end"] == 0 and infos[4]["begin"] > 0 and infos[4]["end"] - infos[4]["begin"] > 8192


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_cell(eng, rows, entry):
    """(one launch | several launches of every pass) x (fp32 | int16 | measure-only): the same words; the one-launch words are the
    restatements'"""
    kw = dict(KW, level_mode=FR.RMS, level_db=-20.0) if entry == "vx_finish" else KW
    cells = [dict(pcm16=False), dict(pcm16=True), dict(out=False)]
    one = [_call(eng, entry, rows, **kw, **cell) for cell in cells]
    try:
        for name, w in WINDOWS:
            getattr(eng, name)(w)
        many = [_call(eng, entry, rows, **kw, **cell) for cell in cells]
    finally:
        for name, _ in WINDOWS:
            getattr(eng, name)(0)
    for cell, a, b in zip(cells, one, many):
        assert a[0] == 0 and b[0] == 0, (cell, a[1], b[1])
        np.testing.assert_array_equal(_bits(a[2]), _bits(b[2]), err_msg=str((entry, cell)))
        assert a[3].tolist() == b[3].tolist()
        for da, db in zip(a[4], b[4]):
            _same_dicts(da, db, (entry, cell))
    for cell, r in zip(cells[:2], one[:2]):
        _restated(entry, eng, rows, cell["pcm16"], *r[2:])
    # measure-only: nothing written, out_lens and the infos of the call with an output -- before anything was applied
    rc, _, outa, ol, dicts = one[2]
    assert (outa == FR.SENT_F).all() and ol.tolist() == one[0][3].tolist()
    _same_dicts(dicts[0], [dict(d, clipped=0) for d in one[0][4][0]], (entry, "measure-only"))
    if entry != "vx_finish":
        _same_dicts(dicts[1], one[0][4][1], (entry, "measure-only loudness"))
    if entry == "vx_finish_limited":        # the detector alone ran
        for a, b in zip(dicts[2], one[0][4][2]):
            assert (_words(a["peak"]), a["nonfinite"], _words(a["ceiling"]), a["min_gain"], a["reduced"]) == (_words(b["peak"]), b["nonfinite"], _words(b["ceiling"]), 1.0, 0)


def test_loudness_after_finish_on_a_fresh_engine(rows):
    """vx_finish allocates the launch buffers alone; the loudness tables are still allocated by the first call that needs them"""
    e = _engine()
    try:
        rc, msg, _, _, _ = _call(e, "vx_finish", rows, **KW)
        assert rc == 0, msg
        coef = e.loudness_coeffs(RATE)
        for b, (got, x) in enumerate(zip(e.loudness(rows, RATE), rows)):
            li = LR.measure(x, RATE, coef)
            assert all(got[k] == li[k] for k in ("blocks", "above_abs", "gated", "nonfinite")), (b, got, li)
            assert _words(got["mean_square"]) == _words(li["mean_square"]), (b, got, li)
            for k in ("loudness", "max_momentary"):
                assert got[k] == li[k] if math.isinf(li[k]) else abs(got[k] - li[k]) <= 1e-12, (b, k, got, li)
    finally:
        e.close()
