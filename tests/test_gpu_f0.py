"""GPU: the pitch tracker (vx_f0, csrc/f0.hip) against tests/_f0_refs.py, the numpy restatement of the header's contract.

Everything is compared word for word: the difference d and its normalisation d' of every frame as doubles, the lags, the candidates,
the aperiodicities and the summaries.  Nothing goes through a transcendental or a library that could differ, so there is no tolerance
anywhere except where the RESTATEMENT is held to the tones' true frequencies.  One un-finalized context serves all tests: the entry
needs no weights.  The restatement of every case is computed once and shared.

Accuracy, measured on the CPU with the restatement alone (docs/log_r26.md): at 8 kHz, hop 40, window 100, lags 8 .. 67, threshold
0.15, five-harmonic tones of 483 samples at 130, 150, 200, 310, 440 and 620 Hz are voiced in every interior frame (frames 2 .. 9: the
window reaches no padding) and the worst candidate is 4.5455 cents off (440 Hz: a period of 18.2 samples); the test allows twice that."""
import ctypes as C

import numpy as np
import pytest

from tests import _f0_refs as R
from vallex_amd import _capi
from vallex_amd._capi import VX_EINVAL, Engine, VallexHipError, _ptr

pytestmark = pytest.mark.gpu

SENT_F = np.float32(-1.0e30)
SENT_I = -123456789
TONES = (130.0, 150.0, 200.0, 310.0, 440.0, 620.0)
WORST_CENTS = 4.5455                     # of the restatement on TONES at R.SMALL, interior frames (measured on the CPU)
STRIDED = (8000, 1000, 100, 8, 67, 0.15)      # a hop far above the window: 12 frames span 12 000 samples


@pytest.fixture(scope="module")
def eng():
    e = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)      # created, never finalized
    yield e
    e.close()


def _rows(opts):
    H = opts[1]
    if opts == R.SMALL:
        return R.rows(40) + [R.hot_row(483), np.zeros(200, np.float32), R.huge_row(331), R.tone(200.0, 8000, 483)]
    if opts == R.TINY:
        return R.rows(16) + [R.hot_row(100), np.zeros(33, np.float32), R.tone(8000.0 / 3.0, 8000, 100, harmonics=1)]
    return [R.tone(101.0, opts[0], 2 * H + 5)]


@pytest.fixture(scope="module")
def ref():
    """per option set: the rows and the restatement (f0, lag, ap, info, d, d') of each"""
    out = {}
    for opts in (R.SMALL, R.TINY, R.LARGEST):
        rows = _rows(opts)
        out[opts] = (rows, [R.f0(x, opts, tables=True) for x in rows])
    return out


def _opts(o):
    return _capi.vx_f0_opts(C.sizeof(_capi.vx_f0_opts), int(o[0]), int(o[1]), int(o[2]), int(o[3]), int(o[4]), float(o[5]))


def _raw(eng, rows, opts, pad=5, with_ap=True, **kw):
    """vx_f0 on sentinel-filled outputs: (rc, message, f0, lag, ap (n, stride + pad), info structs)"""
    n = len(rows)
    ln = np.array([len(r) for r in rows], np.int32)
    ws = max(1, int(ln.max()))
    buf = np.zeros((n, ws), np.float32)
    for i, r in enumerate(rows):
        buf[i, : len(r)] = r
    fs = max(1, R.frames(ws, max(1, opts.hop))) + pad
    f, lag, ap = np.full((n, fs), SENT_F, np.float32), np.full((n, fs), SENT_I, np.int32), np.full((n, fs), SENT_F, np.float32)
    info = (_capi.vx_f0_info * n)()
    for w in info:
        w.frames = SENT_I
    a = dict(wav=_ptr(buf, C.c_float), wav_stride=ws, lens=_ptr(kw.pop("lens_arr", ln), C.c_int32), batch=n, o=C.byref(opts),
             f0=_ptr(f, C.c_float), lag=_ptr(lag, C.c_int32), ap=_ptr(ap, C.c_float) if with_ap else None, frame_stride=fs, info=info)
    a.update(kw)
    rc = eng.lib.vx_f0(eng.ctx, a["wav"], a["wav_stride"], a["lens"], a["batch"], a["o"], a["f0"], a["lag"], a["ap"], a["frame_stride"],
                       a["info"])
    return rc, eng.lib.vx_last_error(eng.ctx).decode(), f, lag, ap, info


def _info(w):
    return {fl[0]: getattr(w, fl[0]) for fl in _capi.vx_f0_info._fields_}


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    view = {4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize]
    np.testing.assert_array_equal(a.view(view), b.view(view), err_msg=str(what))


def _check_batch(out, want, what):
    rc, msg, f, lag, ap, info = out
    assert rc == 0, msg
    for i, (wf, wl, wa, wi, _, _) in enumerate(want):
        m = len(wf)
        _same(f[i, :m], wf, (what, "f0", i))
        _same(lag[i, :m], wl, (what, "lag", i))
        _same(ap[i, :m], wa, (what, "ap", i))
        assert (f[i, m:] == SENT_F).all() and (lag[i, m:] == SENT_I).all() and (ap[i, m:] == SENT_F).all(), (what, i)    # nothing behind M
        assert _info(info[i]) == wi, (what, i, _info(info[i]), wi)


@pytest.mark.parametrize("opts", [R.SMALL, R.TINY], ids=["hop40_win100_lag8_67", "hop16_win16_lag2_3"])
def test_kernel_word_for_word_alone_and_as_one_ragged_batch(eng, ref, opts):
    rows, want = ref[opts]
    H = opts[1]
    assert [len(x) for x in rows[:6]] == [0, 1, H - 1, H, H + 1, 12 * H + 3]
    assert not np.isfinite(rows[6]).all() and not rows[7].any() and want[6][3]["nonfinite"] == 3
    o = _opts(opts)
    for i, (x, (wf, wl, wa, wi, wd, wdp)) in enumerate(zip(rows, want)):
        d, dp = eng.dev_f0_table(x, o)                                # the difference and its normalisation, as doubles
        _same(d, wd, (opts, i, "d"))
        _same(dp, wdp, (opts, i, "dp"))
        assert np.isfinite(d).all() and np.isfinite(dp).all()
        f, lag, ap, info = eng.f0_lags([x], o)                        # the row alone
        _same(f[0], wf, (opts, i, "f0"))
        _same(lag[0], wl, (opts, i, "lag"))
        _same(ap[0], wa, (opts, i, "ap"))
        assert info[0] == wi, (opts, i)
    _check_batch(_raw(eng, rows, o), want, opts)                      # all rows as one ragged batch
    out2 = _raw(eng, rows, o)                                         # two calls give the same bits
    _check_batch(out2, want, opts)
    rc, msg, f, lag, ap, info = _raw(eng, rows, o, with_ap=False)     # ap is optional
    assert rc == 0 and (ap == SENT_F).all()
    _same(lag, out2[3])
    _same(f, out2[2])
    # the all-zero row: unvoiced at lag_min, aperiodicity 1
    z = want[7]
    assert (z[1] == -opts[3]).all() and (z[2] == 1.0).all() and (z[0] == np.float32(opts[0] / opts[3])).all() and z[3]["f0_median"] == 0.0
    assert sum(w[3]["voiced_frames"] for w in want) >= (10 if opts == R.SMALL else 1)
    if opts == R.SMALL:
        assert 0 < want[8][4].max() < np.inf and want[8][4].max() > 1e77        # the +-3e38 row: sums far above fp32, finite in double


def test_largest_options(eng, ref):
    rows, want = ref[R.LARGEST]
    o = _opts(R.LARGEST)
    assert len(want[0][0]) == 3
    d, dp = eng.dev_f0_table(rows[0], o)
    _same(d, want[0][4], "d")
    _same(dp, want[0][5], "dp")
    _check_batch(_raw(eng, rows, o), want, "largest")
    try:                                                               # one frame per launch: the window holds exactly one reach
        eng.dev_f0_window(_capi.DEV_F0_WINDOW_MIN)
        _check_batch(_raw(eng, rows, o), want, "largest, window min")
        d, dp = eng.dev_f0_table(rows[0], o)
        _same(d, want[0][4], "d, window min")
        _same(dp, want[0][5], "dp, window min")
    finally:
        eng.dev_f0_window(0)


def test_a_row_alone_equals_the_row_among_seven_others(eng, ref):
    rows, want = ref[R.SMALL]
    o = _opts(R.SMALL)
    x = rows[5]
    alone = _raw(eng, [x], o)
    assert alone[0] == 0, alone[1]
    for at in (0, 3, 7):
        others = [rows[9], rows[6], rows[4], rows[8], rows[2], rows[7], rows[0]]
        batch = others[:at] + [x] + others[at:]
        got = _raw(eng, batch, o)
        assert got[0] == 0, got[1]
        m = len(want[5][0])
        for j in (2, 3, 4):
            _same(got[j][at, :m], alone[j][0, :m], (at, j))
        _same(got[2][at, :m], want[5][0])
        assert _info(got[5][at]) == _info(alone[5][0]) == want[5][3]


def test_windows(eng, ref):
    """a 12-frame row through several launches: the bits of one pass"""
    x = (R.tone(180.0, 8000, 12000) + 0.05 * R.noise(12000, 9)).astype(np.float32)
    o = _opts(STRIDED)
    want = R.f0(x, STRIDED, tables=True)
    assert len(want[0]) == 12 and want[3]["voiced_frames"] >= 8
    one = eng.f0_lags([x], o)
    d1, dp1 = eng.dev_f0_table(x, o)
    rows, wsm = ref[R.SMALL]
    try:
        for win in (_capi.DEV_F0_WINDOW_MIN, 7777):
            eng.dev_f0_window(win)                                     # 3 or 7 frames of this row per launch
            f, lag, ap, info = eng.f0_lags([x], o)
            d, dp = eng.dev_f0_table(x, o)
            for g, a, w in ((f[0], one[0][0], want[0]), (lag[0], one[1][0], want[1]), (ap[0], one[2][0], want[2]), (d, d1, want[4]),
                            (dp, dp1, want[5])):
                _same(g, a, win)
                _same(g, w, win)
            assert info[0] == one[3][0] == want[3]
            _check_batch(_raw(eng, [x, rows[5], x[:5000], rows[6]], o), [want, R.f0(rows[5], STRIDED, tables=True),
                                                                         R.f0(x[:5000], STRIDED, tables=True),
                                                                         R.f0(rows[6], STRIDED, tables=True)], ("ragged", win))
            _check_batch(_raw(eng, rows, _opts(R.SMALL)), wsm, ("small", win))
        for bad in (1, _capi.DEV_F0_WINDOW_MIN - 1, -5, _capi.F0_WINDOW + 1):
            with pytest.raises(VallexHipError) as ei:
                eng.dev_f0_window(bad)
            assert ei.value.code == VX_EINVAL and "samples" in str(ei.value)
    finally:
        eng.dev_f0_window(0)                                           # 0 restores the default


def test_accuracy_on_harmonic_tones(eng):
    rate, H, W, t0, T, thr = R.SMALL
    L = 12 * H + 3
    o = _opts(R.SMALL)
    xs = [R.tone(fr, rate, L) for fr in TONES]
    got = eng.f0_lags(xs, o)
    worst = 0.0
    for i, (fr, x) in enumerate(zip(TONES, xs)):
        f, lag, ap, info = R.f0(x, R.SMALL)                           # the restatement is the yardstick
        _same(got[0][i], f, fr)
        _same(got[1][i], lag, fr)
        _same(got[2][i], ap, fr)
        ks = R.interior(len(f), H, W, T, L)
        assert ks == list(range(2, 10))
        assert (lag[ks] > 0).all(), fr                                 # every interior frame is voiced
        err = float(np.abs(R.cents(f[ks], fr)).max())
        print(f"f0 accuracy: {fr} Hz worst {err:.4f} cents, ap <= {ap[ks].max():.5f}")
        assert err <= 2.0 * WORST_CENTS, (fr, err)
        worst = max(worst, err)
    assert worst >= 0.5 * WORST_CENTS                                  # the constant is the measurement, not a loose guess


def test_engine_f0_defaults(eng):
    x = R.tone(150.0, 24000, 4800)
    f, voiced, ap, info = eng.f0([x, x[:1000]])
    want = R.f0(x, (24000, 240, 600, 48, 400, 0.15))
    _same(f[0], want[0])
    assert (voiced[0] == (want[1] > 0)).all() and voiced[0].dtype == np.bool_ and info[0] == want[3]
    _same(ap[0], want[2])
    assert len(f[1]) == 5 and info[1]["frames"] == 5
    assert abs(float(R.cents(info[0]["f0_median"], 150.0))) < 1.0
    f2 = eng.f0([x], 24000, hop=480, window=700, fmin=80.0, fmax=400.0, threshold=0.2)[0]
    _same(f2[0], R.f0(x, (24000, 480, 700, 60, 300, 0.2))[0])
    assert eng.f0([]) == ([], [], [], [])
    with pytest.raises(ValueError):
        eng.f0([x], fmin=500.0, fmax=60.0)


def test_refusals_write_nothing(eng, ref):
    rows, _ = ref[R.SMALL]
    rows = rows[3:6]
    good = R.SMALL

    def refused(field, opts=None, **kw):
        rc, msg, f, lag, ap, info = _raw(eng, rows, _opts(good) if opts is None else opts, **kw)
        assert rc == VX_EINVAL and field in msg, (field, rc, msg)
        assert (f == SENT_F).all() and (lag == SENT_I).all() and (ap == SENT_F).all() and all(w.frames == SENT_I for w in info), field

    for field, at, bad in (("sample_rate", 0, 7999), ("sample_rate", 0, 192001), ("hop", 1, 15), ("hop", 1, 4097), ("window", 2, 15),
                           ("window", 2, 2049), ("lag_min", 3, 1), ("lag_min", 3, -8), ("lag_max", 4, 8), ("lag_max", 4, 1025),
                           ("threshold", 5, 0.0), ("threshold", 5, 1.5), ("threshold", 5, float("nan")), ("threshold", 5, float("inf")),
                           ("threshold", 5, -0.15)):
        o = list(good)
        o[at] = bad
        refused(field, _opts(o))
    o = _opts(good)
    o.struct_size -= 4
    refused("struct_size", o)
    for name in ("wav", "lens", "o", "f0", "lag", "info"):
        refused(name, **{name: None})
    refused("batch", batch=0)
    refused("batch", batch=-2)
    refused("lens", lens_arr=np.array([40, -1, 483], np.int32))
    refused("lens", lens_arr=np.array([40, 41, 484], np.int32))       # above wav_stride
    refused("frame_stride", frame_stride=12)                          # the last row has 13 frames
    rc, msg, f, lag, ap, info = _raw(eng, rows, _opts(good))          # and the context still works
    assert rc == 0, msg
    with pytest.raises(VallexHipError) as ei:
        eng.dev_f0_table(rows[0], _opts((8000, 40, 100, 8, 2000, 0.15)))
    assert ei.value.code == VX_EINVAL and "lag_max" in str(ei.value)
