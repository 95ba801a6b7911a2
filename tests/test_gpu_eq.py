"""GPU: the equaliser (vx_eq, csrc/eq.hip) against tests/_eq_refs.py, the numpy restatement of the header's contract, on the
coefficients the library designs.

Outputs, counts and peaks are compared word for word: the contract fixes every operation of the recursion and where every lane starts
it, so there is no tolerance anywhere.  S and W come from vx_eq_plan and are never written down here.  One engine serves all tests (the
entry needs no weights; the last test also decodes twelve frames with it); the restatement of every row is computed once."""
import ctypes as C

import numpy as np
import pytest

from tests import _eq_refs as R
from vallex_amd import _capi
from vallex_amd._capi import VX_EINVAL, Engine, _ptr
from vallex_amd.utils.generation import Eq

pytestmark = pytest.mark.gpu

SENT_F = np.float32(-1.0e30)
INFO = ("warm", "nonfinite", "nonfinite_out", "peak")


@pytest.fixture(scope="module")
def eng():
    from tests._util import get_model
    return get_model(2, 0, 2.5, vocos=True).engine


@pytest.fixture(scope="module")
def filt():
    """name -> (sections, W); S"""
    S = Engine.eq_plan(R.IDENTITY)[1]
    eight = Eq.telephone() + Eq.presence() + Eq.peak(500.0, -6.0, 2.0) + Eq.peak(6000.0, 5.0, 3.0)
    f = {"rumble": Eq.rumble().sections(24000), "presence": Eq.presence().sections(24000), "eight": eight.sections(24000),
         "identity": R.IDENTITY, "shelf": Eq.high_shelf(1000.0, 24.0).sections(24000)}
    out = {k: (s, Engine.eq_plan(s)[0]) for k, s in f.items()}
    assert all(W == R.warm(s) for s, W in out.values()) and len(out["eight"][0]) == 8
    assert out["rumble"][1] > S + 1 and S > out["presence"][1]            # a warm-up that reaches in front of short rows, and one below S
    return out, S


def _same(got, want, tag=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=str(tag))


def _info_same(got, want, tag=""):
    assert {k: got[k] for k in INFO[:3]} == {k: want[k] for k in INFO[:3]}, (tag, got, want)
    assert np.float32(got["peak"]).view(np.uint32) == np.float32(want["peak"]).view(np.uint32), (tag, got, want)


def _lengths(S):
    return [1, S - 1, S, S + 1, 63 * S + 5, 64 * S, 64 * S + 1]


@pytest.fixture(scope="module")
def length_refs(filt):
    """the restatement of every length under both filters, from one noise row with a DC offset"""
    f, S = filt
    x = R.noise_row(64 * S + 1, seed=41, dc=0.3)
    return x, {(name, L): R.eq(x[:L], f[name][0], f[name][1], S) for name in ("rumble", "presence") for L in _lengths(S)}


@pytest.mark.parametrize("name", ["rumble", "presence"])
def test_lengths_word_for_word(eng, filt, length_refs, name):
    f, S = filt
    x, refs = length_refs
    for L in _lengths(S):                                                 # 64 S + 1: a second tile
        rows, infos = eng.eq([x[:L]], f[name][0], return_info=True)
        want, winfo = refs[(name, L)]
        _same(rows[0], want, (name, L))
        _info_same(infos[0], winfo, (name, L))
        assert eng.last_eq_info == infos and infos[0]["warm"] == f[name][1]
    assert eng.eq([], f[name][0]) == [] and eng.eq([], f[name][0], return_info=True) == ([], [])


def test_ragged_batch_word_for_word_and_nothing_behind_a_rows_end(eng, filt):
    f, S = filt
    s, W = f["eight"]
    rows = [R.noise_row(L, seed=50 + i, dc=0.1 * i) for i, L in enumerate((0, 777, 3 * S + 1))]
    got, infos = eng.eq(rows, s, return_info=True)
    for i, x in enumerate(rows):
        want, winfo = R.eq(x, s, W, S)
        _same(got[i], want, i)
        _info_same(infos[i], winfo, i)
        alone, ainfo = eng.eq([x], s, return_info=True)                   # row bits equal the batch-1 bits
        _same(alone[0], got[i], i)
        _info_same(ainfo[0], infos[i], i)
    assert infos[0] == dict(warm=W, nonfinite=0, nonfinite_out=0, peak=0.0) and len(got[0]) == 0
    # the library itself, into a buffer of sentinels with a longer stride: elements behind a row's end are not written
    stride = max(len(x) for x in rows)
    ostride = stride + 8
    buf = np.zeros((3, stride), np.float32)
    for i, x in enumerate(rows):
        buf[i, : len(x)] = x
    lens = np.array([len(x) for x in rows], np.int32)
    out = np.full((3, ostride), SENT_F, np.float32)
    info = (_capi.vx_eq_info * 3)()
    assert eng.lib.vx_eq(eng.ctx, _ptr(buf, C.c_float), stride, _ptr(lens, C.c_int32), 3, _ptr(s, C.c_double), 8, _ptr(out, C.c_float), ostride, info) == 0
    for i, x in enumerate(rows):
        _same(out[i, : len(x)], got[i], i)
        assert (out[i, len(x):] == SENT_F).all()


def test_a_row_cut_across_launches_gives_the_same_bits(eng, filt):
    f, S = filt
    x = R.noise_row(70 * S, seed=61, dc=-0.2)
    short = R.noise_row(777, seed=62)
    for name in ("rumble", "presence"):
        s, W = f[name]
        whole, winfo = eng.eq([short, x], s, return_info=True)
        _same(whole[1], R.eq(x, s, W, S)[0], name)
        assert W + S <= _capi.DEV_EQ_WINDOW_MIN < len(x)                  # the row does not fit one launch at the smallest window
        eng.dev_eq_window(_capi.DEV_EQ_WINDOW_MIN)
        try:
            cut, cinfo = eng.eq([short, x], s, return_info=True)
        finally:
            eng.dev_eq_window(0)
        for i in range(2):
            _same(cut[i], whole[i], (name, i))
            _info_same(cinfo[i], winfo[i], (name, i))


def test_nonfinite_input_is_zero_and_counted(eng, filt):
    f, S = filt
    s, W = f["rumble"]
    x = R.noise_row(3 * S + 7, seed=71, dc=0.2)
    bad = [0, S - 1, S, 2 * S - 1, 2 * S, 2 * S + S // 2, 3 * S + 6]    # a step's first and last samples, one inside the warm-ups
    x[bad] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan]
    got, infos = eng.eq([x], s, return_info=True)
    want, winfo = R.eq(x, s, W, S)
    _same(got[0], want)
    _info_same(infos[0], winfo)
    assert infos[0]["nonfinite"] == len(bad) and infos[0]["nonfinite_out"] == 0 and np.isfinite(got[0]).all()
    clean = x.copy()
    clean[bad] = 0
    _same(eng.eq([clean], s)[0], got[0])                                  # zeros in
    allbad = np.full(S + 1, np.nan, np.float32)
    got, infos = eng.eq([allbad], s, return_info=True)
    assert infos[0]["nonfinite"] == S + 1 and infos[0]["peak"] == 0.0 and not got[0].any()


def test_nonfinite_result_is_written_as_zero_and_counted(eng, filt):
    f, S = filt
    s, W = f["shelf"]
    hot = np.full(S // 2, 3e38, np.float32)
    hot[1::2] *= -1                                                       # the top of the band, where the shelf gives +24 dB
    x = np.concatenate([R.noise_row(S + 5, seed=75), hot, R.noise_row(S, seed=76)])
    got, infos = eng.eq([x], s, return_info=True)
    want, winfo = R.eq(x, s, W, S)
    _same(got[0], want)
    _info_same(infos[0], winfo)
    assert S // 4 < infos[0]["nonfinite_out"] < S and infos[0]["nonfinite"] == 0 and np.isfinite(got[0]).all()
    assert (got[0] == 0).sum() == infos[0]["nonfinite_out"] and 0 < infos[0]["peak"] < np.inf and infos[0]["peak"] == np.abs(got[0]).max()


def test_identity_returns_the_input_bits(eng, filt):
    f, S = filt
    x = R.noise_row(2 * S + 5, seed=81, dc=0.05)
    x[[3, S]] = [np.nan, -np.inf]
    got, infos = eng.eq([x], f["identity"][0], return_info=True)
    want = np.where(np.isfinite(x), x, np.float32(0))
    _same(got[0], want)
    _info_same(infos[0], dict(warm=f["identity"][1], nonfinite=2, nonfinite_out=0, peak=np.abs(want).max()))
    _same(eng.eq([x], np.tile(R.IDENTITY, (8, 1)))[0], want)


def test_argument_errors(eng, filt):
    f, S = filt
    s, W = f["rumble"]
    x = R.noise_row(S, seed=91)
    out = np.full(S, SENT_F, np.float32)
    lens = np.array([S], np.int32)
    info = (_capi.vx_eq_info * 1)()
    px, po, pl, ps = _ptr(x, C.c_float), _ptr(out, C.c_float), _ptr(lens, C.c_int32), _ptr(s, C.c_double)
    unstable = np.array([[1.0, 0.0, 0.0, 0.0, 1.0]])
    nan = np.array([[1.0, np.nan, 0.0, 0.0, 0.0]])
    notch = Engine.eq_design("notch", 50.0, 100.0)[None]
    neg = np.array([-1], np.int32)
    for args, why in (((None, S, pl, 1, ps, 1, po, S, info), "wav"), ((px, S, None, 1, ps, 1, po, S, info), "lens"),
                      ((px, S, pl, 0, ps, 1, po, S, info), "batch"), ((px, S, pl, 1, None, 1, po, S, info), "sections"),
                      ((px, S, pl, 1, ps, 1, None, S, info), "out"), ((px, S, pl, 1, ps, 1, po, S, None), "info"),
                      ((px, S - 1, pl, 1, ps, 1, po, S, info), "wav_stride"), ((px, S, pl, 1, ps, 1, po, S - 1, info), "out_stride"),
                      ((px, S, _ptr(neg, C.c_int32), 1, ps, 1, po, S, info), "lens"),
                      ((px, S, pl, 1, ps, 0, po, S, info), "nsections 0"), ((px, S, pl, 1, ps, 9, po, S, info), "nsections 9"),
                      ((px, S, pl, 1, _ptr(unstable, C.c_double), 1, po, S, info), "section 0 is unstable"),
                      ((px, S, pl, 1, _ptr(nan, C.c_double), 1, po, S, info), "section 0: coefficient 1"),
                      ((px, S, pl, 1, _ptr(notch, C.c_double), 1, po, S, info), "memory is too long")):
        assert eng.lib.vx_eq(eng.ctx, *args) == VX_EINVAL, why
        assert why in eng.lib.vx_last_error(eng.ctx).decode(), (why, eng.lib.vx_last_error(eng.ctx))
        assert (out == SENT_F).all()                                      # nothing written
    with pytest.raises(ValueError, match="too long"):
        eng.eq([x], notch)
    for bad in (1, _capi.DEV_EQ_WINDOW_MIN - 1, _capi.EQ_WINDOW + 1, -5):
        with pytest.raises(_capi.VallexHipError, match="vx_dev_eq_window"):
            eng.dev_eq_window(bad)
    long_memory = Engine.eq_design("highpass", 20.0, 0.7071, 0.0, 48000)[None]      # W + S above the smallest window: refused, not widened
    assert Engine.eq_plan(long_memory)[0] + S > _capi.DEV_EQ_WINDOW_MIN
    eng.dev_eq_window(_capi.DEV_EQ_WINDOW_MIN)
    try:
        with pytest.raises(_capi.VallexHipError, match="vx_dev_eq_window"):
            eng.eq([x], long_memory)
    finally:
        eng.dev_eq_window(0)
    _same(eng.eq([x], long_memory)[0], R.eq(x, long_memory, R.warm(long_memory), S)[0])


def test_vocos_decode_with_an_eq_is_the_stages_one_by_one(eng):
    from tests._util import golden
    codes = [golden("nl2_bestof3")["codes"][0].astype(np.int64)]
    assert codes[0].shape == (12, 8)
    w24 = [w.copy() for w in eng.vocos_decode(codes, 2)]
    tele = Eq.telephone()
    want = eng.resample(eng.eq(w24, tele.sections(24000)), 24000, 8000)
    got = eng.vocos_decode(codes, 2, eq=tele, sample_rate=8000)
    assert len(got) == 1 and len(got[0]) == 12 * 320 // 3
    _same(got[0], want[0])
    assert eng.last_eq_info[0]["warm"] == Engine.eq_plan(tele)[0] and eng.last_eq_info[0]["peak"] > 0
    plain = eng.vocos_decode(codes, 2, sample_rate=8000)
    _same(eng.vocos_decode(codes, 2, sample_rate=8000, eq=None)[0], plain[0])
    _same(plain[0], eng.resample(w24, 24000, 8000)[0])
    assert np.abs(got[0] - plain[0]).max() > 0                            # the band did change the delivered waveform
    with pytest.raises(ValueError, match="too long"):
        eng.vocos_decode(codes, 2, eq=Eq.notch(50.0, 100.0))
